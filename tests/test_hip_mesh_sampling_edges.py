"""The edge branches of the mesh-sampling layer on the GPU, against tests/mesh_sampling_oracle.py alone (the reference
raises or returns NaN on most of these): the ends of the unit interval with zero-weight faces at the ends of f, s = 0
and t = 0, degenerate and non-finite faces among good ones, a fully culled view inside a batch, an unreferenced vertex,
the long face run and the long vertex fan of the backward, and vertices of 1e-30 next to 1e30.  Bounds as in
tests/mesh_sampling_checks.py; the upstream gradients have no zero, so a zero gradient is the layer's."""
import numpy as np
import pytest

import mesh_sampling_cases as cases
import mesh_sampling_oracle as oracle
from mesh_sampling_checks import check_view, run, uniforms_for, view_oracle

pytestmark = pytest.mark.gpu
LAST = np.nextafter(1.0, 0.0)


def upstreams(n_samples, seed):
    """g_pos, g_normal [S, 3] float32 with 0.25 <= |g| < 1"""
    rng = np.random.RandomState(88000 + seed)
    return [cases.f32(rng.uniform(0.25, 1, (n_samples, 3)) * rng.choice([-1, 1], (n_samples, 3))) for _ in range(2)]


def grid(n_faces, seed):
    v, f = cases.grid_mesh(n_faces, np.random.RandomState(seed))
    return cases.f32(v), f


def against_oracle(v, f, u, eye=None, seed=0, subnormal=False):
    g_pos, g_normal = upstreams(len(u), seed)
    got, T = run(v, f, u, eye, g_pos, g_normal), view_oracle(v, f, u, eye, g_pos, g_normal)
    check_view(got, T, None, "", subnormal)
    return got, T


def test_the_ends_of_the_unit_interval_skip_the_zero_weight_faces_at_the_ends_of_f():
    v, f = grid(6, 1)
    f = np.concatenate([[[0, 0, 1]], f, [[2, 3, 3]]])                   # duplicate-vertex faces first and last
    u = uniforms_for(v, f, 40, 11)
    u[:4, 0] = [0.0, LAST, 0.0, LAST]
    got, T = against_oracle(v, f, u, seed=1)
    assert list(got["face"][:4]) == [1, len(f) - 2, 1, len(f) - 2]
    assert got["face"].min() >= 1 and got["face"].max() <= len(f) - 2
    # and with an eye that culls the first and the last good face, the next ones
    flipped = f.copy()
    flipped[[1, len(f) - 2]] = flipped[[1, len(f) - 2]][:, ::-1]
    eye = v.mean(0).astype(np.float64) + [0.0, 0.0, 5.0]
    u = uniforms_for(v, flipped, 40, 12, eye)
    u[:2, 0] = [0.0, LAST]
    got, _ = against_oracle(v, flipped, u, eye, seed=2)
    assert list(got["face"][:2]) == [2, len(f) - 3]


def test_s_0_is_v0_exactly_and_t_0_has_no_third_corner():
    v, f = grid(12, 2)
    u = uniforms_for(v, f, 30, 21)
    u[:10, 1] = 0.0                                                     # s = 0: q = 0, bary = (1, 0, 0)
    u[10:20, 2] = 0.0                                                   # t = 0: bary = (1 - q, q, 0)
    u[20, 1:] = 0.0
    got, _ = against_oracle(v, f, u, seed=3)
    first = np.r_[0:10, 20]
    assert np.array_equal(got["pos"][first], v[f[got["face"][first], 0]])
    assert np.array_equal(got["bary"][first], np.tile(np.float32([1, 0, 0]), (11, 1)))
    assert (got["bary"][10:20, 2] == 0).all() and (got["bary"][10:20, 1] > 0).all()


def test_degenerate_faces_among_good_ones_are_never_chosen_and_get_exactly_zero_gradient():
    v, f = grid(20, 3)
    n = len(v)
    extra = cases.f32([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4],      # collinear: zero area
                       [0.5, 0.1, 0.3], [0.7, 0.2, 0.1]])                      # for the duplicate-vertex faces
    v = np.concatenate([v, extra])
    bad = [[n, n + 1, n + 2], [n + 3, n + 3, n + 4], [n + 4, n + 3, n + 4], [n + 3, n + 3, n + 3]]
    f = np.concatenate([bad[:1], f[:7], bad[1:3], f[7:], bad[3:]])
    bad_at = [0, 8, 9, len(f) - 1]
    u = uniforms_for(v, f, 300, 31)
    got, T = against_oracle(v, f, u, seed=4)
    assert not np.isin(got["face"], bad_at).any()
    assert (T["S_v"][n:] == 0).all() and (got["grad_v"][n:] == 0).all() and np.isfinite(got["grad_v"]).all()


def test_a_non_finite_face_is_never_chosen_and_does_not_poison_its_views_cdf():
    v, f = grid(20, 4)
    n = len(v)
    nan, inf = float("nan"), float("inf")
    extra = cases.f32([[nan, 0.1, 0.2], [0.3, inf, 0.1], [0.2, 0.5, -inf], [0.6, 0.6, 0.6]])
    v = np.concatenate([v, extra])
    bad = [[n, 0, 1], [2, n + 1, 3], [n + 3, 4, n + 2], [n, n + 1, n + 2]]       # each shares vertices with good faces
    f = np.concatenate([bad[:2], f[:9], bad[2:3], f[9:], bad[3:]])
    bad_at = [0, 1, 11, len(f) - 1]
    u = uniforms_for(v, f, 300, 41)
    u[:2, 0] = [0.0, LAST]
    eye = v[:n].mean(0).astype(np.float64) + [0.1, -0.2, 5.0]
    for e in (None, eye):
        got, T = against_oracle(v, f, u, e, seed=5)
        assert not np.isin(got["face"], bad_at).any() and np.isfinite(got["pos"]).all()
        assert (got["grad_v"][n:] == 0).all() and np.isfinite(got["grad_v"]).all()
    assert got["face"][0] == 2 and got["face"][1] == len(f) - 2


def test_a_fully_culled_view_inside_a_batch_is_nan_and_leaves_its_neighbours_alone():
    c = cases.regular(5)                                                # 64 faces, no eye of its own needed
    v, f = c["v"], c["f"]
    keep = v.reshape(-1, 3).astype(np.float64).mean(0) + [0.0, 0.0, 5.0]
    # view 1 sees only back faces: every face wound to face +z, the eye far below
    up = f.copy()
    q = oracle.face_quantities(v[1], f, keep)
    up[~q["keep"]] = up[~q["keep"]][:, ::-1]
    fs = np.stack([f, up, f])
    eyes = np.stack([keep, keep * [1, 1, -1] - [0, 0, 20.0], keep])
    assert not oracle.face_quantities(v[1], up, eyes[1])["keep"].any()
    u = np.stack([uniforms_for(v[b], fs[b], 65, 50 + b, eyes[b] if b != 1 else None) for b in range(3)])
    g_pos, g_normal = (np.stack(x) for x in zip(*[upstreams(65, 60 + b) for b in range(3)]))
    got = run(v, fs, u, eyes, g_pos, g_normal)
    assert (got["face"][1] == -1).all()
    for key in ("pos", "normal", "bary"):
        assert np.isnan(got[key][1]).all(), key
    assert (got["grad_v"][1] == 0).all()
    for b in range(3):
        check_view(got, view_oracle(v[b], fs[b], u[b], eyes[b], g_pos[b], g_normal[b]), b, f"view {b}")
    for b in (0, 2):                                                    # the neighbours: bit-equal to their solo calls
        solo = run(v[b], fs[b], u[b], eyes[b], g_pos[b], g_normal[b])
        for key in solo:
            assert np.array_equal(solo[key], got[key][b]), (key, b)
    # all three views culled: nothing but NaN, and no gradient
    got = run(v, up, u, eyes[1], g_pos, g_normal)
    assert (got["face"] == -1).all() and np.isnan(got["pos"]).all() and (got["grad_v"] == 0).all()


def test_a_vertex_no_face_references_gets_exactly_zero_gradient():
    v, f = grid(30, 6)
    lone = [0, 7, len(v) + 2]                                           # in front of, among and behind the used ones
    for at in lone:                                                     # ascending: each insertion is final
        v = np.insert(v, at, cases.f32([[0.3, 0.3, 9.0]]), axis=0)
        f = f + (f >= at)
    assert lone[-1] == len(v) - 1 and not np.isin(lone, f).any() and len(np.unique(f)) == len(v) - 3
    u = uniforms_for(v, f, 200, 61)
    got, T = against_oracle(v, f, u, seed=6)
    assert (T["S_v"][lone] == 0).all() and (got["grad_v"][lone] == 0).all()


def test_one_face_with_all_1300_samples():
    """the long face run of the backward: 1300 terms in one lane's sums"""
    v = cases.f32([[0.1, 0.2, 0.3], [1.3, 0.1, 0.2], [0.4, 1.1, 0.9]])
    f = np.array([[0, 1, 2]])
    u = cases.draw(71, 1300)
    got, T = against_oracle(v, f, u, seed=7)
    assert (got["face"] == 0).all()
    # among other faces: the run starts and ends inside the order
    v2, f2 = grid(8, 7)
    f2 = np.concatenate([f2[:3] + 3, [[0, 1, 2]], f2[3:] + 3])          # the one face in front of the grid's vertices
    v2 = np.concatenate([v * 40, v2])                                   # the big face takes nearly every sample
    u = uniforms_for(v2, f2, 1300, 72)
    got, _ = against_oracle(v2, f2, u, seed=8)
    assert (got["face"] == 3).sum() > 1200 and len(np.unique(got["face"])) > 1


def test_a_fan_of_1300_faces_around_one_vertex():
    """the long vertex gather of the backward: 1300 corners in one lane's sum"""
    n = 1300
    rng = np.random.RandomState(81)
    a = np.sort(rng.uniform(0, 2 * np.pi, n))
    ring = np.stack([np.cos(a), np.sin(a), 0.1 * rng.standard_normal(n)], 1) * rng.uniform(0.8, 1.2, (n, 1))
    v = cases.f32(np.concatenate([[[0.0, 0.0, 0.5]], ring]))
    k = np.arange(n)
    f = np.stack([np.zeros(n, int), 1 + k, 1 + (k + 1) % n], 1)
    f[::3] = f[::3][:, [1, 2, 0]]                                       # the hub is not always corner 0
    u = uniforms_for(v, f, 2000, 82)
    got, T = against_oracle(v, f, u, seed=9)
    # the hub's sum runs over all 1300 corners; several hundred of them carry a gradient
    assert len(np.unique(got["face"])) > 500 and T["S_v"][0].min() > 0


def test_vertices_of_1e_minus_30_next_to_1e30():
    """fp64 neither underflows nor overflows on float32 inputs; below float32's normal range the store is off by up to
    its spacing 2^-149, which the bound carries as an absolute term"""
    v, f = grid(8, 9)
    big = cases.f32((v - v.mean(0)) * 1e30)
    mixed = big.copy()
    mixed[[0, 3], 0] = 1e-30                                            # components of 1e-30 beside ones of 1e30
    mixed[[1, 4], 2] = -1e-30
    tiny = cases.f32((v - v.mean(0)) * 1e-30)
    both = cases.f32(np.concatenate([tiny[:5], big[5:]]))               # faces of 1e-60 beside faces of 1e60
    for n, vv in enumerate((mixed, tiny, both)):
        u = uniforms_for(vv, f, 120, 91 + n)
        got, T = against_oracle(vv, f, u, seed=10 + n, subnormal=True)
        assert np.isfinite(got["pos"]).all() and np.isfinite(got["normal"]).all() and np.isfinite(got["grad_v"]).all()
    got = run(np.stack([mixed, tiny, both]), f, np.stack([uniforms_for(x, f, 120, 91 + n) for n, x in
                                                           enumerate((mixed, tiny, both))]))
    assert (got["face"] >= 0).all()
