"""CPU pins of tests/backward_run_cases.py, from the oracles' frames alone: every run and merge feature the GPU test
(tests/test_hip_backward_runs.py) relies on is present in at least one case, slab or view, with margins that leave
the GPU no choice of winner -- so no GPU result can skip or soften a case."""
import numpy as np
import pytest

import backward_run_cases as B
from oracle import np_oracle, torch_oracle


@pytest.fixture(scope="module")
def frames():
    """{name: (scene, nearest, hit)} under numpy shading, margins asserted under both shadings."""
    out = {}
    for name, scene in B.cases().items():
        for tch in (False, True):
            nearest, hit, gap, clip, light = B.margins(scene, tch)
            print(f"{name} torch={tch}: winner gap {gap:.3g}  clip gap {clip:.3g}  nearest light {light:.3g}")
            assert gap >= 1e-3, f"{name}: a winner within {gap:.3g} of the runner-up"
            assert clip >= 1e-3, f"{name}: an intersection within {clip:.3g} of near / far"
            assert light >= 1e-3, f"{name}: a hit {light:.3g} from a light"
            if tch:
                assert np.array_equal(hit, out[name][2]) and np.array_equal(nearest[hit], out[name][1][hit])
            else:
                out[name] = (scene, nearest, hit)
    return out


def _features(scene, nearest, hit, row0=0, row1=None):
    kind, mat = B.primitive_table(scene)
    return B.run_features(nearest, hit, row0, nearest.shape[1], row1, kind, mat)


def test_every_feature_is_present(frames):
    found = {}
    for name, (scene, nearest, hit) in frames.items():
        slabs = [(0, None)] + (list(B.SLABS) if name == "129x9" else [])
        for row0, row1 in slabs:
            for f, where in _features(scene, nearest, hit, row0, row1).items():
                found.setdefault(f, []).append((name, row0, row1, where[0]))
    for f in B.FEATURES:
        print(f, found.get(f, [])[:3])
    assert not set(B.FEATURES) - set(found), sorted(set(B.FEATURES) - set(found))


def test_the_frames_and_slabs_hold_what_they_were_designed_for(frames):
    main = frames["129x9"]
    per_slab = {s: _features(*main, s[0], s[1]) for s in B.SLABS}
    whole = _features(*main)
    assert "merge" in per_slab[(2, 6)] and "merge" not in whole           # row0 regroups the rows
    assert (0, 0) in per_slab[(2, 6)]["merge"] and (1, 0) in per_slab[(2, 6)]["foreign_lane0"]
    assert (2, 0) in per_slab[(2, 6)]["edge_live1"]
    assert "two_two" in whole and "three_one" in per_slab[(1, 9)] and "three_one" in per_slab[(3, 8)]
    assert "dead_rows_3" in per_slab[(0, 1)] and "dead_rows_2" in per_slab[(2, 8)] and "dead_rows_1" in per_slab[(2, 9)]
    assert {"run1_lane0", "run1_lane63", "run1_inside", "run2", "cross_wave", "repeat_other"} <= set(whole)
    assert "foreign_lane31" in _features(*frames["65x5"]) and "early_exit" in _features(*frames["65x5"])
    assert "foreign_wave0" in _features(*frames["64x4a"]) and "foreign_lane63" in _features(*frames["64x4b"])
    assert "wave0_miss" in _features(*frames["64x4c"]) and "run63" in _features(*frames["64x4d"])
    assert "repeat_miss" in _features(*frames["63x3"]) and "edge_live63" in _features(*frames["63x4"])
    assert {f.shape for f in (frames[k][1] for k in ("129x9", "65x5", "63x3", "64x4a", "1x7", "1x1"))} == \
        {(9, 129), (5, 65), (3, 63), (4, 64), (7, 1), (1, 1)}


def test_single_pixel_primitives_and_sphere_radius(frames):
    """At least eight primitives of every kind win exactly one pixel: eight discs, spheres and triangles in 129x9
    alone, the eight planes of 1x7 and 1x1 (a plane is unbounded: it wins one pixel only where it is all there is);
    every sphere run has a radius term."""
    singles = dict.fromkeys(B.KINDS, 0)
    for name, (scene, nearest, hit) in frames.items():
        kind, _ = B.primitive_table(scene)
        per_kind = np.bincount(kind[B.single_pixel_primitives(nearest, hit)], minlength=4)
        for k, n in zip(B.KINDS, per_kind):
            singles[k] += int(n)
        if name == "129x9":
            assert all(per_kind[B.KINDS.index(k)] >= 8 for k in ("triangle", "disk", "sphere")), per_kind
        if "sphere" in scene["objects"]:
            H, W = hit.shape
            ref = np_oracle.render(scene)
            _, absolute = torch_oracle.gradient_terms(scene, np.ones((H, W, 3)), np.ones((H, W)), ref=ref)
            assert np.all(absolute["sphere.radius"] > 0), name
    assert all(n >= 8 for n in singles.values()), singles


def test_lights_and_materials():
    scene = B.cases()["129x9"]
    idx = list(scene["lights"]["color_idx"])
    assert len(idx) == 3 and len(set(idx)) == 2
    assert np.all(scene["materials"]["coeffs"][:, 2] <= 32) and np.all(scene["materials"]["coeffs"][:, 1] > 0)
    assert np.all(scene["lights"]["attenuation"].sum(axis=1) > 0) and np.all(scene["lights"]["ambient"] > 0)


def test_views_differ_by_a_non_multiple_of_64_columns():
    scene, cams, overrides = B.views_case()
    maps = []
    for cam in cams:
        sc = dict(scene, camera=cam)
        for tch in (False, True):
            nearest, hit, gap, clip, light = B.margins(sc, tch)
            assert gap >= 1e-3 and clip >= 1e-3 and light >= 1e-3
        maps.append(np.where(hit, nearest, -1))
    for s, m in zip(B.VIEW_SHIFTS[1:], maps[1:]):
        assert s % 64 and not np.array_equal(m, maps[0])
        a, b = (maps[0][:, :-s], m[:, s:]) if s > 0 else (maps[0][:, -s:], m[:, :s])
        assert np.array_equal(a, b), f"view shifted by {s} columns"
    assert [sorted(o) for o in overrides] == [[], ["lights.pos"], []]


def test_atomic_counts_of_a_merged_and_an_unmerged_slab(frames):
    scene, nearest, hit = frames["129x9"]
    kind, mat = B.primitive_table(scene)
    a = int(nearest[2, 0])
    merged, waves, _ = B.atomic_counts(nearest, hit, 2, 129, 6, len(kind), mat)
    assert merged[a] == 1 + 4 + 4 and waves == 12                        # one merge; a run per row beside the disc; column 128
    whole, waves, mats = B.atomic_counts(nearest, hit, 0, 129, None, len(kind), mat)
    assert whole[a] == 4 + 4 + 4 and waves == 27
    assert mats.sum() > waves                                             # some waves shade with several materials


@pytest.mark.parametrize("double_sided", [False, True])
def test_the_lights_shares_add_up_to_the_gradient(double_sided):
    """gradient_terms_tch(only_light=l): the shares of the three lights in the image path's terms add up to the whole
    term, entry by entry, and their absolute sums are no smaller than the whole's."""
    scene = B.cases()["65x5"]
    W, H = scene["camera"]["viewport"][2:]
    g = np.random.RandomState(2).uniform(-1, 1, size=(H, W, 3))
    kw = dict(grad_image=g, double_sided=double_sided)
    total, absolute = torch_oracle.gradient_terms_tch(scene, **kw)
    shares = [torch_oracle.gradient_terms_tch(scene, only_light=l, **kw) for l in range(3)]
    want = torch_oracle.gradients_tch(scene, **kw)
    for key in total:
        summed = sum(s[0][key] for s in shares)
        spread = sum(s[1][key] for s in shares)
        # per row: a unit normal's gradient along the normal is the 1e-9 residue of a projection of O(100) values
        row = spread.max(axis=-1, keepdims=True) if spread.ndim > 1 else spread
        assert np.all(np.abs(total[key] - want[key]) <= 1e-12 * row), key
        assert np.all(np.abs(summed - total[key]) <= 1e-12 * row), key
        assert np.all(spread >= absolute[key] * (1 - 1e-12)), key
