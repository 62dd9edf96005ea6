"""k_mesh_scan's CDF probed on its own values (tests/mesh_scan_cases.py): r0 ON a CDF value and one ulp below it on
meshes whose CDF is known exactly whatever the scan's tree, with zero-weight faces over a lane, a wave, a tile, the tile
seam and the tail at face counts around the tile; and every double within 4 ulp of every CDF value on meshes whose
sums round, held to conditions that name no tree.  The regular cases keep r0 2^-30 away from the CDF and see none of
this.  Values and gradients keep the bounds of tests/mesh_sampling_checks.py, against the oracle's barycentric and
gradients fed the EXPECTED faces (oracle.forward's numpy CDF is not the exact one).  Run with -s for the worst ratios."""
import numpy as np
import pytest

import mesh_sampling_oracle as oracle
import mesh_scan_cases as cases
from mesh_sampling_checks import check_view, run

pytestmark = pytest.mark.gpu
KEYS = ("face", "bary", "pos", "normal", "grad_v")


def truth(v, f, uniforms, face, g_pos, g_normal, eye):
    """the oracle's view (the layout of mesh_sampling_checks.view_oracle) with `face` given, not searched for"""
    v, f = oracle.widen(v), np.asarray(f, np.int64)
    q = oracle.face_quantities(v, f, eye)
    bary, s_bary = oracle.barycentric(uniforms)
    tri = v[f[face]]
    with np.errstate(invalid="ignore"):
        s_normal = (q["normal_terms"] / np.where(q["length"] > 0, q["length"], 1)[:, None])[face]
    T = {"face": face, "bary": bary, "S_bary": s_bary, "pos": np.sum(bary[..., None] * tri, axis=1),
         "S_pos": np.sum(np.abs(bary[..., None] * tri), axis=1), "normal": q["normal"][face], "S_normal": s_normal}
    T.update(oracle.gradients(v, f, face, bary, g_pos, g_normal))
    return T


def run_views(c, views):
    """the batch (a slice) or one of its views (an int) as the cases lay it out"""
    return run(c["v"][views], c["f"][views], c["uniforms"][views], c["eye"], c["g_pos"][views], c["g_normal"][views])


@pytest.mark.parametrize("j", range(len(cases.EXACT_BATCHES)))
def test_r0_on_a_cdf_value_and_one_ulp_below_it_selects_the_exact_face(j):
    c = cases.exact_batch(j)
    got = run_views(c, slice(None))
    worst = worst_g = 0.0
    for b in range(cases.VIEWS):
        name, own, w, cdf, r0 = c["names"][b], int(c["own_faces"][b]), c["weight"][b], c["cdf"][b], c["uniforms"][b][:, 0]
        want = cases.expected_faces(cdf, r0)
        face = got["face"][b]
        wrong = np.flatnonzero(face != want)
        assert len(wrong) == 0, (name, len(wrong), wrong[:8], face[wrong[:8]], want[wrong[:8]], r0[wrong[:8]])
        assert (w[face] > 0).all(), name
        # said without searchsorted: the ends, a value, and the double below it
        live = np.flatnonzero(w > 0)
        at = {x: k for k, x in enumerate(r0)}
        assert face[at[0.0]] == live[0] and face[at[cases.LAST]] == live[-1], name
        values = cdf[live[:-1]]
        assert np.array_equal(face[[at[x] for x in values]], live[1:]), name
        assert np.array_equal(face[[at[x] for x in np.nextafter(values, 0.0)]], live[:-1]), name
        T = truth(c["v"][b], c["f"][b], c["uniforms"][b], want, c["g_pos"][b], c["g_normal"][b], c["eye"])
        a, g = check_view(got, T, b, name)
        worst, worst_g = max(worst, a), max(worst_g, g)
        # a batch equals its views bit for bit ...
        solo = run_views(c, b)
        for key in KEYS:
            assert np.array_equal(solo[key], got[key][b]), (name, key)
        # ... and the view with its own F, without the zero-weight faces that pad it to the batch's
        if own < c["f"].shape[1]:
            alone = run(c["v"][b][:3 * own], c["f"][b][:own], c["uniforms"][b], c["eye"], c["g_pos"][b], c["g_normal"][b])
            for key in KEYS[:-1]:
                assert np.array_equal(alone[key], got[key][b]), (name, key, "own F")
            assert np.array_equal(alone["grad_v"], got["grad_v"][b][:3 * own]) and (got["grad_v"][b][3 * own:] == 0).all()
    print(f"{'/'.join(c['names'])}: {c['uniforms'].shape[1]} probes a view, every face exact; values {worst:.3g} of "
          f"their bound; gradients {worst_g:.3g} of theirs")


@pytest.mark.parametrize("j", range(len(cases.RANGED)))
def test_within_4_ulp_of_every_cdf_value_the_face_is_positive_ordered_and_within_tol_of_its_interval(j):
    c = cases.ranged_batch(j)
    n_faces = cases.RANGED[j]
    tol = cases.tol(n_faces)
    got = run(c["v"], c["f"], c["uniforms"], c["eye"])
    worst = 0.0
    for b in range(cases.VIEWS):
        name, w, cdf, r0, face = c["names"][b], c["weight"][b], c["cdf"][b], c["uniforms"][b][:, 0], got["face"][b]
        assert ((face >= 0) & (face < n_faces)).all(), name
        dead = np.flatnonzero(w[face] == 0)
        assert len(dead) == 0, (name, len(dead), face[dead[:8]], r0[dead[:8]])
        # r0 within tol of [cdf of the positive face in front, cdf of the face)
        live, lo, hi = cases.acceptable_bounds(cdf, w)
        k = np.searchsorted(live, face)
        assert np.array_equal(live[k], face)
        out = np.maximum(np.maximum(lo[k] - r0, r0 - hi[k]), 0.0)
        far = np.flatnonzero(out > tol)
        assert len(far) == 0, (name, len(far), face[far[:8]], r0[far[:8]], out[far[:8]] / tol)
        worst = max(worst, out.max() / tol)
        # monotone in r0, and one face for one r0
        order = np.argsort(r0, kind="stable")
        assert (np.diff(face[order]) >= 0).all(), name
        same = np.diff(r0[order]) == 0
        assert (np.diff(face[order])[same] == 0).all(), name
        assert face[r0 == 0.0].tolist() == [live[0]] * int((r0 == 0).sum()) and (face[r0 == cases.LAST] == live[-1]).all()
    solo = run(c["v"][1], c["f"][1], c["uniforms"][1], c["eye"])
    assert np.array_equal(solo["face"], got["face"][1])
    print(f"ranged F = {n_faces}: {c['uniforms'].shape[1]} probes a view; the farthest r0 lies {worst:.3g} of tol = "
          f"{tol:.3g} outside its face's exact interval")


def test_a_view_without_a_positive_weight_between_two_exact_views_of_2049_faces():
    c = cases.dead_view_batch()
    assert not (c["weight"][1] > 0).any() and c["f"].shape[1] == 2049
    assert not (oracle.face_quantities(c["v"][1], c["f"][1], c["eye"])["weight"] > 0).any()
    got = run_views(c, slice(None))
    assert (got["face"][1] == -1).all()
    for key in ("pos", "normal", "bary"):
        assert np.isnan(got[key][1]).all(), key
    assert (got["grad_v"][1] == 0).all()
    for b in (0, 2):
        want = cases.expected_faces(c["cdf"][b], c["uniforms"][b][:, 0])
        assert np.array_equal(got["face"][b], want), c["names"][b]
        check_view(got, truth(c["v"][b], c["f"][b], c["uniforms"][b], want, c["g_pos"][b], c["g_normal"][b], c["eye"]), b,
                   c["names"][b])
        solo = run_views(c, b)
        for key in KEYS:
            assert np.array_equal(solo[key], got[key][b]), (key, b)
    solo = run_views(c, 1)
    assert (solo["face"] == -1).all() and np.isnan(solo["pos"]).all() and (solo["grad_v"] == 0).all()
