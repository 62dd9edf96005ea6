"""The conditions tests/mesh_scan_cases.py promises of its inputs, on which tests/test_hip_mesh_sampling_scan.py rests,
and the evidence that those inputs have teeth: a model of the scan's tree without its running maximum
(tests/mesh_scan_model.py) breaks the ranged conditions, and on the exact meshes numpy's CDF and a reciprocal multiply
both hand probes to another face.  No GPU.  Run with -s for the counts."""
import numpy as np
import pytest

import mesh_sampling_oracle as oracle
import mesh_scan_cases as cases
import mesh_scan_model as model

EXACT = range(len(cases.EXACT_BATCHES))
RANGED = range(len(cases.RANGED))


def views(c):
    """(name, own F, v, f, kind, weight, cdf, uniforms) of each view of a batch, padding included"""
    return [(c["names"][b], int(c["own_faces"][b]), c["v"][b], c["f"][b], c["kind"][b], c["weight"][b], c["cdf"][b],
             c["uniforms"][b]) for b in range(cases.VIEWS)]


def every_view(batches, make):
    return [x for j in batches for x in views(make(j))]


def dead_run(w, lo, hi):
    """faces [lo, hi) have weight 0 and the run ends there on both sides"""
    return (w[lo:hi] == 0).all() and (lo == 0 or w[lo - 1] > 0) and (hi >= len(w) or w[hi] > 0)


@pytest.mark.parametrize("j", EXACT)
def test_exact_weights_are_the_oracles_integers_and_every_sum_stays_below_2_53(j):
    c = cases.exact_batch(j)
    assert c["v"].dtype == np.float32 and c["f"].shape[0] == cases.VIEWS and c["uniforms"].dtype == np.float64
    for name, own, v, f, kind, w, cdf, u in views(c):
        for n in (own, len(f)):                                         # alone with its own F, and padded in the batch
            got = oracle.face_quantities(v[:3 * n], f[:n], c["eye"])["weight"]
            assert np.array_equal(got, w[:n]), name
        assert np.array_equal(w, np.round(w)) and 0 < w.sum() < 2.0 ** 53
        assert np.array_equal(w > 0, kind < 0) and (w[own:] == 0).all()
        live = w[w > 0]
        assert (np.log2(live) == np.round(np.log2(live))).all()         # powers of two: area2 is one exact product
        assert np.array_equal(cdf[:own], cases.exact_cdf(w[:own])) and np.array_equal(cdf, cases.exact_cdf(w))
        assert (np.diff(cdf) >= 0).all() and cdf[-1] == 1.0
        assert np.array_equal(cdf[1:][w[1:] == 0], cdf[:-1][w[1:] == 0])
        # without the eye the flipped faces would count: the cull is what removes them
        assert (oracle.face_quantities(v, f, None)["weight"][kind == 1] > 0).all()


def test_every_pattern_and_every_kind_of_zero_weight_face_occurs():
    all_views = every_view(EXACT, cases.exact_batch)
    T, W = cases.TILE, cases.WAVE
    own = {name: w[:n] for name, n, _v, _f, _k, w, _c, _u in all_views}
    assert sorted({len(w) for w in own.values()}) == [1023, 1024, 1025, 2048, 2049, 3 * 1024 + 5]
    some = lambda test: any(test(w) for w in own.values())              # noqa: E731
    assert some(lambda w: dead_run(w, 0, cases.LANE))                   # a lane's four faces, at the head
    assert some(lambda w: dead_run(w, W, 2 * W))                        # a wave's share of the tile
    assert some(lambda w: len(w) > 2 * T and dead_run(w, T, 2 * T))     # a whole tile
    assert some(lambda w: len(w) > T + 5 and dead_run(w, T - 4, T + 5))  # the seam
    # the tail from the last positive face to F - 1, across a seam
    assert some(lambda w: (w > 0).sum() > 1 and np.flatnonzero(w > 0)[-1] < T <= len(w) - 1)
    assert some(lambda w: np.flatnonzero(w > 0)[0] >= (len(w) - 1) // T * T)          # positive in the last tile only
    assert some(lambda w: len(w) > 2 * T and 1 < (w > 0).sum() and np.flatnonzero(w > 0)[-1] < T)   # in the first only
    assert some(lambda w: len(w) == 2049 and list(np.flatnonzero(w > 0)) == [T])
    assert some(lambda w: w[w > 0].max() / w[w > 0].min() >= 2.0 ** 30)
    kinds = np.concatenate([k for _n, _o, _v, _f, k, _w, _c, _u in all_views])
    assert {0, 1, 2} <= set(kinds)
    for _name, n, v, f, kind, _w, _c, _u in all_views:
        assert (f[kind == 0, 0] == f[kind == 0, 1]).all()
        assert np.isnan(v[f[kind == 2]]).any(axis=(1, 2)).all() and not np.isnan(v[f[kind != 2]]).any()
        # each of the three kinds stands in every dead run of a lane or more of the view itself
        if dead_run(_w[:n], 0, cases.LANE):
            assert {0, 1, 2} <= set(kind[:cases.LANE])


@pytest.mark.parametrize("j", EXACT)
def test_every_boundary_probe_has_a_positive_weight_face_and_sits_on_or_just_below_a_cdf_value(j):
    c = cases.exact_batch(j)
    for name, own, _v, _f, _kind, w, cdf, u in views(c):
        r0 = u[:, 0]
        assert (u >= 0).all() and (u < 1).all()
        face = cases.expected_faces(cdf, r0)
        assert (face < own).all() and (w[face] > 0).all(), name
        assert np.array_equal(face, cases.expected_faces(cdf[:own], r0))           # the padding changes nothing
        live = np.flatnonzero(w > 0)
        values = cdf[live[:-1]]
        assert np.isin([0.0, cases.LAST], r0).all() and np.isin(values, r0).all()
        assert np.isin(np.nextafter(values, 0.0), r0).all()
        on = np.isin(r0, values)
        assert np.array_equal(face[on], live[1:][np.searchsorted(values, r0[on])])  # on a value: the next positive face
        below = np.isin(r0, np.nextafter(values, 0.0)) & ~on
        assert np.array_equal(face[below], live[:-1][np.searchsorted(values, r0[below])])   # one ulp below: its own
        assert face[r0 == 0].tolist() == [live[0]] * int((r0 == 0).sum())
        assert (face[r0 == cases.LAST] == live[-1]).all()
        assert len(np.unique(r0)) >= 2 * len(values)                    # distinct values, distinct probes


@pytest.mark.parametrize("j", EXACT)
def test_on_the_exact_meshes_numpys_cdf_and_a_reciprocal_multiply_pick_other_faces(j):
    c = cases.exact_batch(j)
    for name, own, _v, _f, _kind, w, cdf, u in views(c):
        w, cdf, r0 = w[:own], cdf[:own], np.unique(u[:, 0])
        want = cases.expected_faces(cdf, r0)
        total = w.sum()
        others = {"numpy": oracle.cdf_numpy(w), "reciprocal": np.cumsum(w) * (1.0 / total)}
        counts = {k: int((cases.expected_faces(a, r0) != want).sum()) for k, a in others.items()}
        differ = {k: float((a != cdf).mean()) for k, a in others.items()}
        print(f"{name}: of {len(r0)} probes numpy's CDF gives {counts['numpy']} another face "
              f"({differ['numpy']:.0%} of its entries differ), a reciprocal multiply "
              f"{counts['reciprocal']} ({differ['reciprocal']:.0%})")
        if (w > 0).sum() > 16:                                          # a view of one or five faces may agree by luck
            assert counts["numpy"] > 0 and counts["reciprocal"] > 0, name


@pytest.mark.parametrize("j", EXACT)
def test_the_model_with_the_running_maximum_gives_the_exact_cdf(j):
    c = cases.exact_batch(j)
    for name, own, _v, _f, _kind, w, cdf, _u in views(c):
        for n in (own, len(w)):
            got = model.cdf(w[:n])
            assert np.array_equal(got, cdf[:n]), name
            assert np.array_equal(model.cdf(w[:n], running_max=False), cdf[:n]), name   # integers: any tree is exact


@pytest.mark.parametrize("j", RANGED)
def test_ranged_shares_are_wide_enough_that_a_probe_has_at_most_two_acceptable_faces(j):
    c = cases.ranged_batch(j)
    n = cases.RANGED[j]
    tol = cases.tol(n)
    assert tol == (2 * n + 2) * 2.0 ** -53
    for name, own, v, f, kind, w, cdf, u in views(c):
        assert own == n == len(f)
        assert np.array_equal(oracle.face_quantities(v, f, c["eye"])["weight"], w)      # area2 = the leg, exactly
        assert np.array_equal(w > 0, kind < 0) and 0.25 < (w == 0).mean() < 0.35 and {0, 1, 2} <= set(kind)
        assert ((w == 0) & (np.arange(n) % cases.LANE == 0)).any()
        assert w[w > 0].max() / w[w > 0].min() > 2.0 ** 15
        assert np.array_equal(cdf, cases.fraction_cdf(w)) and cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all()
        share = w[w > 0] / w.sum()
        assert share.min() > 2 * tol + 16 * 2.0 ** -53, (name, share.min())
        # every double within 4 ulp of every CDF value is a probe
        r0 = u[:, 0]
        for value in (cdf[0], cdf[n // 2], cdf[np.flatnonzero(w > 0)[-2]]):
            near = value
            for _ in range(cases.ULPS):
                near = np.nextafter(near, 0.0)
                assert near in r0
            assert value in r0 and np.nextafter(value, 1.0) in r0
        assert 0.0 in r0 and cases.LAST in r0
        live, lo, hi = cases.acceptable_bounds(cdf, w)
        count = np.searchsorted(lo - tol, r0, side="right") - np.searchsorted(hi + tol, r0, side="right")
        assert count.min() >= 1 and count.max() <= 2, (name, count.min(), count.max())
        # and any fixed-order scan is within tol of the exact CDF: the model's, numpy's and a plain sum are
        for other in (model.cdf(w), oracle.cdf_numpy(w), oracle.cdf_plain(w)):
            assert np.abs(other - cdf).max() <= tol


@pytest.mark.parametrize("j", RANGED)
def test_the_model_without_the_running_maximum_breaks_the_ranged_conditions(j):
    c = cases.ranged_batch(j)
    for name, _own, _v, _f, _kind, w, cdf, u in views(c):
        good = model.cdf(w)
        assert (np.diff(good) >= 0).all() and good[-1] == 1.0
        assert np.array_equal(good[1:][w[1:] == 0], good[:-1][w[1:] == 0])
        bad = model.cdf(w, running_max=False)
        moved = int((bad[1:][w[1:] == 0] != bad[:-1][w[1:] == 0]).sum())
        drops = int((np.diff(bad) < 0).sum())
        # the GPU test's conditions, put to the faulty CDF: a zero-weight face is chosen, or the order is broken
        r0 = np.sort(u[:, 0])
        face = np.minimum(cases.expected_faces(bad, r0), len(w) - 1)
        chosen_dead = int((w[face] == 0).sum())
        print(f"{name}: without the maximum {moved} zero-weight faces leave their predecessor's value, {drops} prefixes "
              f"decrease, {chosen_dead} of {len(r0)} probes select a zero-weight face")
        assert moved >= 1 and drops >= 1, name
        assert chosen_dead >= 1, name
