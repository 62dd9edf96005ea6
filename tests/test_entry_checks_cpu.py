"""tests/entry_checks.py without a GPU: the helper's own edges, and that the per-entry bound sees what the array-scale
tolerance of tests/projection_checks.py cannot -- the reference's own float32 results, recorded beside its float64 ones in
the fixtures of the frame transforms, the point projection, the depth lift, the plane fit and the hard projection.

    (a) check: an error exactly at the bound and one float32 step beyond it, A == 0, NaN and infinity patterns, a
        subnormal reference, a float64 `got`
    (b) every ref32/* of frames, surfels and normals passes the old tolerance and FAILS the bound on at least 20 % of the
        finite entries of each row of SHARES.  20 % is a condition: it sits under the smallest share measured with an
        array-max scale, 31.5 %, and a per-entry A can only be smaller than that scale
    (c) hard projection: the recorded float32 means break the bound where many surfels share a pixel; the gradient is one
        division, correctly rounded in both precisions, so the two records are equal bit for bit and NO bound can tell
        float32 from fp64 there
    (d) every entry of every `magnitudes` is >= |ref|, and on the seeded cases the median of A / |ref| over the nonzero
        entries is below 2^8
    (e) the plane fit's ill-conditioned share: the entries on which the restatement's two summation orders differ by more
        than NORMALS_C64_CAP max|ref| / 4 are at most 1 % of a case (the committed cases have none)
The shares printed by (b) are recorded in profiles/entry_bounds.txt."""
import os

import numpy as np
import pytest

import camera_edge_cases as ce
import entry_checks as ec
import frames_cases as fc
import hard_projection_cases as hc
import normals_cases as nc
import normals_edge_cases as ne
import surfels_cases as sc
from conftest import GOLDEN_DIR
from projection_checks import ATOL_SCALE, RTOL

F32 = np.float32


def _load(sub, name):
    return np.load(os.path.join(GOLDEN_DIR, sub, name + ".npz"), allow_pickle=False)


# ---- (a) the helper's own edges --------------------------------------------------------------------------------------
def _at_bound(ref, A):
    """The largest float32 above `ref` that is still within the bound, and the next one."""
    b = ec.bound(ref, A)
    inside = F32(ref + b)
    if float(inside) - ref > b:
        inside = np.nextafter(inside, F32(-np.inf))
    return inside, np.nextafter(inside, F32(np.inf))


@pytest.mark.parametrize("ref,A", [(1.0, 1.0), (1.0, 2.0 ** 20), (-3.0, 7.5), (1e-3, 40.0), (0.0, 2.0 ** 17)])
def test_an_error_at_the_bound_passes_and_one_step_beyond_it_fails(ref, A):
    inside, beyond = _at_bound(ref, A)
    assert abs(float(inside) - ref) <= ec.bound(ref, A) < abs(float(beyond) - ref)
    assert ec.check(np.array([inside]), np.array([ref]), np.array([A])) <= 1.0
    with pytest.raises(AssertionError):
        ec.check(np.array([beyond]), np.array([ref]), np.array([A]))
    # the bound itself, as a number: 2^-24 |ref| + 2^-40 A + 2^-149
    assert ec.bound(ref, A) == 2.0 ** -24 * abs(ref) + 2.0 ** -40 * A + 2.0 ** -149
    assert ec.check(np.array([F32(ref)]), np.array([ref]), np.array([A])) <= 1.0            # the one store alone


def test_the_ratio_is_the_error_over_the_bound():
    ref, A = np.array([1.0, 2.0]), np.array([2.0 ** 22, 4.0])
    got = (ref + 0.5 * ec.bound(ref, A) * np.array([1.0, 0.0])).astype(F32)
    want = abs(float(got[0]) - 1.0) / ec.bound(1.0, 2.0 ** 22)
    assert ec.check(got, ref, A) == pytest.approx(want, rel=1e-12) and 0 < want <= 1


def test_an_entry_with_no_terms_is_exactly_zero():
    assert ec.check(np.zeros(3, F32), np.zeros(3), np.zeros(3)) == 0.0
    assert ec.check(np.array([-0.0], F32), np.zeros(1), np.zeros(1)) == 0.0
    with pytest.raises(AssertionError):
        ec.check(np.array([0.0, 1e-45], F32), np.zeros(2), np.zeros(2))            # the smallest subnormal is not 0
    with pytest.raises(AssertionError):
        ec.check(np.array([1.0], F32), np.array([1.0]), np.array([0.0]))            # A below |ref|: not a magnitude
    assert ec.check(np.array([1e-45], F32), np.zeros(1), np.array([1e-30])) <= 1.0  # A > 0 allows the one subnormal step


def test_non_finite_references_ask_for_the_same_pattern():
    ref = np.array([np.nan, np.inf, -np.inf, 1.0])
    A = np.array([np.nan, np.inf, np.inf, 1.0])
    assert ec.check(ref.astype(F32), ref, A) == 0.0
    for bad in ([np.inf, np.inf, -np.inf, 1.0], [np.nan, -np.inf, -np.inf, 1.0], [np.nan, np.nan, -np.inf, 1.0],
                [np.nan, np.inf, -np.inf, np.nan], [np.nan, np.inf, 3e38, 1.0], [1.0, np.inf, -np.inf, 1.0]):
        with pytest.raises(AssertionError):
            ec.check(np.array(bad, F32), ref, A)
    with pytest.raises(AssertionError):                                             # finite reference, infinite result
        ec.check(np.array([np.inf], F32), np.array([1.0]), np.array([1.0]))


def test_a_subnormal_reference_is_held_to_one_subnormal_step():
    ref = np.array([3.3 * 2.0 ** -149, 2.0 ** -130 * 1.37])
    A = np.abs(ref)
    got = ref.astype(F32)                                                           # rounds to a multiple of 2^-149
    assert abs(float(got[0]) - ref[0]) > 2.0 ** -24 * ref[0]                        # the relative term alone would refuse it
    assert ec.check(got, ref, A) <= 1.0
    with pytest.raises(AssertionError):
        ec.check(np.array([got[0] + F32(3 * 2.0 ** -149), got[1]], F32), ref, A)


def test_a_float64_result_is_refused_before_any_widening():
    ref = np.array([1.0, 2.0])
    with pytest.raises(AssertionError):
        ec.check(ref.copy(), ref, np.abs(ref))
    with pytest.raises(AssertionError):
        ec.check(ref.astype(np.float16), ref, np.abs(ref))
    assert ec.narrowed(ref).dtype == F32
    with pytest.raises(AssertionError):
        ec.narrowed(np.array([1.0 + 2.0 ** -30]))                                   # not a float32 value
    with pytest.raises(AssertionError):
        ec.check(np.zeros((2, 1), F32), np.zeros(2), np.zeros(2))                   # the shapes


def test_the_held_mask_leaves_the_pattern_checks_on_every_entry():
    ref, A = np.array([1.0, 1.0, np.nan]), np.array([1.0, 1.0, 1.0])
    got = np.array([1.0, 1.001, np.nan], F32)
    with pytest.raises(AssertionError):
        ec.check(got, ref, A)
    assert ec.check(got, ref, A, held=np.array([True, False, True])) == 0.0
    with pytest.raises(AssertionError):
        ec.check(np.array([1.0, 1.001, 0.0], F32), ref, A, held=np.array([True, False, False]))


# ---- (b) the recorded float32 results: the old tolerance passes them, the bound does not ---------------------------------
def _old_passes(ref32, want, values):
    scale = max(np.abs(want).max(), 1.0) if values else np.abs(want).max()
    return bool(np.all(np.abs(ref32.astype(np.float64) - want) <= RTOL * np.abs(want) + ATOL_SCALE * scale))


def _frames_values():
    for name in fc.GOLDEN_TRANSFORM:
        for d in fc.DIRECTIONS:
            npz, want, A = _load("frames", f"fr1_{name}_{d}"), fc.transform_expected(name, d)[0], fc.transform_magnitudes(name, d)[0]
            for k in want:
                yield f"{name} {d} {k}", npz["ref32/" + k], want[k], A[k], True
                if "ref32/one/" + k in npz.files:           # the unbatched function on the one view
                    yield f"{name} {d} {k} unbatched", npz["ref32/one/" + k], want[k][0], A[k][0], True
    for name in fc.GOLDEN_PROJECT:
        npz = _load("frames", "fr1_" + name)
        for coords, out in ((False, "plane"), (True, "px_coord")):
            yield (f"{name} {out}", npz["ref32/" + out], fc.project_expected(name, coords)[0][out],
                   fc.project_magnitudes(name, coords)[0][out], True)


def _surfels(grad):
    for name, variant in sc.ALL:
        npz = _load("surfels", "sf1_" + sc.tag(name, variant))
        want, A = sc.expected(name, variant)[grad], sc.magnitudes(name, variant)[grad]
        k = "depth" if grad else "pos"
        yield sc.tag(name, variant), npz["ref32/grad/depth" if grad else "ref32/pos"].reshape(want[k].shape), want[k], A[k], not grad


def _normals(grad):
    for name, variant in nc.ALL:
        npz = _load("normals", "nm1_" + nc.tag(name, variant))
        want = nc.expected(name, variant)[grad]["pos" if grad else "normal"]
        yield nc.tag(name, variant), npz["ref32/grad/pos" if grad else "ref32/normal"], want, np.abs(want).max(), not grad
        one = "ref32/unbatched/grad/pos" if grad else "ref32/unbatched/normal"
        if one in npz.files:                                # the unbatched function on the one view
            yield nc.tag(name, variant) + " unbatched", npz[one].reshape(want[0].shape), want[0], np.abs(want).max(), not grad


SHARES = {"frames, values": (_frames_values, ec.C), "normals, values": (lambda: _normals(0), ec.NORMALS_C64),
          "normals, gradients": (lambda: _normals(1), ec.NORMALS_C64), "surfels, values": (lambda: _surfels(0), ec.C),
          "surfels, gradients": (lambda: _surfels(1), ec.C)}


@pytest.mark.parametrize("row", list(SHARES))
def test_the_float32_reference_passes_the_old_tolerance_and_fails_the_entry_bound(row):
    rows, floor = SHARES[row]
    beyond = total = 0
    for tag, ref32, want, A, values in rows():
        assert ref32.dtype == F32 and np.all(np.isfinite(want)), tag
        assert _old_passes(ref32, want, values), (row, tag, "the old tolerance refuses the float32 record")
        n, t = ec.share_beyond(ref32, want, A, floor)
        beyond, total = beyond + n, total + t
    print(f"{row}: {beyond} of {total} float32 entries break the per-entry bound ({100.0 * beyond / total:.1f} %)")
    assert beyond >= 0.2 * total, (row, beyond, total)


def test_check_itself_refuses_a_float32_record():
    name, d = "t153_192", "to_cam"
    npz = _load("frames", f"fr1_{name}_{d}")
    with pytest.raises(AssertionError):
        ec.check(npz["ref32/pos"], fc.transform_expected(name, d)[0]["pos"], fc.transform_magnitudes(name, d)[0]["pos"])
    want = fc.transform_expected(name, d)[0]["pos"]
    assert ec.check(want.astype(F32), want, fc.transform_magnitudes(name, d)[0]["pos"]) <= 1.0      # fp64, stored once


# ---- (c) hard projection ---------------------------------------------------------------------------------------------
def test_the_float32_means_of_a_crowded_pixel_break_the_bound_and_the_gradient_cannot_tell():
    """Every occupied pixel of the cluster cases holds many surfels.  The gradient |g_out| / count is one correctly
    rounded division in float32 and in fp64-then-float32 alike (a float32 quotient of float32 operands is not doubly
    rounded through fp64: 53 >= 2 * 24 + 2), so the two records are equal bit for bit and no bound can separate float32
    from fp64 arithmetic on the gradient."""
    clusters = [n for n in hc.NAMES if "cluster" in n]
    assert clusters
    for name in hc.NAMES:
        npz = _load("hard_projection", "hp1_" + name)
        (want, want_g), (A, A_g) = hc.expected(name), hc.magnitudes(name)
        assert _old_passes(npz["ref32/out"], want["out"], True) and _old_passes(npz["ref32/grad/rgb"], want_g["rgb"], False)
        n, t = ec.share_beyond(npz["ref32/out"], want["out"], A["out"])
        print(f"hard projection {name}: {n} of {t} float32 means break the per-entry bound")
        if name in clusters:
            assert want["count"].max() >= 32 and n >= 1, (name, n)
        assert np.array_equal(npz["ref32/grad/rgb"], npz["ref64/grad/rgb"].astype(F32)), name
        assert ec.share_beyond(npz["ref32/grad/rgb"], want_g["rgb"], A_g["rgb"])[0] == 0
        assert ec.check(npz["ref32/grad/rgb"], want_g["rgb"], A_g["rgb"]) <= 1.0


# ---- (d) the scales bound their entries and are not loose ----------------------------------------------------------------
def _seeded():
    """(tag, want, A, per point): every array of every seeded case, camera gradients included."""
    for name in fc.TRANSFORM:
        for d in fc.DIRECTIONS:
            for i, (want, A) in enumerate(zip(fc.transform_expected(name, d), fc.transform_magnitudes(name, d))):
                for k in want:
                    yield f"frames {name} {d} {k}", want[k], A[k], i < 2
    for name in fc.PROJECT:
        for coords in (False, True):
            for i, (want, A) in enumerate(zip(fc.project_expected(name, coords), fc.project_magnitudes(name, coords))):
                for k in A:
                    yield f"frames {name} {coords} {k}", want[k], A[k], i < 2
    for name, variant in sc.ALL:
        for want, A in zip(sc.expected(name, variant), sc.magnitudes(name, variant)):
            for k in want:
                yield f"surfels {sc.tag(name, variant)} {k}", want[k], A[k], True
    for name in hc.NAMES:
        for want, A in zip(hc.expected(name), hc.magnitudes(name)):
            for k in A:
                yield f"hard projection {name} {k}", want[k], A[k], True


def test_every_magnitude_bounds_its_entry_and_the_median_is_within_2_to_the_8():
    """The camera gradients are sums over N points of terms of either sign, so |sum| is about A / sqrt(N) whatever the
    arithmetic: their A / |ref| measures the case's cancellation, not the looseness of A, and only A >= |ref| is held."""
    for tag, want, A, per_point in _seeded():
        assert A.shape == want.shape and np.all(np.isfinite(A)) and np.all(A >= 0), tag
        assert np.all(np.abs(want) <= A * (1 + 2.0 ** -40)), (tag, float((np.abs(want) - A).max()))
        nz = want != 0
        if per_point and nz.any():
            median = float(np.median(A[nz] / np.abs(want[nz])))
            assert median < 2.0 ** 8, (tag, median)
    import surfels_oracle as so
    for name, variant in sc.ALL:                            # the lift's camera gradients, which `expected` does not return
        c = sc.case(name, variant)
        if c["frame"] == "world":
            want = ce.co.lift_gradients({"depth": c["depth"]}, c["camera"], c["upstream"], "world")[2]["camera"]
            A = sc.magnitudes(name, variant)[2]
            for k in want:
                assert np.all(np.abs(want[k]) <= A[k] * (1 + 2.0 ** -40)), (name, k)
    assert so.magnitudes is not None


PER_ENTRY = [i for i in ce.ALL if ce._layer_of(i[0], i[1]) in ("lift", "normals", "transform", "project")]


@pytest.mark.parametrize("layer,name,variant", PER_ENTRY, ids=[ce.tag(*i) for i in PER_ENTRY])
def test_the_magnitudes_of_the_camera_edge_cases_bound_the_restatement(layer, name, variant):
    want, A = ce.expected(layer, name, variant), ce.magnitudes(layer, name, variant)
    rows = [0, 2] if layer == "poisoned" else slice(None)
    for w, a in zip(want, A):
        for k in (a or {}):
            if k in w and np.isfinite(w[k][rows]).all():
                assert np.all(np.abs(w[k][rows]) <= a[k][rows] * (1 + 2.0 ** -40)), (k, w[k], a[k])
                assert ec.check(w[k][rows].astype(F32), w[k][rows], a[k][rows]) <= 1.0           # fp64, stored once


# ---- (e) the plane fit's ill-conditioned share -------------------------------------------------------------------------
NORMALS = [("seeded", n, v) for n, v in nc.ALL] + [("edge", n, None) for n in ne.NAMES]


@pytest.mark.parametrize("kind,name,variant", NORMALS, ids=[f"{k} {nc.tag(n, v)}" for k, n, v in NORMALS])
def test_the_ill_conditioned_entries_of_a_normals_case_are_at_most_one_percent(kind, name, variant):
    first, second = (nc.expected(name, variant), nc.turned(name, variant)) if kind == "seeded" else \
        (ne.expected(name), ne.turned(name))
    for a, b in zip(first, second):
        for k in a:
            fin = np.isfinite(a[k])
            assert np.array_equal(fin, np.isfinite(b[k])), (name, k)
            scale = np.abs(a[k][fin]).max()
            with np.errstate(invalid="ignore"):
                ill = fin & ec.ill_conditioned(a[k], b[k], scale)
            print(f"{nc.tag(name, variant)} {k}: {int(ill.sum())} of {a[k].size} entries ill-conditioned")
            assert ill.sum() <= 0.01 * a[k].size, (name, k, int(ill.sum()))
    assert ec.NORMALS_C64 <= ec.NORMALS_C64_CAP == 2.0 ** -36
