"""GPU: camera_grad=True -- the kView instantiations of the fused layers' backward kernels, view_block_reduce /
view_wave_reduce and k_view_finish -- on the edge inputs of tests/camera_edge_cases.py, against the fp64 restatements
with camera leaves.  tests/test_camera_edge_cases_cpu.py says what those restatements give on the cases: where they are
non-finite, where exactly zero, and that no entry of a finite case is mere rounding noise of the restatement's sum.

The layers are run through the helpers of their camera suites (test_hip_camera_warp, test_hip_dense_camera,
test_hip_splat_camera, test_hip_frames), so a case goes through the call those suites make.

Tolerances.  The rows of the layers that are held per entry -- lift, normals, transform, project and their poisoned
batches -- hold every finite camera gradient entry to 2^-24 |ref| + 2^-40 A + 2^-149, A = |J|^T of the sums of magnitudes
of the fp64 table gradients (tests/entry_checks.py, camera_edge_cases.magnitudes); the values and gradients of the cases no
other suite holds, alike.  A non-finite camera gradient is a sum that overflowed or met a NaN, and which of the two it shows
depends on the order of the sum, so those entries keep the rule below.  Beside that, and for the other layers, the standing
tolerances of the camera suites: rtol 2e-6 with atol 2e-7 max|want| per array (projection_checks;
test_hip_splat_camera's bound against the restatement is the same figures).  An array below 1e-9 of the camera's largest
gradient, or an entry the CPU test lists as rounding noise, is held to that size.  Where the restatement is exactly 0
the layer's entry is exactly 0; where it is non-finite the layer's entry is non-finite (NaN and inf are not told apart:
an overflow shows as either, depending on the order of the sum).

What camera_grad=True must not change is compared by bit pattern, NaNs included.  The scene-parameter gradients of the
two splat renderers that are summed with atomics (everything but disk.pos, disk.normal and disk.light_vis) differ from
run to run and keep test_hip_splat_camera.py's bound for them, atol 2e-4 max|want| + 1e-6."""
import functools

import numpy as np
import pytest
import torch

import camera_edge_cases as ce
import entry_checks as ec
import frames_oracle as fo
import test_hip_camera_warp as cw
import test_hip_dense_camera as dcam
import test_hip_frames as fr
import test_hip_splat_camera as spl
from projection_checks import ATOL_SCALE, RTOL, compare_grads, compare_values, to_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ce.KEYS
SPLATS = ("along_ray", "ndc")
PLAIN = [i for i in ce.ALL if i[0] != "poisoned"]
POISONED = [i for i in ce.ALL if i[0] == "poisoned"]
# one case per layer whose last workgroup is partly empty
PARTLY_EMPTY = [("lift", "row_1x300", None), ("dense", "far_9x7", ("grid", False)), ("normals", "wide_2x300", None),
                ("along_ray", "block_1x257", None), ("ndc", "uniform_partial", None), ("transform", "counts_1_257", "to_cam"),
                ("transform", "counts_257_1", "to_world"), ("project", "zdepth_16x12", True)]
CAMERA_ONLY = [("lift", "row_1x300", None), ("dense", "far_9x7", ("grid", False)), ("normals", "two_2x2", None),
               ("transform", "counts_1_257", "to_cam"), ("transform", "counts_1_257", "to_world")]


def _ids(items):
    return [ce.tag(*i) for i in items]


def _bits(a):
    return a.view({np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}.get(a.dtype, a.dtype))


def assert_same_bits(a, b, rows=slice(None), what=""):
    """Two dicts of arrays (or None) agree in every bit, NaN payloads and the sign of zero included: `rows` of the
    first with the whole second."""
    assert set(a) == set(b), what
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        x, y = np.ascontiguousarray(a[k][rows]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        differ = np.argwhere(_bits(x) != _bits(y))
        assert not len(differ), (what, k, differ[:8], x[tuple(differ[0])], y[tuple(differ[0])])


def hold_camera(got, want, noise, tag):
    """eye / at / up of one camera against the restatement (module docstring)."""
    top = ce.top(want)
    for k in KEYS:
        g, w = got[k], want[k]
        assert g is not None and g.shape == w.shape, (tag, k)
        finite = np.isfinite(w)
        assert not np.isfinite(g[~finite]).any(), (tag, k, "finite where the restatement is not", g, w)
        assert np.isfinite(g[finite]).all(), (tag, k, "non-finite where the restatement is finite", g, w)
        if not finite.any():
            continue
        assert np.all(g[finite & (w == 0)] == 0), (tag, k, "not exactly 0 where the restatement is", g, w)
        scale = np.abs(w[finite]).max()
        by_size = noise[k] | (np.full(w.shape, scale <= 1e-9 * top) & (top > 0))
        held = finite & ~by_size
        err = np.abs(g[held] - w[held])
        print(f"{tag} {k}: max err {err.max() if err.size else 0.0:.3g}, max|want| {scale:.3g}, "
              f"max err / |want| {np.max(err / np.maximum(np.abs(w[held]), 1e-300)) if err.size else 0.0:.3g}")
        np.testing.assert_allclose(g[held], w[held], rtol=RTOL, atol=ATOL_SCALE * scale, err_msg=f"{tag} {k}")
        assert np.all(np.abs(g[finite & by_size]) <= 1e-9 * top), (tag, k, "a noise entry is not small")


PER_ENTRY = ("lift", "normals", "transform", "project")


def check_camera_entries(layer, name, variant, got_cam, want_cam, tag, rows=slice(None)):
    """`rows` of a finite camera gradient of a PER_ENTRY layer against the restatement, entry by entry; the worst ratio."""
    A = ce.magnitudes(layer, name, variant)[2]
    return ec.check_all({k: ec.narrowed(got_cam[k])[rows] for k in KEYS}, {k: want_cam[k][rows] for k in KEYS},
                        {k: A[k][rows] for k in KEYS}, tag + " camera")


def _splat(layer, c, camera_grad=True, others=True):
    res, grads = spl._run(layer, c["scene"], c["kwargs"], c["upstream"]["image"], camera_grad=camera_grad, others=others)
    return ({k: to_np(v) for k, v in res.items()}, {k: to_np(g) for k, g in grads.items() if k not in spl.CAMERA},
            {k: to_np(grads["camera." + k]) for k in KEYS})


def call(layer, c, variant=None, mode="leaves"):
    """(values, gradients, camera gradients) of a case dict of `layer` from the GPU.  mode: 'leaves' (camera_grad=True,
    everything requires grad), 'camera_only' (camera_grad=True, nothing else requires grad) or 'detached' (the call
    without the keyword and with the camera as data: its camera gradients are None)."""
    on, others = mode != "detached", mode != "camera_only"
    if layer == "lift":
        v, g, cam = cw.lift(c, cameras=None if on else {"camera": c["camera"]}, wrt=("depth",) if others else (), camera_grad=on)
        return v, g, cam["camera"]
    if layer == "dense":
        return dcam.dense(c, camera=None if on else c["camera"], wrt=dcam.do.INPUTS if others else (), camera_grad=on)
    if layer == "normals":
        return dcam.normals(c, camera=None if on else c["camera"], wrt=others, camera_grad=on)
    if layer in SPLATS:
        return _splat(layer, c, camera_grad=on, others=others)
    if layer == "transform":
        return fr.transform(c, variant, camera_grad=on, wrt=others)
    assert layer == "project", layer
    one = dict(c, upstream={k: u for k, u in c["upstream"].items() if k == ("px_coord" if variant else "plane")})
    return fr.project(one, variant, camera_grad=on, wrt=others)


def _layer(layer, name):
    return ce.poisoned_layer(name) if layer == "poisoned" else layer


@functools.lru_cache(maxsize=None)
def full(layer, name, variant=None):
    """The case's run with every leaf requiring grad, computed once and shared; the arrays must not be written to."""
    return call(_layer(layer, name), ce.case(layer, name, variant), variant)


def _no_noise(want):
    return {k: np.zeros(want[k].shape, bool) for k in KEYS}


# ---- every case against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("layer,name,variant", PLAIN, ids=_ids(PLAIN))
def test_camera_gradients_match_the_restatement(layer, name, variant):
    got, got_g, got_cam = full(layer, name, variant)
    want, want_g, want_cam = ce.expected(layer, name, variant)
    tag = ce.tag(layer, name, variant)
    finite = all(np.isfinite(w).all() for w in want_cam.values())
    assert finite == ((layer, name) not in ce.NONFINITE)
    if layer in PER_ENTRY and finite:
        check_camera_entries(layer, name, variant, got_cam, want_cam, tag)
    hold_camera(got_cam, want_cam, ce.noise(layer, name, variant) if finite else _no_noise(want_cam), tag)
    for k in ce.EXACT_ZERO.get((layer, name), ()):
        assert np.all(want_cam[k] == 0) and np.all(got_cam[k] == 0), (tag, k)
    if layer in ("transform", "project") or name == "special_finite_3x3":        # cases no other suite holds
        idx = {"px_idx"} & set(got)
        for k in idx:
            assert np.array_equal(got[k], want[k]), (tag, k)
        A, A_g, _ = ce.magnitudes(layer, name, variant)
        ec.check_all({k: ec.narrowed(v) for k, v in got.items() if k not in idx}, {k: v for k, v in want.items() if k not in idx},
                     A, tag + " values")
        ec.check_all({k: ec.narrowed(g) for k, g in got_g.items()}, want_g, A_g, tag + " gradients")
        compare_values({k: v for k, v in got.items() if k not in idx}, {k: v for k, v in want.items() if k not in idx}, tag)
        compare_grads(got_g, want_g, tag)


@pytest.mark.parametrize("layer,name,variant", ce.ALL, ids=_ids(ce.ALL))
def test_values_and_every_other_gradient_are_those_of_the_detached_call_bit_for_bit(layer, name, variant):
    sub, c = _layer(layer, name), ce.case(layer, name, variant)
    got, got_g, _ = full(layer, name, variant)
    base, base_g, base_cam = call(sub, c, variant, "detached")
    assert all(g is None for g in base_cam.values())
    tag = ce.tag(layer, name, variant)
    assert_same_bits(base, got, what=tag)
    if sub in SPLATS:
        written = set(spl.WRITTEN)
        assert_same_bits({k: g for k, g in base_g.items() if k in written}, {k: g for k, g in got_g.items() if k in written},
                         what=tag)
        for k in set(base_g) - written:
            assert (base_g[k] is None) == (got_g[k] is None), (tag, k)
            if base_g[k] is not None:
                np.testing.assert_allclose(got_g[k], base_g[k], rtol=0, atol=2e-4 * np.abs(base_g[k]).max() + 1e-6, err_msg=f"{tag} {k}")
    else:
        assert_same_bits(base_g, got_g, what=tag)


@pytest.mark.parametrize("layer,name,variant", PARTLY_EMPTY + POISONED, ids=_ids(PARTLY_EMPTY + POISONED))
def test_two_runs_are_bit_identical_in_the_camera_gradients(layer, name, variant):
    again = call(_layer(layer, name), ce.case(layer, name, variant), variant)[2]
    assert_same_bits(full(layer, name, variant)[2], again, what=ce.tag(layer, name, variant))


@pytest.mark.parametrize("layer,name,variant", CAMERA_ONLY, ids=_ids(CAMERA_ONLY))
def test_camera_only(layer, name, variant):
    """Nothing else requires grad, so the kernels get NULL gradient buffers: the others' .grad stays None, and the
    values and the camera gradients have the bits they have beside the other gradients."""
    got, got_g, got_cam = call(layer, ce.case(layer, name, variant), variant, "camera_only")
    assert all(g is None for g in got_g.values())
    whole = full(layer, name, variant)
    assert_same_bits(whole[0], got)
    assert_same_bits(whole[2], got_cam)


# ---- poisoned batches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer,name,variant", POISONED, ids=_ids(POISONED))
def test_a_non_finite_view_spoils_its_own_camera_and_leaves_its_neighbours_their_bits(layer, name, variant):
    """Each view's camera is its own row of the [3, 3] leaves.  View 1 is non-finite in every entry; views 0 and 2 are
    finite, within the bound of the restatement, and have the bits of the same view run alone: the non-finite partial
    rows of view 1 do not reach its neighbours in k_view_finish."""
    sub, c = ce.poisoned_layer(name), ce.case(layer, name, variant)
    got_cam = full(layer, name, variant)[2]
    want_cam = ce.expected(layer, name, variant)[2]
    tag = ce.tag(layer, name, variant)
    for k in KEYS:
        assert got_cam[k].shape == (3, 3) and not np.isfinite(want_cam[k][ce.POISONED_VIEW]).any()
        assert np.isfinite(want_cam[k][[0, 2]]).all()
    if sub in PER_ENTRY:
        check_camera_entries(layer, name, variant, got_cam, want_cam, tag, rows=[0, 2])
    hold_camera(got_cam, want_cam, _no_noise(want_cam), tag)
    for b in (0, 2):
        alone = call(sub, ce.one_view(sub, c, b), variant)[2]
        assert_same_bits(got_cam, alone, slice(b, b + 1), what=f"{tag} view {b}")


def _shared(c):
    """(camera with one [1, 3] leaf per entry -- view 0's -- expanded over the batch, the leaves)."""
    leaf = {k: torch.tensor(c["camera"][k][:1], device=DEV, requires_grad=True) for k in KEYS}
    return dict(c["camera"], **{k: t.expand(3, -1) for k, t in leaf.items()}), leaf


@pytest.mark.parametrize("layer,name,variant", POISONED, ids=_ids(POISONED))
def test_a_leaf_shared_by_the_batch_gets_the_non_finite_sum(layer, name, variant):
    sub, c = ce.poisoned_layer(name), ce.case(layer, name, variant)
    camera, leaf = _shared(c)
    if sub == "lift":
        cw.lift(c, cameras={"camera": camera})
    elif sub == "dense":
        dcam.dense(c, camera=camera)
    elif sub == "normals":
        dcam.normals(c, camera=camera)
    else:
        import surf_renderer_amd as sra
        fn = {"to_cam": sra.world_to_cam_batched, "to_world": sra.cam_to_world_batched}[variant]
        res = fn(torch.tensor(c["pos"], device=DEV), torch.tensor(c["normal"], device=DEV), camera, camera_grad=True)
        sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
        torch.cuda.synchronize()
    for k in KEYS:
        g = to_np(leaf[k].grad)
        assert g.shape == (1, 3) and not np.isfinite(g).any(), (name, k, g)


# ---- the frame transforms and the point projection -------------------------------------------------------------------
@pytest.mark.parametrize("direction", fr.cases.DIRECTIONS)
@pytest.mark.parametrize("name,half", [("counts_1_257", "pos"), ("counts_257_1", "normal")])
def test_the_half_with_one_lane_has_the_bits_it_has_with_the_other_input_absent(name, half, direction):
    """A loss on the one-lane half alone: the other half, present with 257 points, brings the camera exact zeros, so
    the half's output, gradient and camera gradient are those of the call with the other input None."""
    c = ce.case("transform", name, direction)
    other = "normal" if half == "pos" else "pos"
    assert c[half].shape[1] == 1 and c[other].shape[1] == 257
    ups = {half: c["upstream"][half]}
    both = fr.transform(dict(c, upstream=ups), direction, camera_grad=True)
    alone = fr.transform(dict(c, upstream=ups, **{other: None}), direction, camera_grad=True)
    assert np.all(both[1][other] == 0)
    assert_same_bits({half: both[0][half]}, alone[0])
    assert_same_bits({half: both[1][half]}, alone[1])
    assert_same_bits(both[2], alone[2])
    want_cam = fo.transform_gradients(direction, {half: c[half], other: None}, c["camera"], ups)[2]
    ec.check_all(alone[2], want_cam, fo.transform_magnitudes(direction, {half: c[half], other: None}, c["camera"], ups)[2],
                 f"{name} {direction} {half} alone camera")
    hold_camera(alone[2], want_cam, _no_noise(want_cam), f"{name} {direction} {half} alone")


@pytest.mark.parametrize("direction", fr.cases.DIRECTIONS)
def test_a_point_with_w_zero_gets_the_gradient_of_w_and_brings_nothing_to_the_translation(direction):
    """grad_pos[..., 3] = g . M[:, 3] + g3 whatever w is; a row with w = 0 brings 0 to column 3 of d loss / d view_pos,
    which the comparison of the camera gradients with the restatement holds (test_camera_gradients_match_the_restatement)
    and the second half of this test isolates: with the upstream of every other row zeroed, the loss is a function of
    the rotation alone and the camera gradient matches the restatement's for it."""
    c = ce.case("transform", "w0_153", direction)
    rows = list(ce.W0_ROWS)
    _, got_g, _ = full("transform", "w0_153", direction)
    w2c, c2w = fo._tables(c["camera"], torch.zeros(1, dtype=torch.float64))
    M = (w2c if direction == "to_cam" else c2w).numpy()
    g = c["upstream"]["pos"].astype(np.float64)
    want = np.einsum("bnr,br->bn", g[..., :3], M[:, :, 3]) + g[..., 3]
    ec.check(got_g["pos"][..., 3], want, np.einsum("bnr,br->bn", np.abs(g[..., :3]), np.abs(M[:, :, 3])) + np.abs(g[..., 3]),
             f"w0_153 {direction} grad w")
    np.testing.assert_allclose(got_g["pos"][..., 3], want, rtol=RTOL, atol=ATOL_SCALE * np.abs(want).max())
    only = np.zeros_like(c["upstream"]["pos"])
    only[:, rows] = c["upstream"]["pos"][:, rows]
    one = dict(c, normal=None, upstream={"pos": only})
    got_cam = fr.transform(one, direction, camera_grad=True)[2]
    want_cam = fo.transform_gradients(direction, {"pos": one["pos"], "normal": None}, one["camera"], one["upstream"])[2]
    ec.check_all(got_cam, want_cam, fo.transform_magnitudes(direction, {"pos": one["pos"], "normal": None}, one["camera"],
                                                            one["upstream"])[2], f"w0_153 {direction} w0 rows alone camera")
    hold_camera(got_cam, want_cam, _no_noise(want_cam), f"w0_153 {direction} w0 rows alone")


@pytest.mark.parametrize("coords", [False, True], ids=["project_surfels", "project_image_coordinates"])
def test_a_surfel_at_z_zero_brings_its_x_and_y_terms_and_no_division_by_z(coords):
    """The named surfels of zdepth_16x12 alone carry the loss: their camera gradient is finite and the restatement's
    ((dX, dY, -g_z) to the camera sums, no 1 / Zd^2 term), and their grad_surfels are the detached call's, bit for bit."""
    c = ce.case("project", "zdepth_16x12", coords)
    key = "px_coord" if coords else "plane"
    only = np.zeros_like(c["upstream"][key])
    only[:, list(ce.ZDEPTH_ROWS)] = c["upstream"][key][:, list(ce.ZDEPTH_ROWS)]
    one = dict(c, upstream={key: only})
    got, got_g, got_cam = fr.project(one, coords, camera_grad=True)
    want, want_g, want_cam = fo.project_gradients(coords, one["surfels"], one["camera"], one["upstream"])
    assert all(np.abs(w).max() > 0 for w in (want_cam["eye"], want_cam["at"]))
    A = fo.project_magnitudes(coords, one["surfels"], one["camera"], one["upstream"])
    ec.check_all(got_cam, want_cam, A[2], f"zdepth_16x12 {key} named surfels alone camera")
    ec.check_all(got_g, want_g, A[1], f"zdepth_16x12 {key} named surfels alone gradients")
    hold_camera(got_cam, want_cam, _no_noise(want_cam), f"zdepth_16x12 {key} named surfels alone")
    compare_grads(got_g, want_g, f"zdepth_16x12 {key} named surfels alone")
    assert_same_bits(fr.project(one, coords, camera_grad=False)[1], got_g)
