"""GPU: world_to_cam[_batched], cam_to_world[_batched], project_surfels and project_image_coordinates
(surf_renderer_amd/csrc/srh_frames.h) against the fp64 restatement tests/frames_oracle.py on the same fp32 inputs;
tests/test_frames_oracle_cpu.py ties that to the reference's own functions (tests/golden/frames/fr1_*.npz).

Stated tolerances: the kernels compute the restatement's fp64 arithmetic from the same fp32 inputs and store fp32 once,
so every output element, every gradient entry and every camera gradient entry is held to its own bound
|got - ref| <= 2^-24 |ref| + 2^-40 A + 2^-149, A the restatement's sum of the magnitudes of the entry's terms
(tests/entry_checks.py, frames_oracle.transform_magnitudes / project_magnitudes; a camera entry's A is |J|^T of the table
gradients' sums).  The same arithmetic in float32 does not meet that bound (tests/test_entry_checks_cpu.py).  The older
array-scale comparison stays beside it: rtol 2e-6 with atol 2e-7 max(|want|, 1) for values and 2e-7 max|want| for
gradients (projection_checks), camera gradients alike, an entry below 1e-9 of the camera's largest gradient being held
to that size.  px_idx equals the oracle's on every surfel: the seeded surfels keep 1e-3 px from every rounding boundary
(frames_cases)."""
import numpy as np
import pytest
import torch

import entry_checks as ec
import frames_cases as cases
import frames_oracle as fo
from entry_checks import to_np
from projection_checks import assert_bit_identical, compare_grads, compare_values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VIEW_KEYS = ("eye", "at", "up")
TRANSFORMS = [(n, d) for n in cases.TRANSFORM for d in cases.DIRECTIONS]


def compare_camera(got, want, tag):
    """One camera's eye / at / up gradients under the stated tolerance.  An entry the loss cannot reach but through
    rounding has a gradient of fp64 rounding noise in the restatement and in the layer alike, which no relative
    comparison can hold to; such an entry, below 1e-9 of the camera's largest, must be as small here."""
    top = max(np.abs(w).max() for w in want.values())
    live = {k: w for k, w in want.items() if top == 0 or np.abs(w).max() > 1e-9 * top}
    compare_grads({k: got[k] for k in live}, live, tag, nonzero=False)
    for k in set(want) - set(live):
        assert got[k].shape == want[k].shape and np.abs(got[k]).max() <= 1e-9 * top, (tag, k)


def check_entries(got, want, A, tag):
    """(values, gradients, camera gradients) from the GPU against the restatement's and its magnitudes, entry by entry
    (entry_checks.check); an int64 px_idx has no magnitude and is compared where it is popped.  A None stands for a part
    that is not compared.  Returns the worst ratio of an error to its bound."""
    worst = 0.0
    for what, g, w, a in zip(("values", "gradients", "camera"), got, want, A):
        if g is not None:
            worst = max(worst, ec.check_all(g, {k: v for k, v in w.items() if k in a}, a, f"{tag} {what}"))
    return worst


def _camera(camera, camera_grad):
    """The camera to call with, and its eye / at / up leaves (empty when detached)."""
    if not camera_grad:
        return camera, {}
    leaves = {k: torch.tensor(camera[k], device=DEV, requires_grad=True) for k in VIEW_KEYS}
    return dict(camera, **leaves), leaves


def _finish(outs, upstream, leaves, cam_leaves):
    loss = sum((outs[k] * torch.tensor(g, device=DEV)).sum() for k, g in upstream.items() if k in outs)
    if loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    values = {k: (v.cpu().numpy() if v.dtype == torch.int64 else to_np(v)) for k, v in outs.items()}
    return values, {k: to_np(t.grad) for k, t in leaves.items()}, {k: to_np(t.grad) for k, t in cam_leaves.items()}


def transform(c, direction, camera_grad=False, wrt=True, batched=True):
    """(values, gradients, camera gradients) of a transform case from the GPU; `batched` False: the unbatched function
    on a one-view case, the results given their B back."""
    import surf_renderer_amd as sra
    fn = getattr(sra, {"to_cam": "world_to_cam", "to_world": "cam_to_world"}[direction] + ("_batched" if batched else ""))
    leaves = {k: torch.tensor(c[k], device=DEV, requires_grad=wrt) for k in ("pos", "normal") if c[k] is not None}
    camera, cam_leaves = _camera(c["camera"], camera_grad)
    args = [leaves.get("pos"), leaves.get("normal")]
    if batched:
        res = fn(*args, camera, camera_grad=camera_grad)
    else:
        res = fn(*(None if a is None else a[0] for a in args), {k: v[0] for k, v in camera.items()},
                 camera_grad=camera_grad)
        res = {k: None if v is None else v[None] for k, v in res.items()}
    assert set(res) == {"pos", "normal"}
    for k, cols in (("pos", 4), ("normal", 3)):
        assert (res[k] is None) == (c[k] is None)
        if res[k] is not None:
            assert res[k].shape == (*c[k].shape[:2], cols) and res[k].dtype == torch.float32 and res[k].is_cuda
    return _finish({k: v for k, v in res.items() if v is not None}, c["upstream"], leaves, cam_leaves)


def project(c, coords, camera_grad=False, wrt=True):
    import surf_renderer_amd as sra
    leaves = {"surfels": torch.tensor(c["surfels"], device=DEV, requires_grad=wrt)}
    camera, cam_leaves = _camera(c["camera"], camera_grad)
    B, N = c["surfels"].shape[:2]
    if coords:
        idx, px = sra.project_image_coordinates(leaves["surfels"], camera, camera_grad=camera_grad)
        assert idx.shape == (B, N) and idx.dtype == torch.int64 and idx.is_cuda and not idx.requires_grad
        outs = {"px_coord": px, "px_idx": idx}
    else:
        outs = {"plane": sra.project_surfels(leaves["surfels"], camera, camera_grad=camera_grad)}
    out = outs["px_coord" if coords else "plane"]
    assert out.shape == (B, N, 3) and out.dtype == torch.float32 and out.is_cuda
    return _finish(outs, c["upstream"], leaves, cam_leaves)


def _one_view(c, b, keys):
    return dict(c, **{k: (None if c[k] is None else c[k][b:b + 1]) for k in keys},
                upstream={k: u[b:b + 1] for k, u in c["upstream"].items()},
                camera=dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in VIEW_KEYS}))


# ---- values and gradients against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("name,direction", TRANSFORMS)
def test_a_transform_matches_the_restatement(name, direction):
    c = cases.transform_case(name)
    values, grads, cam_grads = transform(c, direction, camera_grad=True)
    want, want_g, want_c = cases.transform_expected(name, direction)
    tag = f"{name} {direction}"
    check_entries((values, grads, cam_grads), (want, want_g, want_c), cases.transform_magnitudes(name, direction), tag)
    compare_values(values, want, tag)
    compare_grads(grads, want_g, tag)
    compare_camera(cam_grads, want_c, tag)
    if c["pos"] is not None:                       # column 3 is w itself
        w = c["pos"][..., 3] if c["pos"].shape[-1] == 4 else np.ones(c["pos"].shape[:2], np.float32)
        assert np.array_equal(values["pos"][..., 3], w)
    if c["normal"] is not None and c["normal"].shape[-1] == 4:
        assert np.all(grads["normal"][..., 3] == 0)
    for k in VIEW_KEYS:
        assert cam_grads[k].shape == c["camera"][k].shape
        if cam_grads[k].shape[-1] == 4:
            assert np.all(cam_grads[k][..., 3] == 0)


@pytest.mark.parametrize("coords", [False, True], ids=["project_surfels", "project_image_coordinates"])
@pytest.mark.parametrize("name", cases.PROJECT)
def test_a_projection_matches_the_restatement(name, coords):
    c = cases.project_case(name)
    values, grads, cam_grads = project(c, coords, camera_grad=True)
    want, want_g, want_c = cases.project_expected(name, coords)
    tag = f"{name} {'px_coord' if coords else 'plane'}"
    if coords:
        W, H = c["frame"]
        assert np.array_equal(values.pop("px_idx"), want["px_idx"])            # every surfel
        assert want["px_idx"].size < 16 or ((want["px_idx"] == W * H).any() and (want["px_idx"] < W * H).any())
    check_entries((values, grads, cam_grads), (want, want_g, want_c), cases.project_magnitudes(name, coords), tag)
    compare_values(values, {k: v for k, v in want.items() if k != "px_idx"}, tag)
    compare_grads(grads, want_g, tag)
    compare_camera(cam_grads, want_c, tag)


def test_nothing_requires_grad():
    c = cases.transform_case("t153_192")
    values, grads, _ = transform(c, "to_world", wrt=False)
    ec.check_all(values, cases.transform_expected("t153_192", "to_world")[0],
                 cases.transform_magnitudes("t153_192", "to_world")[0], "forward only")
    compare_values(values, cases.transform_expected("t153_192", "to_world")[0], "forward only")
    assert grads == {"pos": None, "normal": None}


def test_a_loss_on_one_output_leaves_the_other_input_a_zero_gradient():
    c = cases.transform_case("t153_192")
    for keep in ("pos", "normal"):
        one = dict(c, upstream={keep: c["upstream"][keep]})
        _, grads, cam = transform(one, "to_cam", camera_grad=True)
        _, want_g, want_c = fo.transform_gradients("to_cam", cases.transform_inputs(c), c["camera"], one["upstream"])
        other = "normal" if keep == "pos" else "pos"
        assert np.all(grads[other] == 0) and np.all(want_g[other] == 0)
        A = fo.transform_magnitudes("to_cam", cases.transform_inputs(c), c["camera"], one["upstream"])
        assert np.all(A[1][other] == 0)
        check_entries((None, grads, cam), (None, want_g, want_c), A, f"loss on {keep}")
        compare_grads({keep: grads[keep]}, {keep: want_g[keep]}, f"loss on {keep}")
        compare_camera(cam, want_c, f"loss on {keep}")


# ---- bitwise properties ----------------------------------------------------------------------------------------------
BITWISE_T = [("t1728", "to_cam"), ("t153_192", "to_world"), ("t153_b3", "to_cam")]
BITWISE_P = [("p1728_48x36", True), ("p153_5x3", False), ("p192_16x12", True)]


@pytest.mark.parametrize("name,direction", BITWISE_T)
def test_two_transform_runs_are_bit_identical_and_camera_grad_changes_nothing_else(name, direction):
    c = cases.transform_case(name)
    first = transform(c, direction, camera_grad=True)
    assert_bit_identical(first, transform(c, direction, camera_grad=True))
    assert_bit_identical(first[:2], transform(c, direction, camera_grad=False)[:2])


@pytest.mark.parametrize("name,coords", BITWISE_P)
def test_two_projection_runs_are_bit_identical_and_camera_grad_changes_nothing_else(name, coords):
    c = cases.project_case(name)
    first = project(c, coords, camera_grad=True)
    assert_bit_identical(first, project(c, coords, camera_grad=True))
    assert_bit_identical(first[:2], project(c, coords, camera_grad=False)[:2])


@pytest.mark.parametrize("name,direction", [("t153_192", "to_world"), ("t153_b3", "to_cam"), ("t16896", "to_world")])
def test_a_transform_batch_equals_its_views_bit_for_bit(name, direction):
    c = cases.transform_case(name)
    whole = transform(c, direction, camera_grad=True)
    for b in range(c["camera"]["eye"].shape[0]):
        assert_bit_identical(whole, transform(_one_view(c, b, ("pos", "normal")), direction, camera_grad=True),
                             slice(b, b + 1))


@pytest.mark.parametrize("name,coords", [("p153_5x3", True), ("p192_16x12", False), ("p192_16x12", True)])
def test_a_projection_batch_equals_its_views_bit_for_bit(name, coords):
    c = cases.project_case(name)
    whole = project(c, coords, camera_grad=True)
    for b in range(c["surfels"].shape[0]):
        assert_bit_identical(whole, project(_one_view(c, b, ("surfels",)), coords, camera_grad=True), slice(b, b + 1))


@pytest.mark.parametrize("name", ["t1", "t192_pos", "t153_normal", "t1728"])
@pytest.mark.parametrize("direction", cases.DIRECTIONS)
def test_the_unbatched_form_is_the_batched_form_of_one_view(name, direction):
    c = cases.transform_case(name)
    assert_bit_identical(transform(c, direction, camera_grad=True),
                         transform(c, direction, camera_grad=True, batched=False))


@pytest.mark.parametrize("name", ["p192_16x12", "p1728_48x36"])
def test_px_idx_is_the_hard_projections_key(name):
    """N = W H: the same inputs through srh_hard_projection_keys, whose dropped surfels get N = W H as well."""
    import ctypes as C
    from surf_renderer_amd import _lib
    from surf_renderer_amd._camera import camera_views
    from surf_renderer_amd._projection import upload_view
    c = cases.project_case(name)
    W, H = c["frame"]
    B, N = c["surfels"].shape[:2]
    assert N == W * H and c["surfels"].shape[2] == 3
    fovy, focal, view = camera_views("test", c["camera"], B)
    s = torch.tensor(c["surfels"], device=DEV)
    keys = torch.empty((B, N), dtype=torch.int32, device=DEV)
    p = _lib.SrhHardProjectionParams(n_views=B, width=W, height=H, channels=1, fovy=fovy, focal_length=focal)
    _lib.check(_lib.load().srh_hard_projection_keys(C.byref(p), upload_view(view, DEV).data_ptr(), s.data_ptr(),
                                                    keys.data_ptr(), None))
    torch.cuda.synchronize()
    values, _, _ = project(c, True, wrt=False)
    assert np.array_equal(values["px_idx"], keys.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("direction", cases.DIRECTIONS)
def test_a_camera_tensor_shared_by_the_views_gets_the_sum(direction):
    """One [1, 3] leaf expanded to every view: its gradient is the sum of the per-view gradients (each view's an fp64
    sum stored once as float32; the views added by torch in the leaf's float32)."""
    import surf_renderer_amd as sra
    fn = {"to_cam": sra.world_to_cam_batched, "to_world": sra.cam_to_world_batched}[direction]
    c = cases.transform_case("t153_192")
    B = 2
    shared = {k: c["camera"][k][:1] for k in VIEW_KEYS}
    leaves = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in shared.items()}
    res = fn(torch.tensor(c["pos"], device=DEV), torch.tensor(c["normal"], device=DEV),
             {k: t.expand(B, 3) for k, t in leaves.items()}, camera_grad=True)
    sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
    torch.cuda.synchronize()
    same = dict(c, camera={k: np.repeat(v, B, 0) for k, v in shared.items()})
    _, _, per_view = fo.transform_gradients(direction, cases.transform_inputs(same), same["camera"], same["upstream"])
    got = {k: to_np(t.grad) for k, t in leaves.items()}
    assert all(got[k].shape == (1, 3) for k in VIEW_KEYS)
    # The expansion is the caller's own float32 op: torch hands every view's gradient to it as float32 -- one store per
    # view and entry, the layer's contract -- and adds the B of them in float32.  So the leaf's entry is a float32 sum of
    # float32 terms, 2^-24 sum_b |g_b| beside the sum's own rounding, and A carries that at 2^16 per unit of |g_b|.
    A = fo.transform_magnitudes(direction, cases.transform_inputs(same), same["camera"], same["upstream"])[2]
    ec.check_all(got, {k: v.sum(0, keepdims=True) for k, v in per_view.items()},
                 {k: (A[k] + 2.0 ** 16 * np.abs(per_view[k])).sum(0, keepdims=True) for k in A}, f"shared camera {direction}")
    compare_camera(got, {k: v.sum(0, keepdims=True) for k, v in per_view.items()}, f"shared camera {direction}")


# ---- conversions, round trip, end to end -----------------------------------------------------------------------------
def test_other_dtypes_devices_and_layouts_are_converted_and_gradients_come_back_in_the_leafs_own():
    import surf_renderer_amd as sra
    c = cases.transform_case("t153_192")
    want, want_g, want_c = cases.transform_expected("t153_192", "to_world")
    pos = torch.tensor(c["pos"].astype(np.float64), requires_grad=True)                          # fp64 CPU leaf
    normal_t = torch.tensor(np.ascontiguousarray(c["normal"].transpose(1, 0, 2)), device=DEV, requires_grad=True)
    cam = {"eye": torch.tensor(c["camera"]["eye"].astype(np.float64), requires_grad=True),       # fp64 CPU
           "at": torch.tensor(c["camera"]["at"], device=DEV, requires_grad=True),                # fp32 GPU
           "up": c["camera"]["up"]}                                                              # an ndarray
    res = sra.cam_to_world_batched(pos, normal_t.permute(1, 0, 2), cam, camera_grad=True)        # not contiguous
    sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
    torch.cuda.synchronize()
    A = cases.transform_magnitudes("t153_192", "to_world")
    ec.check_all({k: to_np(v) for k, v in res.items()}, want, A[0], "converted")
    compare_values({k: to_np(v) for k, v in res.items()}, want, "converted")
    for leaf in (pos, normal_t, cam["eye"], cam["at"]):
        assert leaf.grad.dtype == leaf.dtype and leaf.grad.device == leaf.device and leaf.grad.shape == leaf.shape
    got_g = {"pos": ec.narrowed(to_np(pos.grad)), "normal": to_np(normal_t.grad.permute(1, 0, 2))}
    # a float64 leaf gets the float64 sum of the host's chain unrounded: its 2^-24 |ref| term is slack, the floor holds
    got_c = {"eye": to_np(cam["eye"].grad).astype(np.float32), "at": to_np(cam["at"].grad)}
    ec.check_all(got_g, want_g, A[1], "converted gradients")
    ec.check_all(got_c, {k: want_c[k] for k in ("eye", "at")}, A[2], "converted camera")
    compare_grads({"pos": to_np(pos.grad), "normal": to_np(normal_t.grad.permute(1, 0, 2))}, want_g, "converted")
    compare_camera({k: to_np(cam[k].grad) for k in ("eye", "at")}, {k: want_c[k] for k in ("eye", "at")}, "converted")


@pytest.mark.parametrize("name", ["t153_192", "t1728"])
def test_the_round_trip_returns_the_inputs(name):
    """cam_to_world_batched(**world_to_cam_batched(pos, normal, camera)), as the reference's own test_tform_cc_wc."""
    import surf_renderer_amd as sra
    c = cases.transform_case(name)
    there = sra.world_to_cam_batched(c["pos"], c["normal"], c["camera"])
    back = sra.cam_to_world_batched(there["pos"], there["normal"], c["camera"])
    torch.cuda.synchronize()
    w = c["pos"][..., 3:] if c["pos"].shape[-1] == 4 else np.ones((*c["pos"].shape[:2], 1))
    compare_values({"pos": to_np(back["pos"]), "normal": to_np(back["normal"])},
                   {"pos": np.concatenate((c["pos"][..., :3], w), -1).astype(np.float64),
                    "normal": c["normal"][..., :3].astype(np.float64)}, f"{name} round trip")


def test_a_splat_render_goes_to_the_world_frame_and_a_loss_there_reaches_the_scene():
    import copy
    import surf_renderer_amd as sra
    from splat_edge_scenes import base_scene, given_normals, surface
    B, H, W = 2, 5, 13                                        # 65 pixels: one live lane in the second wave
    scene = copy.deepcopy(base_scene(H, W, seed=60, given=False))
    disk = scene["objects"]["disk"]
    pos = torch.tensor(np.stack([surface(H, W, 61 + b) for b in range(B)]), device=DEV, requires_grad=True)
    disk["pos"] = pos
    disk["normal"] = torch.tensor(np.stack([given_normals(H, W, 71 + b) for b in range(B)]), device=DEV)
    disk["material_idx"] = torch.as_tensor(np.asarray(disk["material_idx"]), device=DEV)
    scene["lights"]["color_idx"] = torch.as_tensor(np.asarray(scene["lights"]["color_idx"]), device=DEV)
    scene["camera"]["eye"] = np.array([[0.8 + 0.3 * b, 1.5 - 0.2 * b, 6.0, 1.0] for b in range(B)], np.float32)
    res = sra.render_splats_along_ray_batch(scene, samples=1)
    camera = {"eye": scene["camera"]["eye"], "at": np.tile(scene["camera"]["at"], (B, 1)),
              "up": np.tile(scene["camera"]["up"], (B, 1))}
    pos_cc, normal_cc = res["pos"].reshape(B, H * W, 3), res["normal"].reshape(B, H * W, 3)
    world = sra.cam_to_world_batched(pos_cc, normal_cc, camera)
    inputs = {"pos": to_np(pos_cc).astype(np.float64), "normal": to_np(normal_cc).astype(np.float64)}
    want = fo.cam_to_world_batched(torch.tensor(inputs["pos"]), torch.tensor(inputs["normal"]), camera)
    ec.check_all({k: to_np(v) for k, v in world.items()}, {k: v.numpy() for k, v in want.items()},
                 fo.transform_magnitudes("to_world", inputs, camera, {})[0], "splat to world")
    compare_values({k: to_np(v) for k, v in world.items()}, {k: v.numpy() for k, v in want.items()}, "splat to world")
    up = torch.tensor(np.random.RandomState(5).uniform(-1, 1, (B, H * W, 4)).astype(np.float32), device=DEV)
    (world["pos"] * up).sum().backward()
    torch.cuda.synchronize()
    grad = to_np(pos.grad)
    assert grad.shape == (B, H * W) and np.all(np.isfinite(grad)) and np.count_nonzero(grad) == grad.size
