"""GPU: camera_grad=True of projection_renderer_differentiable_camera and of estimate_surface_normals_plane_fit_batched(frame=
'world') (srh_dense_projection_bwd_view, srh_normals_bwd_view) against the fp64 restatement with camera leaves,
tests/dense_camera_oracle.py, on every seeded case of dense_projection_cases and normals_cases;
tests/test_dense_camera_oracle_cpu.py ties that restatement to the layers' own oracles and to central differences,
tests/test_dense_camera_golden_cpu.py to the reference's own camera gradients.

Stated tolerance for the camera gradients: the layers' own, rtol 2e-6 with atol 2e-7 max|want| per array
(projection_checks.compare_grads), every element compared, no entry left out.  It holds for the same reason as for the
other gradients: the kernels sum the restatement's fp64 products from the same fp32 inputs without atomics, the chain
from the per-view matrix to eye / at / up is fp64 autograd, and the result is rounded once into the leaf's dtype.

Where the dense reduction (one wave per workgroup, then one finish workgroup per view) can break: four live lanes of one
wave (2x2); a last workgroup of 25 live lanes whose dead lanes repeat surfel 152 (17x9); three full workgroups (12x16);
21 workgroups (35x37); B = 2 with 27 workgroups each (36x48); and 65 workgroups (65x64, built here), the smallest frame
at which a row of the finish kernel adds a second partial before its tree.  The normals run 256-lane workgroups: the
seeded cases have at most seven, and 132x128 (66) is built here."""
import functools

import numpy as np
import pytest
import torch

import camera_chain_oracle as co
import dense_camera_oracle as dco
import dense_projection_cases as dc
import dense_projection_oracle as do
import normals_cases as nc
import projection_cases as pc
import surfels_cases as sc
from projection_checks import assert_bit_identical, compare_grads, compare_values, one_view, to_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = co.CAMERA_KEYS


def leaves(camera, dtype=torch.float32, device=DEV):
    """The camera with eye, at and up as leaves that require grad."""
    return dict(camera, **{k: torch.tensor(np.asarray(camera[k]), dtype=dtype, device=device, requires_grad=True)
                           for k in KEYS})


def camera_grads(camera):
    return {k: to_np(camera[k].grad) for k in KEYS if isinstance(camera[k], torch.Tensor) and camera[k].is_leaf}


def dense(c, camera=None, wrt=do.INPUTS, camera_grad=True):
    """(values, gradients, camera gradients) of a dense case; `camera`: the camera to call with."""
    from surf_renderer_amd import projection_renderer_differentiable, projection_renderer_differentiable_camera
    camera = leaves(c["camera"]) if camera is None else camera
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=k in wrt) for k in do.INPUTS if c[k] is not None}
    # the detached call is the function under the reference's name, which has no such keyword
    fn, kw = (projection_renderer_differentiable_camera, {"camera_grad": True}) if camera_grad else \
        (projection_renderer_differentiable, {})
    out, mask = fn(x["surfels"], x["rgb"], camera, x.get("rotated_image"), blur_size=c["blur_size"], **kw)
    loss = sum((r * torch.tensor(c["upstream"][k], device=DEV)).sum() for k, r in (("out", out), ("mask", mask)))
    if loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    return ({"out": to_np(out), "mask": to_np(mask)}, {k: to_np(t.grad) for k, t in x.items()}, camera_grads(camera))


def normals(c, camera=None, wrt=True, camera_grad=True, frame="world"):
    """(values, gradients, camera gradients) of a normals case, in the world frame whatever the case's own."""
    from surf_renderer_amd import estimate_surface_normals_plane_fit_batched as fit
    camera = leaves(c["camera"]) if camera is None else camera
    p = torch.tensor(c["pos"], device=DEV, requires_grad=wrt)
    kw = {"camera_grad": True} if camera_grad else {}
    n = fit(p, camera, frame=frame, **kw)
    loss = (n * torch.tensor(c["upstream"]["normal"], device=DEV)).sum()
    if loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    return {"normal": to_np(n)}, {"pos": to_np(p.grad)}, camera_grads(camera)


@functools.lru_cache(maxsize=None)
def expected_dense(frame, layout="grid", rotated=False):
    c = dc.case(frame, layout, rotated)
    return dco.project_gradients(dc.inputs(c), c["camera"], c["upstream"], c["blur_size"])


@functools.lru_cache(maxsize=None)
def expected_normals(name, variant=None):
    c = nc.case(name, variant)
    return dco.normals_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], "world")


def compare_camera(got, want, tag, camera):
    for k in KEYS:
        assert got[k].shape == np.asarray(camera[k]).shape, (tag, k)
    compare_grads(got, want, tag)


def detached(run, c, **kw):
    """(values, gradients) of the same call without the keyword and with the camera as data."""
    return run(c, camera=c["camera"], camera_grad=False, **kw)[:2]


# ---- the dense layer ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame,layout,rotated", dc.ALL)
def test_dense_camera_gradients_match_the_restatement(frame, layout, rotated):
    c = dc.case(frame, layout, rotated)
    tag = "dense " + dc.tag(frame, layout, rotated)
    got, got_g, got_cam = dense(c)
    want, want_g, want_cam = expected_dense(frame, layout, rotated)
    compare_values(got, want, tag)
    compare_grads(got_g, want_g, tag)
    compare_camera(got_cam, want_cam["camera"], tag + " camera", c["camera"])


@functools.lru_cache(maxsize=None)
def big_dense_case():
    """65 x 64, B = 1, D = 1: N = 4160 is 65 one-wave workgroups, one more than the finish kernel has rows."""
    B, H, W, D, sigma = 1, 65, 64, 1, 1.2
    rng = np.random.RandomState(7300)
    eye, at, up = pc.draw_camera(rng, B)
    px, py = pc.jittered_grid(rng, B, H, W, 1.2)
    z = rng.uniform(1.5, 3.0, (B, H * W))
    c = {"surfels": pc.f32(pc.lift(px, py, z, eye, at, up, W, H)), "rgb": pc.f32(rng.uniform(0, 1, (B, H, W, D))),
         "rotated_image": pc.f32(rng.uniform(0, 1, (B, H, W, D))),
         "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY),
                    "focal_length": pc.FOCAL},
         "blur_size": float(np.float32(6 * sigma / W)), "shape": (B, H, W, D),
         "upstream": {"out": pc.f32(rng.uniform(-1, 1, (B, H, W, D))), "mask": pc.f32(rng.uniform(-1, 1, (B, H, W, 1)))}}
    assert do.z_margin(c["surfels"], c["camera"]) >= dc.Z_MARGIN
    return c


def test_dense_more_partials_than_the_finish_kernel_has_rows():
    c = big_dense_case()
    # the separable restatement: the dense one would hold several [4160, 4160] fp64 tensors for autograd
    want, want_g, want_cam = dco.project_gradients(dc.inputs(c), c["camera"], c["upstream"], c["blur_size"],
                                                   fn=do.project_separable)
    got, got_g, got_cam = dense(c)
    compare_values(got, want, "dense 65x64")
    compare_grads(got_g, want_g, "dense 65x64")
    compare_camera(got_cam, want_cam["camera"], "dense 65x64 camera", c["camera"])
    assert_bit_identical(detached(dense, c), (got, got_g))
    assert_bit_identical((got_cam,), (dense(c)[2],))


DENSE_PROPERTY_CASES = [("2x2", "grid", False), ("17x9", "flat", False), ("12x16", "grid", True), ("35x37", "grid", False),
                        ("36x48", "grid", True)]


@pytest.mark.parametrize("frame,layout,rotated", DENSE_PROPERTY_CASES)
def test_dense_outputs_and_the_other_gradients_are_bit_identical_to_the_detached_call(frame, layout, rotated):
    c = dc.case(frame, layout, rotated)
    assert_bit_identical(detached(dense, c), dense(c)[:2])


@pytest.mark.parametrize("frame,layout,rotated", DENSE_PROPERTY_CASES)
def test_dense_two_runs_are_bit_identical_in_the_camera_gradients(frame, layout, rotated):
    c = dc.case(frame, layout, rotated)
    assert_bit_identical((dense(c)[2],), (dense(c)[2],))


@pytest.mark.parametrize("frame,layout,rotated", [("17x9", "flat", False), ("12x16", "grid", True), ("36x48", "grid", True)])
def test_dense_a_view_of_a_batch_has_the_bits_of_the_view_alone(frame, layout, rotated):
    c = dc.case(frame, layout, rotated)
    whole = dense(c)[2]
    for b in range(c["shape"][0]):
        assert_bit_identical((whole,), (dense(one_view(c, b, do.INPUTS))[2],), slice(b, b + 1))


@pytest.mark.parametrize("frame,layout,rotated", [("17x9", "grid", False), ("36x48", "grid", True)])
def test_dense_camera_only(frame, layout, rotated):
    """Nothing else requires grad: no grad_surfels buffer exists, the others' .grad stays None, and the camera gradient
    has the bits it has with them."""
    c = dc.case(frame, layout, rotated)
    got, got_g, got_cam = dense(c, wrt=())
    assert all(g is None for g in got_g.values())
    full = dense(c)
    assert_bit_identical((got,), (full[0],))
    assert_bit_identical((got_cam,), (full[2],))
    for wrt in (("rgb",), ("rotated_image",) if rotated else ("surfels",)):        # and beside one other leaf
        assert_bit_identical((dense(c, wrt=wrt)[2],), (full[2],))


def test_dense_a_tensor_shared_by_two_cameras_and_a_leaf_sliced_into_the_batch_get_the_sum():
    c = dc.case("12x16", "grid", True)
    B = c["shape"][0]
    per_view = dense(c)[2]
    # one leaf [B + 1, 3] whose rows 1.. are the batch's eyes
    leaf = torch.tensor(np.concatenate((np.zeros((1, 3)), c["camera"]["eye"])), dtype=torch.float32, device=DEV,
                        requires_grad=True)
    cam = dict(leaves(c["camera"]), eye=leaf[1:])
    dense(c, camera=cam)
    assert np.array_equal(to_np(leaf.grad)[1:], per_view["eye"]) and not np.any(to_np(leaf.grad)[0])
    # the same eye for both views, as one [1, 3] leaf expanded, against the two views' own gradients
    same = dict(c, camera=dict(c["camera"], eye=np.repeat(c["camera"]["eye"][:1], B, axis=0)))
    separate = dense(same)[2]
    one = torch.tensor(c["camera"]["eye"][:1], dtype=torch.float32, device=DEV, requires_grad=True)
    dense(same, camera=dict(leaves(same["camera"]), eye=one.expand(B, -1)))
    want = separate["eye"].sum(0, keepdims=True)
    assert one.grad.shape == (1, 3)
    np.testing.assert_allclose(to_np(one.grad), want, rtol=2e-6, atol=2e-7 * np.abs(separate["eye"]).max())
    # and one tensor as the eye of two calls' cameras: the sum of the two calls' gradients
    shared = leaves(c["camera"])
    dense(c, camera=shared)
    dense(c, camera=dict(leaves(c["camera"]), eye=shared["eye"]))
    assert np.array_equal(to_np(shared["eye"].grad), (2 * per_view["eye"].astype(np.float32)).astype(np.float64))


def test_dense_fp64_and_cpu_camera_leaves_get_their_gradient_in_their_own_dtype_and_device():
    c = dc.case("12x16", "grid", False)
    want = expected_dense("12x16")[2]["camera"]
    for dtype, device in ((torch.float64, DEV), (torch.float64, "cpu"), (torch.float32, "cpu")):
        cam = leaves(c["camera"], dtype, device)
        got = dense(c, camera=cam)[2]
        for k in KEYS:
            g = cam[k].grad
            assert g.dtype == dtype and g.device.type == torch.device(device).type and g.shape == cam[k].shape
        compare_grads(got, want, f"dense {dtype} {device}")


def test_dense_homogeneous_cameras_get_zero_in_w():
    c = dc.case("17x9", "grid", False)
    w = {"eye": 1.0, "at": 1.0, "up": 0.0}
    hom = dict(c["camera"], **{k: np.concatenate((c["camera"][k], np.full((3, 1), w[k])), axis=1) for k in KEYS})
    got = dense(dict(c, camera=hom))[2]
    want = expected_dense("17x9")[2]["camera"]
    for k in KEYS:
        assert got[k].shape == (3, 4) and not np.any(got[k][:, 3])
    compare_grads({k: got[k][:, :3] for k in KEYS}, want, "dense 17x9 [B, 4]")


def test_dense_surfels_outside_the_frame_still_move_the_camera_and_the_fast_layer_does_not():
    """Why the layer matters for pose refinement: the camera is moved sideways until every surfel of the view projects
    outside the frame by at least three sigma.  The dense layer's camera gradient is then still non-zero and within the bound of
    the restatement; the fast layer's, for the same inputs, is exactly zero."""
    from surf_renderer_amd import projection_renderer_differentiable_fast
    c = one_view(dc.case("12x16", "grid", False), 0, do.INPUTS)
    B, H, W, D = c["shape"]
    sigma = dc.sigma(c)
    eye, at, up = (c["camera"][k] for k in KEYS)
    side = np.cross(up, eye - at)
    side /= np.linalg.norm(side)
    for step in np.arange(0.25, 16.0, 0.25):                     # move the camera sideways until the view is empty
        cam = dict(c["camera"], eye=pc.f32(eye + step * side), at=pc.f32(at + step * side))
        px = co.pixel_coordinates(torch.as_tensor(c["surfels"].astype(np.float64)), cam).numpy()[..., :2]
        off = np.maximum.reduce([-px[..., 0], px[..., 0] - W, -px[..., 1], px[..., 1] - H])
        if off.min() >= 3 * sigma + 2:                           # (+ 2: clear of the fast layer's four-pixel footprint)
            break
    assert off.min() >= 3 * sigma + 2 and off.min() <= 8 * sigma, (off.min(), sigma)
    c = dict(c, camera=cam)
    assert do.z_margin(c["surfels"], cam) >= dc.Z_MARGIN
    want, want_g, want_cam = dco.project_gradients(dc.inputs(c), cam, c["upstream"], c["blur_size"])
    got, got_g, got_cam = dense(c)
    assert all(np.abs(g).max() > 0 for g in want_cam["camera"].values())
    compare_values(got, want, "dense outside")
    compare_grads(got_g, want_g, "dense outside")
    compare_camera(got_cam, want_cam["camera"], "dense outside camera", cam)
    fast_cam = leaves(cam)
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=True) for k in ("surfels", "rgb")}
    out, _ = projection_renderer_differentiable_fast(x["surfels"], x["rgb"], fast_cam, blur_size=c["blur_size"],
                                                     camera_grad=True)
    (out * torch.tensor(c["upstream"]["out"], device=DEV)).sum().backward()
    torch.cuda.synchronize()
    assert all(fast_cam[k].grad is not None and not np.any(to_np(fast_cam[k].grad)) for k in KEYS)


# ---- the normals in the world frame ---------------------------------------------------------------------------------

def _with_camera(c, kind):
    """The case with its camera per view [B, 3], per view [B, 4], or shared [3] / [4] (view 0's)."""
    cam, w = c["camera"], {"eye": 1.0, "at": 1.0, "up": 0.0}
    B = c["shape"][0]
    if kind in ("shared3", "shared4"):
        cam = dict(cam, **{k: cam[k][0] for k in KEYS})
    if kind in ("view4", "shared4"):
        cam = dict(cam, **{k: np.concatenate((cam[k], np.full((*cam[k].shape[:-1], 1), w[k])), axis=-1) for k in KEYS})
    return dict(c, camera=cam), B


@pytest.mark.parametrize("kind", ["view3", "view4", "shared3", "shared4"])
@pytest.mark.parametrize("name,variant", nc.ALL)
def test_normals_camera_gradients_match_the_restatement(name, variant, kind):
    c, B = _with_camera(nc.case(name, variant), kind)
    tag = f"normals {nc.tag(name, variant)} {kind}"
    got, got_g, got_cam = normals(c)
    if kind == "view3":
        want, want_g, want_cam = expected_normals(name, variant)
    else:
        want, want_g, want_cam = dco.normals_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], "world")
    compare_values(got, want, tag)
    compare_grads(got_g, want_g, tag)
    for k in KEYS:
        assert got_cam[k].shape == np.asarray(c["camera"][k]).shape, (tag, k)
        if kind.endswith("4"):
            assert not np.any(got_cam[k][..., 3]), (tag, k)
    compare_grads({k: got_cam[k][..., :3] for k in KEYS}, {k: want_cam["camera"][k][..., :3] for k in KEYS}, tag + " camera")


@functools.lru_cache(maxsize=None)
def big_normals_case():
    """132 x 128: N = 16896 is 66 workgroups of 256, so two of the finish kernel's 64 rows add a second partial."""
    B, H, W = 1, 132, 128
    rng = np.random.RandomState(7400)
    eye, at, up = pc.draw_camera(rng, B)
    camera = {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY), "focal_length": pc.FOCAL}
    return {"pos": nc.lifted(nc.draw_depth(rng, B, H, W), camera), "camera": camera, "frame": "world", "shape": (B, H, W),
            "upstream": {"normal": pc.f32(np.round(rng.uniform(-1, 1, (B, H, W, 3)) * 64) / 64)}}


def test_normals_more_partials_than_the_finish_kernel_has_rows():
    c = big_normals_case()
    want, want_g, want_cam = dco.normals_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], "world")
    got, got_g, got_cam = normals(c)
    compare_values(got, want, "normals 132x128")
    compare_grads(got_g, want_g, "normals 132x128")
    compare_camera(got_cam, want_cam["camera"], "normals 132x128 camera", c["camera"])
    assert_bit_identical(detached(normals, c), (got, got_g))
    assert_bit_identical((got_cam,), (normals(c)[2],))


@pytest.mark.parametrize("name", ["2x2", "12x16", "17x9", "36x48"])
def test_normals_bit_identity_with_the_detached_call_and_from_run_to_run(name):
    c = nc.case(name)
    got, got_g, got_cam = normals(c)
    assert_bit_identical(detached(normals, c), (got, got_g))
    assert_bit_identical((got_cam,), (normals(c)[2],))


@pytest.mark.parametrize("name", ["12x16", "17x9"])
def test_normals_a_view_of_a_batch_has_the_bits_of_the_view_alone(name):
    c = nc.case(name)
    whole = normals(c)[2]
    for b in range(c["shape"][0]):
        assert_bit_identical((whole,), (normals(one_view(c, b, ("pos",)))[2],), slice(b, b + 1))


@pytest.mark.parametrize("name", ["17x9", "36x48"])
def test_normals_camera_only(name):
    c = nc.case(name)
    got, got_g, got_cam = normals(c, wrt=False)
    assert got_g["pos"] is None
    full = normals(c)
    assert_bit_identical((got,), (full[0],))
    assert_bit_identical((got_cam,), (full[2],))


def test_normals_fp64_and_cpu_camera_leaves_get_their_gradient_in_their_own_dtype_and_device():
    c = nc.case("17x9")
    want = expected_normals("17x9")[2]["camera"]
    for dtype, device in ((torch.float64, DEV), (torch.float64, "cpu"), (torch.float32, "cpu")):
        cam = leaves(c["camera"], dtype, device)
        got = normals(c, camera=cam)[2]
        for k in KEYS:
            g = cam[k].grad
            assert g.dtype == dtype and g.device.type == torch.device(device).type and g.shape == cam[k].shape
        compare_grads(got, want, f"normals {dtype} {device}")


def test_normals_in_the_camera_frame_leave_the_camera_without_a_gradient():
    c = nc.case("12x16")
    cam = leaves(c["camera"])
    got, got_g, _ = normals(c, camera=cam, frame="camera")
    assert all(cam[k].grad is None for k in KEYS)
    assert_bit_identical(detached(normals, c, frame="camera"), (got, got_g))


# ---- the chains -------------------------------------------------------------------------------------------------------

def test_the_chain_from_a_depth_map_through_two_cameras_into_the_dense_layer():
    """depth -> depth_to_surfels(camera_a) -> projection_renderer_differentiable_camera(camera_b) -> weighted sum of out and
    mask, at 12x16 with B = 2: the gradients of depth, rgb, camera_a and camera_b against the composed restatement (which
    rounds the surfels between the two layers to fp32, as the layers hand them on)."""
    from surf_renderer_amd import depth_to_surfels, projection_renderer_differentiable_camera
    cl, cp = sc.case("12x16"), dc.case("12x16", "grid", True)
    depth = np.abs(cl["depth"]) + (cl["depth"] == 0) * 2.0          # every point in front of camera A
    want, want_g, want_cam = dco.lift_project_gradients(depth, cp["rgb"], cl["camera"], cp["camera"], cp["upstream"],
                                                        cp["rotated_image"], cp["blur_size"])
    pos64 = co.lift(torch.as_tensor(depth.astype(np.float64)), cl["camera"]).numpy()
    assert do.z_margin(pos64, cp["camera"]) >= dc.Z_MARGIN
    cam_a, cam_b = leaves(cl["camera"]), leaves(cp["camera"])
    d = torch.tensor(depth, device=DEV, requires_grad=True)
    rgb = torch.tensor(cp["rgb"], device=DEV, requires_grad=True)
    pos = depth_to_surfels(d, cam_a, camera_grad=True)
    out, mask = projection_renderer_differentiable_camera(pos, rgb, cam_b, torch.tensor(cp["rotated_image"], device=DEV),
                                                          blur_size=cp["blur_size"], camera_grad=True)
    ((out * torch.tensor(cp["upstream"]["out"], device=DEV)).sum()
     + (mask * torch.tensor(cp["upstream"]["mask"], device=DEV)).sum()).backward()
    torch.cuda.synchronize()
    compare_values({"out": to_np(out), "mask": to_np(mask)}, want, "dense chain")
    compare_camera(camera_grads(cam_a), want_cam["camera_a"], "dense chain camera_a", cl["camera"])
    compare_camera(camera_grads(cam_b), want_cam["camera_b"], "dense chain camera_b", cp["camera"])
    compare_grads({"rgb": to_np(rgb.grad), "depth": to_np(d.grad).reshape(want_g["depth"].shape)}, want_g, "dense chain")


def test_the_chain_from_a_depth_map_to_world_normals():
    """depth -> depth_to_surfels(frame='camera') -> world normals -> weighted sum: the gradients of depth and of the
    camera (through the rotation alone: the lift in the camera frame does not read eye / at / up)."""
    from surf_renderer_amd import depth_to_surfels, estimate_surface_normals_plane_fit_batched
    c = nc.case("12x16", "flat")
    B, H, W = c["shape"]
    depth = pc.f32(nc.draw_depth(np.random.RandomState(7500), B, H, W)).reshape(B, H * W)
    want, want_g, want_cam = dco.lift_normals_gradients(depth, c["camera"], c["upstream"])
    cam = leaves(c["camera"])
    d = torch.tensor(depth, device=DEV, requires_grad=True)
    pos = depth_to_surfels(d, cam, frame="camera", camera_grad=True)
    n = estimate_surface_normals_plane_fit_batched(pos, cam, frame="world", camera_grad=True)
    (n * torch.tensor(c["upstream"]["normal"], device=DEV)).sum().backward()
    torch.cuda.synchronize()
    compare_values({"normal": to_np(n)}, want, "normals chain")
    compare_grads({"depth": to_np(d.grad)}, want_g, "normals chain")
    compare_camera(camera_grads(cam), want_cam["camera"], "normals chain camera", c["camera"])
