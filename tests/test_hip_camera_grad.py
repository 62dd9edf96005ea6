"""GPU: gradients of render(scene, shading='torch') with respect to the camera's eye, at and up (srh_render_bwd_camera:
the kCam variants of k_render_bwd_tch and k_camera_finish) against the fp64 oracle with the camera in its graph
(oracle/torch_oracle.gradients_tch, camera=True), which tests/test_camera_grad_golden_cpu.py ties to the reference torch
backend's autograd (tests/golden/c1_*.npz).

Stated tolerances, the project's own: per array |got - want| <= 2e-4 * max|want| + 1e-6 against the helper fed the GPU
frame's winners (tests/test_hip_backward.py), 2e-3 * max|ref| against the reference fixtures
(tests/test_hip_aux_grad.py), 2e-5 of the largest entry between two runs of the fp32-atomic scene gradients."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from grad_cases import (CAM, DEV, RUN_TO_RUN, TCH_KEYS, assert_grads_close, camera_leaves, full_scene, gpu_leaf_scene,
                        grad_kwargs, leaf_grads, load, masked_loss, random_upstream, to_np, upstream, winners)
from oracle.golden_io import unpack_scene
from oracle.torch_oracle import CAMERA_KEYS as CAM_KEYS, OUTPUTS, gradients_tch

pytestmark = pytest.mark.gpu

CASES = ["c1_camera_grad_phong", "c1_camera_grad_phong_ds_quartic", "c1_camera_grad_ortho"]


def _hip(scene, g, rows=None, mask=True, camera=True, **kw):
    """render() with GPU leaves -- the scene's and, with ``camera``, eye / at / up -- and masked_loss over the outputs
    named in g; returns ({leaf: grad ndarray}, result)."""
    from surf_renderer_amd import render
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
    cam_leaves = {}
    if camera:
        cam_leaves = camera_leaves(scene["camera"])
        leaf_scene["camera"] = dict(leaf_scene["camera"], **cam_leaves)
    res = render(leaf_scene, device=DEV, shading="torch", rows=rows, **kw)
    masked_loss(res, g, scene["camera"]["far"], mask).backward()
    torch.cuda.synchronize()
    grads = leaf_grads(leaves)
    for k, t in cam_leaves.items():
        assert t.grad is not None, f"camera.{k} got no gradient"
        assert t.grad.shape == t.shape and t.grad.dtype == t.dtype and t.grad.device == t.device
        grads["camera." + k] = to_np(t.grad)
    return grads, res


def _helper(scene, g, res, **kw):
    return gradients_tch(scene, **grad_kwargs(g), ref=winners(res), camera=True, **kw)


@pytest.mark.parametrize("case", CASES)
def test_reference_fixtures_through_render(case):
    npz, scene, kw = load(case)
    g = upstream(npz)
    got, res = _hip(scene, g, **kw)
    same = (res["nearest"].cpu().numpy() == npz["ref/nearest"]) & (npz["ref/depth"] <= scene["camera"]["far"])
    assert same.mean() > 0.995
    assert_grads_close(got, _helper(scene, g, res, **kw), 2e-4, case)
    for key in CAM_KEYS:
        ref = npz["grad/" + key].astype(np.float64)
        print(case, key, "against the reference:", np.abs(got[key] - ref).max() / np.abs(ref).max())
        np.testing.assert_allclose(got[key], ref, rtol=0, atol=2e-3 * np.abs(ref).max(), err_msg=key)
    # the scene's own gradients are those of the same call with the camera detached
    detached, _ = _hip(scene, g, camera=False, **kw)
    for key, w in detached.items():
        np.testing.assert_allclose(got[key], w, rtol=0, atol=RUN_TO_RUN * np.abs(w).max() + 1e-7, err_msg=key)


@pytest.mark.parametrize("ortho", [False, True])
def test_full_scene_with_spheres(ortho):
    scene = full_scene(ortho)
    g = random_upstream()
    got, res = _hip(scene, g)
    for key in CAM_KEYS:
        assert np.all(np.isfinite(got[key])) and np.abs(got[key]).max() > 0.1, key
    assert_grads_close(got, _helper(scene, g, res), 2e-4, f"spheres ortho={ortho}")


@pytest.mark.parametrize("case", ["c1_camera_grad_phong", "c1_camera_grad_ortho"])
def test_each_output_alone_and_linearity(case):
    npz, scene, kw = load(case)
    g = upstream(npz)
    parts = {}
    for which in OUTPUTS:
        parts[which], res = _hip(scene, {which: g[which]}, **kw)
        assert_grads_close(parts[which], _helper(scene, {which: g[which]}, res, **kw), 2e-4, f"{case} {which}")
        if which != "image":                                # the geometry-only kernel: no light / colour / material term
            for key in TCH_KEYS:
                assert np.all(parts[which][key] == 0), (which, key)
    both, _ = _hip(scene, g, **kw)
    assert_grads_close(both, {k: sum(p[k] for p in parts.values()) for k in both}, 2e-4, "sum of parts")


def test_row_slabs_sum_to_the_whole_frame():
    npz, scene, kw = load("c1_camera_grad_phong_ds_quartic")
    g = upstream(npz)
    full, _ = _hip(scene, g, **kw)
    r = 17                                                  # not a multiple of the workgroup's four rows
    top, tres = _hip(scene, {k: v[:r] for k, v in g.items()}, rows=(0, r), **kw)
    bottom, _ = _hip(scene, {k: v[r:] for k, v in g.items()}, rows=(r, 36), **kw)
    assert tres["image"].shape == (r, 48, 3)
    assert_grads_close({k: top[k] + bottom[k] for k in CAM_KEYS}, {k: full[k] for k in CAM_KEYS}, 2e-4, "slabs")


def test_shadow_rays():
    """Visibility is a constant 0 / 1 factor per light: the helper is fed the GPU's own visibility bits."""
    from surf_renderer_amd import render
    scene = full_scene()
    g = random_upstream()
    got, res = _hip(scene, g, shadow=True)
    with torch.no_grad():
        plain = render(scene, device=DEV, shading="torch", shadow=True)
    bits = plain["light_visibility"].cpu().numpy()
    nl = np.asarray(scene["lights"]["pos"]).shape[0]
    vis = np.stack([((bits >> l) & 1).astype(np.float64).reshape(-1) for l in range(nl)])
    assert 0.02 < 1.0 - vis.mean() < 0.98                   # some lights are shadowed somewhere
    want = _helper(scene, g, res, visibility=vis)
    assert_grads_close(got, want, 2e-4, "shadow")
    unshadowed = _helper(scene, g, res)
    assert np.abs(want["camera.eye"] - unshadowed["camera.eye"]).max() > 1e-3 * np.abs(want["camera.eye"]).max()


def test_structure_and_reproducibility():
    npz, scene, kw = load("c1_camera_grad_phong")
    g = upstream(npz)
    a, _ = _hip(scene, g, **kw)
    b, _ = _hip(scene, g, **kw)
    for key in CAM_KEYS:
        assert a[key][3] == 0.0, key
        assert np.array_equal(a[key], b[key]), key          # the slab reduction: no atomics, a fixed order
    up = np.asarray(scene["camera"]["up"], dtype=np.float64)[:3]
    assert abs(np.dot(up, a["camera.up"][:3])) <= (2e-4 * np.abs(a["camera.up"]).max() + 1e-6) * np.linalg.norm(up)
    # a 3-vector up gets 3 values
    from surf_renderer_amd import render
    leaf_scene = copy.deepcopy(scene)
    up3 = torch.tensor(up, dtype=torch.float32, device=DEV, requires_grad=True)
    leaf_scene["camera"] = dict(leaf_scene["camera"], up=up3)
    masked_loss(render(leaf_scene, device=DEV, shading="torch", **kw), g, scene["camera"]["far"]).backward()
    assert up3.grad.shape == (3,)
    assert np.array_equal(up3.grad.cpu().numpy().astype(np.float64), a["camera.up"][:3])


def _bunny(ortho):
    from surf_renderer_amd import synthetic
    mesh = synthetic.bunny_mesh_scene(1024, 1024)
    if ortho:                                               # the same 1.4-unit view of the mesh: h = 2 f tan(fovy / 2)
        mesh["camera"].update({"proj_type": "ortho", "focal_length": 10.0})
    tri = mesh["objects"]["triangle"]
    leaves = {"triangle.face": torch.tensor(np.asarray(tri["face"], dtype=np.float32), device=DEV, requires_grad=True),
              "lights.pos": torch.tensor(np.asarray(mesh["lights"]["pos"], dtype=np.float32), device=DEV,
                                         requires_grad=True)}
    mesh["objects"]["triangle"] = dict(tri, face=leaves["triangle.face"])
    mesh["lights"]["pos"] = leaves["lights.pos"]
    cam = camera_leaves(mesh["camera"])
    mesh["camera"] = dict(mesh["camera"], **cam)
    return mesh, leaves, cam


@pytest.mark.parametrize("ortho", [False, True])
def test_translation_invariance_on_the_bunny(ortho):
    """Config 4 (bunny.obj at 1024 x 1024): moving camera, geometry and lights together changes neither image nor depth
    nor normal, so g_eye + g_at + sum g_face[:, 0] + sum g_lights_pos vanishes per component -- within 2e-4 of S, the sum
    of the absolute values of those terms.  (pos moves along with the scene, so it is not in this loss.)"""
    from surf_renderer_amd import render
    mesh, leaves, cam = _bunny(ortho)
    res = render(mesh, device=DEV, shading="torch", validate=False)
    gen = torch.Generator(device=DEV).manual_seed(5)
    hit = res["depth"].detach() <= mesh["camera"]["far"]
    assert 0.2 < float(hit.float().mean()) < 0.9
    loss = (res["image"] * (torch.rand(res["image"].shape, device=DEV, generator=gen) - 0.3)).sum() + \
        torch.where(hit, res["depth"] * (torch.rand(hit.shape, device=DEV, generator=gen) - 0.5),
                    torch.zeros_like(res["depth"])).sum() + \
        (res["normal"] * (torch.rand(res["normal"].shape, device=DEV, generator=gen) - 0.5)).sum()
    loss.backward()
    torch.cuda.synchronize()
    terms = [cam["eye"].grad[:3], cam["at"].grad[:3], *leaves["triangle.face"].grad[:, 0, :3],
             *leaves["lights.pos"].grad[:, :3]]
    terms = torch.stack([t.double() for t in terms]).cpu().numpy()
    residual, S = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    print("ortho" if ortho else "persp", "residual", residual, "S", S, "g_eye", terms[0], "g_at", terms[1])
    assert np.all(np.isfinite(terms)) and np.all(S > 1.0)
    assert np.abs(terms[0]).max() > 1e-3 * S.max()          # the camera terms take part
    assert np.all(np.abs(residual) <= 2e-4 * S)


def test_camera_only():
    """Nothing but the camera requires grad: the render is differentiable and the scene's tensors get no .grad."""
    from surf_renderer_amd import render
    npz, scene, kw = load("c1_camera_grad_phong")
    g = upstream(npz)
    want, _ = _hip(scene, g, **kw)
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
    for t in leaves.values():
        t.requires_grad_(False)
    cam = camera_leaves(scene["camera"])
    leaf_scene["camera"] = dict(leaf_scene["camera"], **cam)
    res = render(leaf_scene, device=DEV, shading="torch", **kw)
    assert res["image"].requires_grad and res["depth"].requires_grad
    masked_loss(res, g, scene["camera"]["far"]).backward()
    for k, t in leaves.items():
        assert t.grad is None, k
    for k in CAM:
        assert np.array_equal(cam[k].grad.cpu().numpy().astype(np.float64), want["camera." + k]), k
    # norm_depth_image_only: the image is a function of depth alone
    cam2 = camera_leaves(scene["camera"])
    leaf_scene["camera"] = dict(leaf_scene["camera"], **cam2)
    res = render(leaf_scene, device=DEV, shading="torch", norm_depth_image_only=True, **kw)
    res["image"].sum().backward()
    assert all(cam2[k].grad is not None and bool(torch.isfinite(cam2[k].grad).all()) for k in CAM)
    assert float(cam2["eye"].grad.abs().max()) > 0


def test_resident_scene_descent_follows_the_reference():
    """Ten Adam steps on eye and at through ResidentScene against the trajectory of the reference in float64
    (tests/golden/c2_camera_descent.npz).  Margin: 10 x the distance between the reference's own float32 and float64
    runs, not less than 1e-3 per component -- a thirtieth of one Adam step (lr 0.03): a missing or wrong-signed
    gradient component is off by a whole step after the first iteration."""
    from surf_renderer_amd import ResidentScene
    npz = np.load(os.path.join(GOLDEN_DIR, "c2_camera_descent.npz"), allow_pickle=False)
    scene = unpack_scene(npz)
    eye = torch.tensor(npz["start/eye"], dtype=torch.float32, device=DEV, requires_grad=True)
    at = torch.tensor(npz["start/at"], dtype=torch.float32, device=DEV, requires_grad=True)
    scene["camera"] = dict(scene["camera"], eye=eye, at=at)
    rs = ResidentScene(scene, device=DEV, shading="torch")
    target = torch.as_tensor(npz["target/image"], device=DEV)
    target_depth = torch.as_tensor(npz["target/depth"], device=DEV)
    far = float(scene["camera"]["far"])
    opt = torch.optim.Adam([eye, at], lr=float(npz["lr"]))
    losses = []
    for step in range(10):
        opt.zero_grad()
        res = rs.render()
        hit = res["depth"].detach() <= far
        loss = torch.mean((res["image"] - target) ** 2) + \
            0.05 * torch.mean(torch.where(hit, res["depth"] - target_depth, torch.zeros_like(target_depth)) ** 2)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        print(step, losses[-1], float(npz["loss"][step]), (eye.detach().cpu().numpy() - npz["eye"][step]),
              (at.detach().cpu().numpy() - npz["at"][step]))
    assert losses[-1] < losses[0]
    margin = max(10.0 * float(npz["spread"]), 1e-3)
    np.testing.assert_allclose(eye.detach().cpu().numpy().astype(np.float64), npz["eye"][9], rtol=0, atol=margin)
    np.testing.assert_allclose(at.detach().cpu().numpy().astype(np.float64), npz["at"][9], rtol=0, atol=margin)
    # the loss along the way: fp32 frames differ from the reference's by ~1e-6 per pixel; 1e-3 relative leaves room for a
    # pixel whose winner flips (1 / 1728 of the frame)
    np.testing.assert_allclose(losses, npz["loss"], rtol=1e-3)


def test_float64_cpu_camera_leaf():
    npz, scene, kw = load("c1_camera_grad_ortho")
    g = upstream(npz)
    want, _ = _hip(scene, g, **kw)
    from surf_renderer_amd import render
    leaf_scene = copy.deepcopy(scene)
    cam = camera_leaves(scene["camera"], device="cpu", dtype=torch.float64)
    leaf_scene["camera"] = dict(leaf_scene["camera"], **cam)
    masked_loss(render(leaf_scene, device=DEV, shading="torch", **kw), g, scene["camera"]["far"]).backward()
    for k in CAM:
        assert cam[k].grad.dtype == torch.float64 and cam[k].grad.device.type == "cpu" and cam[k].grad.shape == (4,)
        assert np.array_equal(cam[k].grad.numpy(), want["camera." + k]), k


def test_numpy_shading_keeps_detaching_the_camera():
    from surf_renderer_amd import render, synthetic
    scene = synthetic.splat_basic_scene(64, 48)
    pos = torch.tensor(np.asarray(scene["objects"]["disk"]["pos"], dtype=np.float32), device=DEV, requires_grad=True)
    scene["objects"]["disk"]["pos"] = pos
    eye = torch.tensor(scene["camera"]["eye"], dtype=torch.float32, device=DEV, requires_grad=True)
    scene["camera"] = dict(scene["camera"], eye=eye)
    render(scene, device=DEV)["image"].sum().backward()
    assert pos.grad is not None and eye.grad is None


def test_misses_and_scratch_reuse():
    """Workgroups that leave early (no hit pixel) must not leave a previous frame's partial sums behind: a 48 x 36 frame
    with misses, differentiated right after a full-hit 256 x 192 frame through the same ResidentScene (same scratch)."""
    from surf_renderer_amd import ResidentScene
    scene = full_scene(plane=False)
    small_cam = dict(scene["camera"])
    # looking straight at the largest disc (centre (0.5, 2, -1), radius 2.2) from 4 units away: every pixel hits
    big_cam = dict(scene["camera"], viewport=[0, 0, 256, 192], eye=[0.5, 2.0, 3.0, 1.0], at=[0.5, 2.0, -1.0, 1.0],
                   fovy=float(np.deg2rad(30.0)))
    g = random_upstream()

    def resident(camera):
        leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
        cam = camera_leaves(camera)
        leaf_scene["camera"] = dict(camera, **cam)
        return ResidentScene(leaf_scene, device=DEV, shading="torch", aux=True), leaves, cam

    def backward(rs, cam, upstream, mask=True):
        for t in cam.values():
            t.grad = None
        res = rs.render()
        masked_loss(res, upstream, scene["camera"]["far"], mask).backward()
        torch.cuda.synchronize()
        return {"camera." + k: cam[k].grad.cpu().numpy().astype(np.float64) for k in CAM}, res

    rs, _, cam_big = resident(big_cam)
    rng = np.random.RandomState(3)
    g_big = {"image": rng.uniform(-1, 1, size=(192, 256, 3)), "depth": rng.uniform(-1, 1, size=(192, 256)),
             "normal": rng.uniform(-1, 1, size=(192, 256, 3)), "pos": rng.uniform(-1, 1, size=(192, 256, 3))}
    big, bres = backward(rs, cam_big, g_big)
    assert bool((bres["depth"].detach() <= scene["camera"]["far"]).all())           # full hit: every slot written
    assert all(np.abs(big[k]).max() > 0.1 for k in CAM_KEYS)
    scratch = rs.buf.camera_scratch
    cam_small = camera_leaves(small_cam)
    rs.set_camera(dict(small_cam, **cam_small))
    got, res = backward(rs, cam_small, g)
    assert rs.buf.camera_scratch is scratch                                         # the same scratch
    miss = res["depth"].detach().cpu().numpy() > scene["camera"]["far"]
    assert 0.05 < miss.mean() < 0.95
    # at least one workgroup (4 rows x 64 pixels) of the small frame has no hit at all
    blocks = [miss[r:r + 4, :].all() for r in range(0, 36, 4)]
    print("miss share", miss.mean(), "workgroups without a hit:", sum(blocks), "of", len(blocks))
    assert sum(blocks) >= 1
    assert_grads_close(got, _helper(scene, g, res), 2e-4, "misses", keys=CAM_KEYS)
    fresh_rs, _, cam_fresh = resident(small_cam)
    fresh, _ = backward(fresh_rs, cam_fresh, g)
    for k in CAM_KEYS:
        assert np.array_equal(got[k], fresh[k]), k
    poisoned = dict(g)
    for k in ("depth", "normal", "pos"):
        poisoned[k] = np.where(miss if k == "depth" else miss[..., None], 1e30, g[k])
    hot, _ = backward(rs, cam_small, poisoned, mask=False)                          # the 1e30 reach the backward kernel
    for k in CAM_KEYS:
        assert np.array_equal(hot[k], got[k]), k
