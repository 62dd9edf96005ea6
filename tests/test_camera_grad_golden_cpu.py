"""The gradient oracle with the camera in its graph (oracle/torch_oracle.py: rays, gradients_tch with camera=True)
against the reference torch backend under autograd (tests/golden/c1_*.npz, oracle/golden_c1_c2.py -- the
sphere-free fixture scene, camera eye / at / up as leaves beside all others), against the same oracle on its numpy rays
(the camera outside the graph), and against central differences on the full scene with
spheres (where the reference's own camera gradients are NaN).

Distances seen when these tests were written (largest over the three fixtures):
  helper against grad64/camera.* (both fp64 runs of the same formulae)   8e-15 of the largest entry  (bound 1e-9)
  helper against the float32 grad/camera.*                               1.3e-5                      (bound 2e-3)
  camera gradients against central differences, step 1e-6                7.8e-6 of the largest entry (perspective, the
      up[0] component; every other component <= 3e-8; orthographic 3e-8)  (bound 5e-5).  The up[0] figure is the
      truncation term of the central difference, not an error of the gradient: it falls with the square of the step
      (7.8e-4 at 1e-5, 7.8e-6 at 1e-6, 3.4e-7 at 1e-7, where rounding takes over), so the bound leaves the measured
      truncation a factor of six and would still catch a gradient that is off in its fifth digit.
  translation identity residual                                          2e-14 against S ~ 10..40    (bound 1e-12 S)
"""
import copy

import numpy as np
import pytest
import torch

from grad_cases import full_scene, grad_kwargs, load, random_upstream, upstream
from oracle import np_oracle_tch, torch_oracle
from oracle.torch_oracle import gradients_tch

CASES = ["c1_camera_grad_phong", "c1_camera_grad_phong_ds_quartic", "c1_camera_grad_ortho"]


@pytest.mark.parametrize("ortho", [False, True])
def test_rays_equal_the_numpy_oracle(ortho):
    cam = full_scene(ortho)["camera"]
    assert np_oracle_tch.is_ortho(cam) == ortho
    eye, orig, d, H, W = torch_oracle.rays(cam, torch_oracle.make_camera_leaves(cam, requires_grad=False))
    if ortho:
        eye_np, orig_np, dvec, H2, W2 = np_oracle_tch.generate_rays_ortho(cam)
        np.testing.assert_allclose(orig.numpy(), orig_np, rtol=0, atol=1e-12)
        np.testing.assert_allclose(d.numpy(), np.broadcast_to(dvec[None, :], orig_np.shape), rtol=0, atol=1e-12)
    else:
        eye_np, ray_np, H2, W2 = np_oracle_tch.generate_rays(cam)
        np.testing.assert_allclose(d.numpy(), ray_np.T, rtol=0, atol=1e-12)
        np.testing.assert_allclose(orig.numpy(), np.broadcast_to(eye_np[None, :3], (H * W, 3)), rtol=0, atol=1e-12)
    assert (H, W) == (H2, W2)
    np.testing.assert_allclose(eye.numpy(), eye_np[:3], rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", CASES)
def test_camera_gradients_match_the_reference(case):
    npz, scene, kw = load(case)
    ref = {"nearest": npz["ref/nearest"], "depth": npz["ref/depth"].astype(np.float64)}
    assert (ref["depth"] <= scene["camera"]["far"]).all()          # the fixture frames hit something at every pixel
    got = gradients_tch(scene, ref=ref, camera=True, **grad_kwargs(upstream(npz)), **kw)
    for key in torch_oracle.CAMERA_KEYS:
        want64 = npz["grad64/" + key]
        dist = np.abs(got[key] - want64).max() / np.abs(want64).max()
        print(case, key, "against fp64 reference:", dist)
        assert dist <= 1e-9, (key, dist)
        want32 = npz["grad/" + key].astype(np.float64)
        dist32 = np.abs(got[key] - want32).max() / np.abs(want32).max()
        print(case, key, "against fp32 reference:", dist32)
        assert dist32 <= 2e-3, (key, dist32)
        assert got[key][3] == 0 and want64[3] == 0
        assert np.abs(want64).max() > 1.0                           # finite and far from zero
    # the scene leaves against the reference too (tolerance of tests/test_aux_grad_golden_cpu.py)
    checked = 0
    for key in npz.files:
        if key.startswith("grad/") and not key.startswith("grad/camera."):
            want = npz[key].astype(np.float64)
            g = got[key[5:]]
            if key[5:] in ("lights.pos", "plane.pos", "disk.pos"):
                g, want = g[:, :3], want[:, :3]
            np.testing.assert_allclose(g, want, atol=2e-3 * max(np.abs(want).max(), 1e-6), err_msg=key)
            checked += 1
    assert checked == 13


@pytest.mark.parametrize("ortho", [False, True])
@pytest.mark.parametrize("kw", [{}, {"double_sided": True, "use_quartic": True}])
def test_scene_leaf_gradients_equal_the_existing_helper(ortho, kw):
    """Once one copy of the oracle against another; since they became one core, its torch-ray path (camera leaves in the
    graph) against its numpy-ray path, scene leaf by scene leaf."""
    scene = full_scene(ortho)
    ref = np_oracle_tch.render(scene, **kw)
    g = grad_kwargs(random_upstream())
    want = gradients_tch(scene, g["grad_image"], g["grad_depth"], g["grad_normal"], g["grad_pos"], ref=ref, **kw)
    got = gradients_tch(scene, ref=ref, camera=True, **g, **kw)
    for key, w in want.items():
        np.testing.assert_allclose(got[key], w, rtol=0, atol=1e-12 * max(np.abs(w).max(), 1.0), err_msg=key)


def _translation_residual(scene, grads):
    """g_eye + g_at + every position gradient, per component, and S = the sum of their absolute values."""
    terms = [grads["camera.eye"][:3], grads["camera.at"][:3]]
    for kind in scene["objects"]:
        terms += list((grads[f"{kind}.face"][:, 0, :3] if kind == "triangle" else grads[f"{kind}.pos"][:, :3]))
    terms += list(grads["lights.pos"][:, :3])
    terms = np.asarray(terms)
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


@pytest.mark.parametrize("ortho", [False, True])
def test_full_scene_with_spheres(ortho):
    """Finite camera gradients where the reference's are NaN; equal to central differences of the helper's own loss
    with the winners frozen; and the translation identity: moving camera, geometry and lights together changes
    nothing."""
    scene = full_scene(ortho)
    ref = np_oracle_tch.render(scene)
    hit = ref["depth"] <= scene["camera"]["far"]
    sphere_first = sum((g["face"] if k == "triangle" else g["pos"]).shape[0]
                       for k, g in list(scene["objects"].items())[:list(scene["objects"]).index("sphere")])
    n_sph = scene["objects"]["sphere"]["pos"].shape[0]
    assert ((ref["nearest"] >= sphere_first) & (ref["nearest"] < sphere_first + n_sph) & hit).sum() > 20
    g = grad_kwargs(random_upstream())
    grads = gradients_tch(scene, ref=ref, camera=True, **g)
    for key in torch_oracle.CAMERA_KEYS:
        assert np.all(np.isfinite(grads[key])) and np.abs(grads[key]).max() > 0.1, key

    leaves = torch_oracle.make_leaves_tch(scene, requires_grad=False)

    def loss(cam_values):
        cl = {k: torch.tensor(v) for k, v in cam_values.items()}
        with torch.no_grad():
            return float(torch_oracle.loss_camera(scene, leaves, cl, ref, **g))

    base = {k: v.detach().numpy().copy() for k, v in torch_oracle.make_camera_leaves(scene["camera"]).items()}
    eps, worst = 1e-6, 0.0
    for key in torch_oracle.CAMERA_KEYS:
        for i in range(3):
            vals = []
            for sign in (+1, -1):
                moved = copy.deepcopy(base)
                moved[key][i] += sign * eps
                vals.append(loss(moved))
            fd = (vals[0] - vals[1]) / (2 * eps)
            scale = np.abs(grads[key]).max()
            worst = max(worst, abs(grads[key][i] - fd) / scale)
    print("ortho" if ortho else "persp", "camera gradients against central differences:", worst)
    assert worst <= 5e-5

    # image, depth and normal do not change when camera, geometry and lights move together; pos moves along, so a
    # loss on pos is left out of this identity
    inv = gradients_tch(scene, ref=ref, camera=True, **{k: v for k, v in g.items() if k != "grad_pos"})
    res, S = _translation_residual(scene, inv)
    print("translation residual", res, "S", S)
    assert np.all(np.abs(res) <= 1e-12 * S)
    # up enters through its direction only
    up = base["camera.up"][:3]
    assert abs(np.dot(up, grads["camera.up"][:3])) <= 1e-8 * np.abs(grads["camera.up"]).max() * np.linalg.norm(up)
