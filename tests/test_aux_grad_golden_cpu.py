"""The normal / pos side of the gradient oracle (oracle/torch_oracle.py: render_aux, gradients_tch with grad_normal /
grad_pos) against the reference torch backend under autograd (tests/golden/n1_*.npz, oracle/golden_n1.py): forward normal and pos at hit pixels, and every leaf gradient of
loss = sum image g_i + sum_hit (depth g_d + normal . g_n + pos . g_p).  The reference's sphere gradients are NaN (sqrt
under a mask, torch/utils.py:238-279), so the sphere leaves are pinned by central differences instead."""
import copy

import numpy as np
import pytest

from grad_cases import load
from oracle import np_oracle_tch, torch_oracle
from oracle.torch_oracle import gradients_tch, render_aux

CASES = ["n1_aux_grad_phong", "n1_aux_grad_phong_ds_quartic", "n1_aux_grad_ortho"]


@pytest.mark.parametrize("case", CASES)
def test_forward_normal_and_pos_match_the_reference(case):
    npz, scene, kw = load(case)
    ref = np_oracle_tch.render(scene, **kw)
    normal, pos, hit = render_aux(scene, torch_oracle.make_leaves_tch(scene, requires_grad=False), ref, **kw)
    same = (np.asarray(npz["ref/nearest"]) == ref["nearest"]) & hit.numpy()
    assert same.mean() > 0.995
    # float32 reference: the tolerances of tests/test_hip_torch_shading.py (normal 3e-4, pos 2e-4)
    np.testing.assert_allclose(normal.numpy()[same], npz["ref/normal"][same], atol=3e-4)
    np.testing.assert_allclose(pos.numpy()[same], npz["ref/pos"][same], atol=2e-4)
    assert np.all(normal.numpy()[~hit.numpy()] == 0) and np.all(pos.numpy()[~hit.numpy()] == 0)


@pytest.mark.parametrize("case", CASES)
def test_gradients_match_the_reference_torch_backend(case):
    npz, scene, kw = load(case)
    grads = gradients_tch(scene, *(npz["grad_in/" + k].astype(np.float64) for k in ("image", "depth", "normal", "pos")),
                          **kw)
    checked = 0
    for key in npz.files:
        if not key.startswith("grad/") or key.startswith("grad/sphere."):
            continue
        name = key[5:]
        want = npz[key].astype(np.float64)
        got = grads[name]
        if name in ("lights.pos", "plane.pos", "disk.pos"):
            got, want = got[:, :3], want[:, :3]
        scale = max(np.abs(want).max(), 1e-6)
        np.testing.assert_allclose(got, want, atol=2e-3 * scale, err_msg=name)
        checked += 1
    assert checked == 13
    assert np.isnan(npz["grad/sphere.pos"]).any()                  # documents why spheres are left out
    # the aux terms matter: the same loss without them gives other geometry gradients
    plain = torch_oracle.gradients_tch(scene, npz["grad_in/image"].astype(np.float64),
                                       npz["grad_in/depth"].astype(np.float64), **kw)
    for name in ("triangle.face", "disk.normal", "sphere.pos"):
        assert np.abs(grads[name] - plain[name]).max() > 1e-2 * np.abs(grads[name]).max(), name


@pytest.mark.parametrize("case", ["n1_aux_grad_phong", "n1_aux_grad_ortho"])
def test_sphere_gradients_are_consistent_with_finite_differences(case):
    npz, scene, kw = load(case)
    ref = np_oracle_tch.render(scene, **kw)
    g_n, g_p = npz["grad_in/normal"].astype(np.float64), npz["grad_in/pos"].astype(np.float64)
    grads = gradients_tch(scene, grad_normal=g_n, grad_pos=g_p, ref=ref, **kw)

    def loss(sc):
        normal, pos, hit = render_aux(sc, torch_oracle.make_leaves_tch(sc, requires_grad=False), ref, **kw)
        m = hit.numpy()[..., None]
        return float(np.sum(np.where(m, normal.numpy() * g_n + pos.numpy() * g_p, 0.0)))

    for key, idx in (("sphere.pos", (0, 0)), ("sphere.pos", (1, 2)), ("sphere.radius", (0,)), ("sphere.radius", (1,)),
                     ("triangle.face", (1, 0, 1)), ("disk.normal", (2, 1))):
        a, b = key.split(".")
        eps = 1e-6
        vals = []
        for sign in (+1, -1):
            sc = copy.deepcopy(scene)
            sc["objects"][a][b][idx] += sign * eps
            vals.append(loss(sc))
        fd = (vals[0] - vals[1]) / (2 * eps)
        np.testing.assert_allclose(grads[key][idx], fd, rtol=5e-5, atol=2e-7, err_msg=f"{key}{idx}")


def test_geometry_only_loss_leaves_shading_inputs_untouched():
    npz, scene, kw = load("n1_aux_grad_phong")
    grads = gradients_tch(scene, grad_normal=npz["grad_in/normal"].astype(np.float64),
                          grad_pos=npz["grad_in/pos"].astype(np.float64), **kw)
    for name in ("lights.pos", "lights.attenuation", "lights.ambient", "colors", "materials.albedo", "materials.coeffs"):
        assert np.all(grads[name] == 0), name
    assert np.abs(grads["plane.normal"]).max() > 0 and np.abs(grads["sphere.radius"]).max() > 0


def test_linearity_of_the_helper():
    npz, scene, kw = load("n1_aux_grad_ortho")
    ref = np_oracle_tch.render(scene, **kw)
    g = {k: npz["grad_in/" + k].astype(np.float64) for k in ("image", "depth", "normal", "pos")}
    both = gradients_tch(scene, g["image"], g["depth"], g["normal"], g["pos"], ref=ref, **kw)
    img = gradients_tch(scene, g["image"], g["depth"], ref=ref, **kw)
    aux = gradients_tch(scene, grad_normal=g["normal"], grad_pos=g["pos"], ref=ref, **kw)
    for k in both:
        np.testing.assert_allclose(both[k], img[k] + aux[k], rtol=1e-9, atol=1e-9 * max(np.abs(both[k]).max(), 1.0))
