"""GPU: differentiable ``normal`` and ``pos`` outputs of render(scene, shading='torch') (srh_render_bwd_aux, the kAux /
kImage variants of k_render_bwd_tch) against the fp64 oracle (oracle/torch_oracle.gradients_tch), which
tests/test_aux_grad_golden_cpu.py ties to the reference torch backend's autograd (tests/golden/n1_*.npz).

Stated tolerances: gradients per input array |got - want| <= 2e-4 * max|want| + 1e-6 (tests/test_hip_backward.py);
forward normal 3e-4 and pos 2e-4 at hit pixels against the float32 reference (tests/test_hip_torch_shading.py)."""
import copy

import numpy as np
import pytest
import torch

from grad_cases import (RUN_TO_RUN, TCH_KEYS, assert_grads_close, gpu_leaf_scene, grad_kwargs, leaf_grads, load,
                        masked_loss, upstream, winners)
from grad_fuzz_cases import _fuzz_scene
from oracle import np_oracle_tch
from oracle.torch_oracle import OUTPUTS, gradients_tch

pytestmark = pytest.mark.gpu

CASES = ["n1_aux_grad_phong", "n1_aux_grad_phong_ds_quartic", "n1_aux_grad_ortho"]


def _hip(scene, g, rows=None, mask=True, **kw):
    """render() with GPU leaves and masked_loss over the outputs named in g; returns ({leaf: grad ndarray}, result)."""
    from surf_renderer_amd import render
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
    res = render(leaf_scene, device="cuda:0", shading="torch", rows=rows, **kw)
    masked_loss(res, g, scene["camera"]["far"], mask).backward()
    torch.cuda.synchronize()
    return leaf_grads(leaves), res


@pytest.mark.parametrize("case", CASES)
def test_reference_fixtures_through_render(case):
    npz, scene, kw = load(case)
    g = upstream(npz)
    got, res = _hip(scene, g, **kw)
    assert res["normal"].requires_grad and res["pos"].requires_grad
    # forward, at hit pixels won by the reference's primitive
    same = (res["nearest"].cpu().numpy() == npz["ref/nearest"]) & (npz["ref/depth"] <= scene["camera"]["far"])
    assert same.mean() > 0.995
    np.testing.assert_allclose(res["normal"].detach().cpu().numpy()[same], npz["ref/normal"][same], atol=3e-4)
    np.testing.assert_allclose(res["pos"].detach().cpu().numpy()[same], npz["ref/pos"][same], atol=2e-4)
    # every leaf against the fp64 helper, and against the reference's own gradients where those are finite
    want = gradients_tch(scene, g["image"], g["depth"], g["normal"], g["pos"], ref=winners(res), **kw)
    assert_grads_close(got, want, 2e-4, case)
    for key in npz.files:
        if key.startswith("grad/") and not key.startswith("grad/sphere."):
            ref = npz[key].astype(np.float64)
            np.testing.assert_allclose(got[key[5:]].reshape(ref.shape)[..., :3], ref[..., :3],
                                       atol=2e-3 * max(np.abs(ref).max(), 1e-6), err_msg=key)


@pytest.mark.parametrize("case", ["n1_aux_grad_phong", "n1_aux_grad_ortho"])
@pytest.mark.parametrize("which", ["normal", "pos"])
def test_geometry_only_losses(case, which):
    """A loss on normal or pos alone runs the geometry-only kernel: no light / colour / material gradient."""
    npz, scene, kw = load(case)
    g = upstream(npz, which)
    got, res = _hip(scene, g, **kw)
    assert_grads_close(got, gradients_tch(scene, **grad_kwargs(g), ref=winners(res), **kw), 2e-4, which)
    for key in TCH_KEYS:
        assert np.all(got[key] == 0), key


def test_gradients_are_linear_in_the_losses():
    npz, scene, kw = load("n1_aux_grad_phong_ds_quartic")
    g = upstream(npz)
    both, _ = _hip(scene, g, **kw)
    parts = [_hip(scene, {k: g[k] for k in keys}, **kw)[0] for keys in (("image", "depth"), ("normal",), ("pos",))]
    assert_grads_close(both, {k: sum(p[k] for p in parts) for k in both}, 2e-4, "sum of parts")


def test_huge_upstream_gradients_on_misses_change_nothing():
    """normal and pos are the constant 0 where nothing is hit: whatever arrives there from upstream is ignored."""
    npz, scene, kw = load("n1_aux_grad_phong")
    scene = copy.deepcopy(scene)
    del scene["objects"]["plane"]                      # the background plane: without it, part of the frame misses
    g = upstream(npz)
    base, res = _hip(scene, g, **kw)
    miss = res["depth"].detach().cpu().numpy() > scene["camera"]["far"]
    assert 0.05 < miss.mean() < 0.95
    assert_grads_close(base, gradients_tch(scene, g["image"], g["depth"], g["normal"], g["pos"], ref=winners(res), **kw), 2e-4)
    poisoned = dict(g)
    for k in ("depth", "normal", "pos"):
        poisoned[k] = np.where(miss if k == "depth" else miss[..., None], 1e30, g[k])
    got, _ = _hip(scene, poisoned, mask=False, **kw)           # the 1e30 reach the backward kernel
    for key, w in base.items():
        assert np.all(np.isfinite(got[key])), key
        np.testing.assert_allclose(got[key], w, rtol=0, atol=RUN_TO_RUN * np.abs(w).max() + 1e-7, err_msg=key)


def test_shadow_rays_do_not_change_geometry_gradients():
    npz, scene, kw = load("n1_aux_grad_phong")
    g = upstream(npz, "depth", "normal", "pos")
    lit, _ = _hip(scene, g, **kw)
    shadowed, res = _hip(scene, g, shadow=True, **kw)
    assert res["normal"].requires_grad and res["pos"].requires_grad
    for key, w in lit.items():
        np.testing.assert_allclose(shadowed[key], w, rtol=0, atol=RUN_TO_RUN * np.abs(w).max() + 1e-7, err_msg=key)


def test_row_slab_equals_the_rows_of_the_full_frame():
    npz, scene, kw = load("n1_aux_grad_ortho")
    r0, r1 = 9, 25
    g = upstream(npz)
    rows = np.arange(g["image"].shape[0])
    inside = (rows >= r0) & (rows < r1)
    full_g = {k: v * (inside[:, None, None] if v.ndim == 3 else inside[:, None]) for k, v in g.items()}
    full, fres = _hip(scene, full_g, **kw)
    slab, sres = _hip(scene, {k: v[r0:r1] for k, v in g.items()}, rows=(r0, r1), **kw)
    assert sres["normal"].shape == (r1 - r0, g["image"].shape[1], 3)
    for k in ("normal", "pos"):
        assert torch.equal(sres[k].detach(), fres[k].detach()[r0:r1]), k
    assert_grads_close(slab, full, 2e-4, "slab")


def test_fuzz_against_the_helper():
    """24 random scenes with all four primitive types, every third one orthographic, random double_sided / use_quartic
    and a random subset of the four outputs in the loss (normal or pos always among them).  Tolerance 5e-4 of the
    largest entry per array, as in the image / depth fuzz of tests/test_hip_backward.py."""
    from surf_renderer_amd.scene import scene_to_numpy
    rng = np.random.RandomState(2611)
    for it in range(24):
        ortho = it % 3 == 2
        scene = scene_to_numpy(_fuzz_scene(rng, ortho), round_fp32=True)
        kw = {"double_sided": bool(rng.randint(2)), "use_quartic": bool(rng.randint(2))}
        W, H = scene["camera"]["viewport"][2:]
        keys = [k for k in OUTPUTS if rng.randint(2)]
        if "normal" not in keys and "pos" not in keys:
            keys.append(str(rng.choice(["normal", "pos"])))
        g = {k: rng.uniform(-1, 1, size=(H, W, 3) if k != "depth" else (H, W)).astype(np.float32).astype(np.float64)
             for k in keys}
        got, res = _hip(scene, g, **kw)
        ref = np_oracle_tch.render(scene, **kw)
        assert (res["nearest"].cpu().numpy() == ref["nearest"]).mean() > 0.999, it
        want = gradients_tch(scene, *(g.get(k) for k in OUTPUTS), ref=winners(res), **kw)
        assert_grads_close(got, want, 5e-4, f"scene {it} {kw} {keys} ortho={ortho}")


def test_captured_step_with_a_normal_loss_equals_the_eager_iteration():
    from surf_renderer_amd import ResidentScene, synthetic
    scene = synthetic.bunny_mesh_scene(160, 128)
    tri = scene["objects"]["triangle"]
    face = torch.tensor(np.asarray(tri["face"], dtype=np.float32), device="cuda:0", requires_grad=True)
    normal = torch.tensor(np.asarray(tri["normal"], dtype=np.float32), device="cuda:0", requires_grad=True)
    scene["objects"]["triangle"] = dict(tri, face=face, normal=normal)
    with pytest.raises(ValueError):
        ResidentScene(scene, device="cuda:0", aux=True)          # numpy shading has no normal / pos
    assert "normal" not in ResidentScene(scene, device="cuda:0", shading="torch").render()     # opt-in
    rs = ResidentScene(scene, device="cuda:0", shading="torch", aux=True)
    target = torch.rand((128, 160, 3), device="cuda:0")
    t_nrm = torch.rand((128, 160, 3), device="cuda:0") - 0.5

    def loss_fn(res):
        return ((res["image"] - target) ** 2).sum() + (res["normal"] * t_nrm).sum() + 0.01 * res["pos"].sum()

    def eager():
        face.grad = None
        normal.grad = None
        loss = loss_fn(rs.render())
        loss.backward()
        return loss.detach().clone(), face.grad.clone(), normal.grad.clone()

    step = rs.capture_step(loss_fn)
    assert step.result["normal"].requires_grad
    for it in range(3):
        want = eager()
        face.grad = None
        normal.grad = None
        got_loss = step.replay().clone()
        torch.cuda.synchronize()
        got = (got_loss, face.grad.clone(), normal.grad.clone())
        torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=0)
        for g, w in zip(got[1:], want[1:]):
            torch.testing.assert_close(g, w, rtol=1e-4, atol=1e-6 * float(w.abs().max()))
        with torch.no_grad():                            # an optimiser step, in place, and a new normal target
            face[:, 0, :3] += 0.002 * torch.randn_like(face[:, 0, :3])
            t_nrm.copy_(torch.rand_like(t_nrm) - 0.5)
