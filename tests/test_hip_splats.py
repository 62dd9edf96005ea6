"""GPU: render_splats_along_ray / render_splats_along_ray_batch (srh_splat_fwd / srh_splat_bwd) against the fp64
restatement tests/splat_oracle.py, which tests/test_splat_oracle_cpu.py ties to the reference (tests/golden/p1_*.npz).

Stated tolerances, as tests/test_hip_torch_shading.py and tests/test_hip_aux_grad.py: the kernels compute the
restatement's fp64 arithmetic and store fp32, so outputs match to fp32 rounding (rtol 2e-6, atol 2e-7 relative to the
output's largest entry); gradients per input array |got - want| <= 2e-4 max|want| + 1e-6 (scene parameters leave as
fp32 atomic sums).  Against the float32 reference itself the tolerances of tests/test_splat_oracle_cpu.py apply."""
import os

import numpy as np
import pytest
import torch

import splat_oracle
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.splitext(f)[0] for f in os.listdir(GOLDEN_DIR) if f.startswith("p1_") and f.endswith(".npz"))
DEV = "cuda:0"
_GPU_LEAVES = {"disk.pos": ("objects", "disk", "pos"), "disk.normal": ("objects", "disk", "normal"),
               "disk.light_vis": ("objects", "disk", "light_vis"), "lights.pos": ("lights", "pos"),
               "lights.attenuation": ("lights", "attenuation"), "lights.ambient": ("lights", "ambient"),
               "colors": ("colors",), "materials.albedo": ("materials", "albedo"),
               "materials.coeffs": ("materials", "coeffs")}


def _load(case):
    npz = np.load(os.path.join(GOLDEN_DIR, case + ".npz"), allow_pickle=False)
    return npz, splat_oracle.unpack(npz), splat_oracle.kwargs_of(npz)


def _gpu_scene(scene):
    """The scene with fp32 GPU leaves (requires_grad) for every differentiable input; returns (scene, leaves)."""
    import copy
    sc = copy.deepcopy(scene)
    leaves = {}
    for name, path in _GPU_LEAVES.items():
        d = sc
        for p in path[:-1]:
            d = d[p]
        if path[-1] not in d or d[path[-1]] is None:
            continue
        t = torch.tensor(np.asarray(d[path[-1]], dtype=np.float32), device=DEV, requires_grad=True)
        d[path[-1]] = leaves[name] = t
    sc["lights"]["color_idx"] = torch.as_tensor(np.asarray(sc["lights"]["color_idx"]), device=DEV)
    md = sc["objects"]["disk"].get("material_idx")
    if md is not None:
        sc["objects"]["disk"]["material_idx"] = torch.as_tensor(np.asarray(md), device=DEV)
    return sc, leaves


def _hip(scene, up, **kw):
    from surf_renderer_amd import render_splats_along_ray
    sc, leaves = _gpu_scene(scene)
    res = render_splats_along_ray(sc, normal_estimation_method="plane", **kw)
    loss = sum(torch.sum(res[k] * torch.as_tensor(up[k], dtype=torch.float32, device=DEV)) for k in up)
    loss.backward()
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in res.items()}
    grads = {k: t.grad.cpu().numpy().astype(np.float64) if t.grad is not None else np.zeros(tuple(t.shape))
             for k, t in leaves.items()}
    return out, grads


def _compare_outputs(got, want, tag):
    for k, w in want.items():
        w = np.asarray(w, dtype=np.float64)
        g = got[k].reshape(w.shape)
        np.testing.assert_allclose(g, w, rtol=2e-6, atol=2e-7 * max(np.abs(w).max(), 1.0), err_msg=f"{tag} {k}")


def _compare_grads(got, want, tag, tol=2e-4):
    for k, w in want.items():
        assert np.all(np.isfinite(w)), (tag, k)
        g = got[k].reshape(w.shape)
        np.testing.assert_allclose(g, w, rtol=0, atol=tol * np.abs(w).max() + 1e-6, err_msg=f"{tag} {k}")


@pytest.mark.parametrize("case", CASES)
def test_forward_and_gradients_match_the_restatement_and_the_reference(case):
    npz, scene, kw = _load(case)
    up = {k: npz["grad_in/" + k] for k in splat_oracle.OUTPUTS}
    got, got_g = _hip(scene, up, **kw)
    want, want_g = splat_oracle.gradients(scene, up, **kw)
    _compare_outputs(got, want, case)
    _compare_grads(got_g, want_g, case)
    given = "in/disk.normal" in npz.files
    for k in splat_oracle.OUTPUTS:                         # the float32 reference (tests/test_splat_oracle_cpu.py)
        w = npz["ref/" + k].astype(np.float64)
        tol = 2e-3 if (k == "normal" and not given) else 2e-5 * max(np.abs(w).max(), 1.0)
        np.testing.assert_allclose(got[k].reshape(w.shape), w, rtol=0, atol=tol, err_msg=f"{case} ref {k}")
    for key in npz.files:
        if key.startswith("grad/"):
            w = npz[key].astype(np.float64)
            np.testing.assert_allclose(got_g[key[5:]].reshape(w.shape), w, rtol=0, atol=3e-3 * max(np.abs(w).max(), 1e-6),
                                       err_msg=f"{case} ref {key}")


def test_sub_pixel_order_at_two_samples_on_a_non_square_frame():
    _, scene, _ = _load("p1_samples2_20x28")
    from surf_renderer_amd import render_splats_along_ray
    sc, _ = _gpu_scene(scene)
    with torch.no_grad():
        res = render_splats_along_ray(sc, samples=2)
    pos = res["pos"].cpu().numpy()
    assert pos.shape == (40, 56, 3)
    # the x shift of a splat's sub-pixels runs down the output rows, the y shift along them (reshape_upsampled_data)
    blk = pos[0:2, 0:2]
    xr = blk[..., 0] / -blk[..., 2]
    yr = blk[..., 1] / -blk[..., 2]
    assert xr[1, 0] > xr[0, 0] and abs(xr[0, 1] - xr[0, 0]) < 1e-6 * abs(xr[0, 0])
    assert yr[0, 1] < yr[0, 0] and abs(yr[1, 0] - yr[0, 0]) < 1e-6 * abs(yr[0, 0])
    want = splat_oracle.render(scene, splat_oracle.make_leaves(scene, requires_grad=False), samples=2)
    np.testing.assert_allclose(pos, want["pos"].numpy(), rtol=2e-6, atol=1e-6)


def _batch_scene(B, H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    z = np.stack([-(4.0 + 0.5 * np.sin(2 * xx + b) * np.cos(1.5 * yy) + 0.3 * b * xx * yy) for b in range(B)])
    z = (z + 0.02 * rng.standard_normal(z.shape)).reshape(B, H * W)
    n = np.stack([rng.uniform(-0.3, 0.3, (B, H * W)), rng.uniform(-0.3, 0.3, (B, H * W)),
                  rng.uniform(0.8, 1.1, (B, H * W))], -1)
    eye = np.stack([[0.5 + 0.3 * b, 1.0 - 0.2 * b, 6.0, 1.0] for b in range(B)])
    lpos = np.stack([[[3.0 - b, 4.0, 8.0, 1.0], [-4.0, 1.0 + b, 5.0, 1.0]] for b in range(B)])
    return {
        "camera": {"viewport": [0, 0, W, H], "fovy": float(np.deg2rad(45.0)), "focal_length": 0.8, "eye": eye,
                   "at": np.array([0.1, -0.2, 0.0, 1.0]), "up": np.array([0.2, 1.0, 0.3, 0.0]), "far": 100.0},
        "lights": {"pos": lpos, "color_idx": np.array([1, 2]),
                   "attenuation": np.array([[1.0, 0.0, 0.0], [0.6, 0.04, 0.003]]), "ambient": np.array([0.05, 0.04, 0.06])},
        "colors": np.array([[0, 0, 0], [0.9, 0.8, 0.7], [0.3, 0.5, 0.9]]),
        "materials": {"albedo": np.array([[0.7, 0.6, 0.5], [0.3, 0.8, 0.4]]),
                      "coeffs": np.array([[0.8, 0.2, 5.0], [0.6, 0.4, 12.0]])},
        "objects": {"disk": {"pos": z.astype(np.float32), "normal": n.astype(np.float32),
                             "material_idx": (rng.uniform(size=H * W) < 0.4).astype(np.int64)}},
    }


def _view(scene, b, keep_normal=True):
    import copy
    sc = copy.deepcopy(scene)
    sc["camera"]["eye"] = scene["camera"]["eye"][b]
    sc["lights"]["pos"] = scene["lights"]["pos"][b]
    sc["objects"]["disk"]["pos"] = scene["objects"]["disk"]["pos"][b]
    if keep_normal:
        sc["objects"]["disk"]["normal"] = scene["objects"]["disk"]["normal"][b]
    else:
        sc["objects"]["disk"].pop("normal", None)
    return sc


@pytest.mark.parametrize("given", [True, False])
def test_batched_equals_single_calls_bit_for_bit(given):
    from surf_renderer_amd import render_splats_along_ray, render_splats_along_ray_batch
    B, H, W = 3, 24, 32
    scene = _batch_scene(B, H, W, 1)
    if not given:
        scene["objects"]["disk"].pop("normal")
    up = np.random.RandomState(4).uniform(-1, 1, (B, H, W, 3)).astype(np.float32)
    sc, leaves = _gpu_scene(scene)
    res = render_splats_along_ray_batch(sc, samples=2)
    (res["image"].sum() + (res["pos"] * torch.as_tensor(np.repeat(np.repeat(up, 2, 1), 2, 2), device=DEV)).sum()
     + res["depth"].sum()).backward()
    for b in range(B):
        one, one_leaves = _gpu_scene(_view(scene, b, given))
        r1 = render_splats_along_ray(one, samples=2)
        (r1["image"].sum() + (r1["pos"] * torch.as_tensor(np.repeat(np.repeat(up[b], 2, 0), 2, 1), device=DEV)).sum()
         + r1["depth"].sum()).backward()
        for k in ("image", "depth", "pos", "normal"):
            assert torch.equal(res[k][b], r1[k]), (b, k)
        assert torch.equal(leaves["disk.pos"].grad[b], one_leaves["disk.pos"].grad), b
        # scene parameters are fp32 atomic sums: equal up to the order of the additions
        _compare_grads({"l": leaves["lights.pos"].grad[b].cpu().numpy()},
                       {"l": one_leaves["lights.pos"].grad.cpu().numpy().astype(np.float64)}, f"view {b}", tol=2e-5)
        if given:
            assert torch.equal(leaves["disk.normal"].grad[b], one_leaves["disk.normal"].grad), b


def test_batched_gradients_of_shared_normals_and_light_vis_are_the_sums_over_views():
    from surf_renderer_amd import render_splats_along_ray, render_splats_along_ray_batch
    B, H, W = 3, 24, 32
    scene = _batch_scene(B, H, W, 3)
    d = scene["objects"]["disk"]
    d["normal"] = d["normal"][0]                                            # [N, 3], shared by every view
    d["light_vis"] = np.random.RandomState(8).uniform(0, 1, (2, H * W)).astype(np.float32)      # [L, N], shared
    up = np.random.RandomState(9).uniform(-1, 1, (B, H, W, 3)).astype(np.float32)
    sc, leaves = _gpu_scene(scene)
    res = render_splats_along_ray_batch(sc)
    ((res["image"] * torch.as_tensor(up, device=DEV)).sum() + res["depth"].sum()).backward()
    want = {"disk.normal": 0.0, "disk.light_vis": 0.0}
    for b in range(B):
        one = _view(scene, b, keep_normal=False)
        one["objects"]["disk"]["normal"] = d["normal"]
        one_sc, one_leaves = _gpu_scene(one)
        r1 = render_splats_along_ray(one_sc)
        ((r1["image"] * torch.as_tensor(up[b], device=DEV)).sum() + r1["depth"].sum()).backward()
        for k in want:
            want[k] = want[k] + one_leaves[k].grad.cpu().numpy().astype(np.float64)
    got = {k: leaves[k].grad.cpu().numpy().astype(np.float64) for k in want}
    assert got["disk.normal"].shape == (H * W, 3) and got["disk.light_vis"].shape == (2, H * W)
    # each view's per-pixel gradient is written as the single call writes it; only the fp32 sum over views may round
    _compare_grads(got, want, "shared", tol=1e-6)


def test_geometry_only_frames_give_no_light_vis_or_shading_gradients():
    from surf_renderer_amd import render_splats_along_ray
    npz, scene, _ = _load("p1_given_normals_vis_30x40")
    sc, leaves = _gpu_scene(scene)
    assert "disk.light_vis" in leaves
    res = render_splats_along_ray(sc, norm_depth_image_only=True)
    (res["image"].sum() + res["depth"].sum() + res["pos"].sum() + res["normal"].sum()).backward()
    torch.cuda.synchronize()
    for k in ("disk.light_vis", "lights.pos", "colors", "lights.attenuation", "lights.ambient", "materials.albedo",
              "materials.coeffs"):
        g = leaves[k].grad
        assert g is None or bool(torch.all(g == 0)), k               # the reference's autograd gives None
    assert torch.isfinite(leaves["disk.pos"].grad).all() and torch.isfinite(leaves["disk.normal"].grad).all()
    want = splat_oracle.gradients(scene, {k: np.ones(tuple(res[k].shape)) for k in ("image", "depth", "pos", "normal")},
                                  norm_depth_image_only=True)[1]
    _compare_grads({k: leaves[k].grad.cpu().numpy() for k in ("disk.pos", "disk.normal")},
                   {k: want[k] for k in ("disk.pos", "disk.normal")}, "geometry only")


def test_per_pixel_gradients_are_identical_across_runs():
    npz, scene, kw = _load("p1_samples3_12x16")
    up = {k: npz["grad_in/" + k] for k in splat_oracle.OUTPUTS}
    _, g1 = _hip(scene, up, **kw)
    _, g2 = _hip(scene, up, **kw)
    for k in ("disk.pos", "disk.light_vis"):
        assert np.array_equal(g1[k], g2[k]), k
    npz, scene, kw = _load("p1_given_normals_vis_30x40")
    up = {k: npz["grad_in/" + k] for k in splat_oracle.OUTPUTS}
    _, g1 = _hip(scene, up, **kw)
    _, g2 = _hip(scene, up, **kw)
    for k in ("disk.pos", "disk.normal", "disk.light_vis"):
        assert np.array_equal(g1[k], g2[k]), k


@pytest.mark.parametrize("B,size", [(64, 128), (1, 512)])
def test_large_frames_match_the_restatement(B, size):
    from surf_renderer_amd import render_splats_along_ray_batch
    scene = _batch_scene(B, size, size, 2)
    scene["objects"]["disk"].pop("normal")
    sc, leaves = _gpu_scene(scene)
    res = render_splats_along_ray_batch(sc)
    rng = np.random.RandomState(5)
    g_img = rng.uniform(-1, 1, (B, size, size, 3)).astype(np.float32)
    (res["image"] * torch.as_tensor(g_img, device=DEV)).sum().backward()
    img = res["image"].detach().cpu().numpy()
    gz = leaves["disk.pos"].grad.cpu().numpy()
    glp = leaves["lights.pos"].grad.cpu().numpy()
    views = range(B) if B <= 4 else (0, 17, B - 1)
    for b in views:
        one = _view(scene, b, keep_normal=False)
        want, want_g = splat_oracle.gradients(one, {"image": g_img[b]})
        np.testing.assert_allclose(img[b], want["image"], rtol=2e-6, atol=2e-7 * max(np.abs(want["image"]).max(), 1.0))
        _compare_grads({"disk.pos": gz[b], "lights.pos": glp[b]},
                       {"disk.pos": want_g["disk.pos"], "lights.pos": want_g["lights.pos"]}, f"view {b}")


def test_a_camera_that_requires_grad_is_refused():
    from surf_renderer_amd import render_splats_along_ray
    _, scene, _ = _load("p1_estimated_36x48")
    sc, _ = _gpu_scene(scene)
    sc["camera"]["eye"] = torch.tensor(np.asarray(scene["camera"]["eye"], dtype=np.float32), device=DEV,
                                       requires_grad=True)
    with pytest.raises(ValueError, match="camera"):
        render_splats_along_ray(sc)


def test_other_normal_estimation_methods_are_refused():
    from surf_renderer_amd import render_splats_along_ray
    _, scene, _ = _load("p1_estimated_36x48")
    sc, _ = _gpu_scene(scene)
    with pytest.raises(ValueError, match="avg_normal"):
        render_splats_along_ray(sc, normal_estimation_method="avg_normal")
