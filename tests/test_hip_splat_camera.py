"""GPU: camera_grad=True of render_splats_along_ray / render_splats_NDC and their batch forms (srh_splat_bwd_view /
srh_splat_ndc_bwd_view) against the reference's own float64 and float32 records (tests/golden/splat_camera/sc1_*.npz)
and the fp64 restatement with camera leaves (tests/splat_camera_oracle.py).

Tolerances.  The camera sums leave the device as fp64 without atomics and the chain to eye / at / up is fp64 on the
host, so against the float64 record and the restatement they are held to the camera layers' stated tolerance (tests/
test_hip_dense_camera.py): rtol 2e-6, atol 2e-7 max|want| per array.  Against the float32 record: atol 3e-3
max(max|want|, 1e-6), the figure tests/test_hip_splats.py and test_hip_splats_ndc.py use for the float32 reference.
The atomic scene-parameter gradients keep test_hip_splats.py's atol 2e-4 max|want| + 1e-6.

Every test that passes camera_grad=True fails without the feature: the call raises ValueError there."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

import splat_camera_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splat_camera")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "sc1_*.npz")))
CAMERA = ("camera.eye", "camera.at", "camera.up")
WRITTEN = ("disk.pos", "disk.normal", "disk.light_vis")          # written by the lane that owns the pixel: no atomics
_LEAVES = {"disk.pos": ("objects", "disk", "pos"), "disk.normal": ("objects", "disk", "normal"),
           "disk.light_vis": ("objects", "disk", "light_vis"), "lights.pos": ("lights", "pos"), "colors": ("colors",),
           "lights.attenuation": ("lights", "attenuation"), "lights.ambient": ("lights", "ambient"),
           "materials.albedo": ("materials", "albedo"), "materials.coeffs": ("materials", "coeffs"),
           "camera.eye": ("camera", "eye"), "camera.at": ("camera", "at"), "camera.up": ("camera", "up")}


def _load(name):
    return oracle.load(os.path.join(GOLDEN, f"sc1_{name}.npz"))


def _gpu_scene(scene, camera=True, others=True, camera_dtype=torch.float32, camera_device=DEV):
    """The scene with GPU leaves; `camera` / `others`: whether eye, at, up / every other differentiable input requires
    grad.  Returns (scene, leaves)."""
    sc = copy.deepcopy(scene)
    leaves = {}
    for name, path in _LEAVES.items():
        d = sc
        for p in path[:-1]:
            d = d[p]
        if d.get(path[-1]) is None:
            continue
        cam = name in CAMERA
        t = torch.tensor(np.asarray(d[path[-1]], dtype=np.float32), dtype=camera_dtype if cam else torch.float32,
                         device=camera_device if cam else DEV, requires_grad=camera if cam else others)
        d[path[-1]] = leaves[name] = t
    sc["lights"]["color_idx"] = torch.as_tensor(np.asarray(sc["lights"]["color_idx"]), device=DEV)
    md = sc["objects"]["disk"].get("material_idx")
    if md is not None:
        sc["objects"]["disk"]["material_idx"] = torch.as_tensor(np.asarray(md), device=DEV)
    return sc, leaves


def _entry(kind, batched):
    import surf_renderer_amd as S
    return {("along_ray", False): S.render_splats_along_ray, ("along_ray", True): S.render_splats_along_ray_batch,
            ("ndc", False): S.render_splats_NDC, ("ndc", True): S.render_splats_NDC_batch}[kind, batched]


def _upstreams(res, g_image, only_image=False):
    """image's recorded upstream; for the other outputs seeded ones in (-1, 1) of their own shapes."""
    ups = {"image": torch.as_tensor(g_image, dtype=torch.float32, device=DEV)}
    if not only_image:
        rng = np.random.RandomState(41)
        for k in ("depth", "pos", "normal"):
            ups[k] = torch.as_tensor(rng.uniform(-1, 1, tuple(res[k].shape)).astype(np.float32), device=DEV)
    return ups


def _run(kind, scene, kw, g_image, camera_grad=True, only_image=False, outputs=None, **leaf_kw):
    """(outputs, {leaf: .grad or None}) of one call and its backward."""
    sc, leaves = _gpu_scene(scene, camera=camera_grad, **leaf_kw)
    extra = {"camera_grad": True} if camera_grad else {}
    res = _entry(kind, bool(oracle.n_views(kind, scene)))(sc, **kw, **extra)
    ups = _upstreams(res, g_image, only_image)
    loss = sum(torch.sum(res[k] * ups[k]) for k in (outputs or ups) if res[k].requires_grad)
    loss.backward()
    torch.cuda.synchronize()
    return {k: v.detach() for k, v in res.items()}, {k: t.grad for k, t in leaves.items()}


_RUNS = {}


def _full(name):
    """The case's run with every leaf requiring grad, computed once and shared."""
    if name not in _RUNS:
        kind, scene, kw, g_image, *_ = _load(name)
        _RUNS[name] = _run(kind, scene, kw, g_image)
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_camera_gradients_match_both_records_and_the_restatement(name):
    kind, scene, kw, g_image, want, meta = _load(name)
    _, grads = _full(name)
    restated = oracle.batch_gradients(kind, scene, g_image, **kw)
    for k in CAMERA:
        g = grads[k]
        shape = np.shape(scene["camera"][k.split(".")[1]])
        assert g is not None and tuple(g.shape) == shape and g.dtype == torch.float32 and g.device.type == "cuda", k
        got = g.cpu().numpy().astype(np.float64)
        assert np.all(got[..., 3:] == 0), k                                  # the reference slices [:3]
        for tag, w in (("float64 record", want["64"][k]), ("restatement", restated[k])):
            big = np.abs(w).max()
            err = np.abs(got - w)
            print(f"{name} {k} vs {tag}: max err {err.max():.3g} = {err.max() / big:.3g} of max|want| {big:.4g}")
        big32 = max(np.abs(want["32"][k]).max(), 1e-6)
        print(f"{name} {k} vs float32 record: {np.abs(got - want['32'][k]).max() / big32:.3g} of max|want|")
    for k in CAMERA:
        got = grads[k].cpu().numpy().astype(np.float64)
        for tag, w in (("float64 record", want["64"][k]), ("restatement", restated[k])):
            np.testing.assert_allclose(got, w, rtol=2e-6, atol=2e-7 * np.abs(w).max(), err_msg=f"{name} {k} {tag}")
        w = want["32"][k]
        np.testing.assert_allclose(got, w, rtol=0, atol=3e-3 * max(np.abs(w).max(), 1e-6), err_msg=f"{name} {k} float32")


@pytest.mark.parametrize("name", CASES)
def test_outputs_and_every_other_gradient_are_the_detached_call_s(name):
    kind, scene, kw, g_image, *_ = _load(name)
    res, grads = _full(name)
    res0, grads0 = _run(kind, scene, kw, g_image, camera_grad=False)
    assert set(res) == set(res0) == {"image", "depth", "pos", "normal"}
    for k in res0:
        assert torch.equal(res[k], res0[k]), k
    for k, g0 in grads0.items():
        if k in CAMERA:
            assert g0 is None
        elif k in WRITTEN:
            assert (g0 is None and grads[k] is None) or torch.equal(grads[k], g0), k
        else:
            w = g0.cpu().numpy().astype(np.float64)
            np.testing.assert_allclose(grads[k].cpu().numpy(), w, rtol=0, atol=2e-4 * np.abs(w).max() + 1e-6, err_msg=k)


@pytest.mark.parametrize("name", ["ar_36x48", "ar_12x16_s2", "ar_17x9_b3_quartic", "ndc_36x48", "ndc_17x9_b3"])
def test_camera_gradients_are_identical_from_run_to_run(name):
    kind, scene, kw, g_image, *_ = _load(name)
    _, again = _run(kind, scene, kw, g_image)
    for k in CAMERA:
        assert torch.equal(_full(name)[1][k], again[k]), k


@pytest.mark.parametrize("name", ["ar_17x9_b3_quartic", "ndc_17x9_b3"])
def test_a_view_alone_gets_its_bits_and_a_shared_leaf_the_fp64_sum(name):
    """float64 leaves, so that nothing is rounded on the way back: row b of the per-view eye's gradient is the
    single-view call's, bit for bit, and the shared at / up get the sum of the per-view results."""
    kind, scene, kw, g_image, *_ = _load(name)
    _, batch = _run(kind, scene, kw, g_image, only_image=True, camera_dtype=torch.float64)
    B = oracle.n_views(kind, scene)
    assert B == 3 and batch["camera.eye"].shape == (B, 4) and batch["camera.eye"].dtype == torch.float64
    alone = [_run(kind, oracle.view(kind, scene, b), kw, g_image[b], only_image=True, camera_dtype=torch.float64)[1]
             for b in range(B)]
    for b in range(B):
        assert torch.equal(batch["camera.eye"][b], alone[b]["camera.eye"]), b
    for k in ("camera.at", "camera.up"):
        total = sum(a[k].cpu().numpy() for a in alone)
        np.testing.assert_allclose(batch[k].cpu().numpy(), total, rtol=0, atol=1e-14 * np.abs(total).max(), err_msg=k)


@pytest.mark.parametrize("name", ["ar_3x5", "ar_12x16_s2", "ar_17x9_b3_quartic", "ndc_2x2", "ndc_17x9_b3"])
def test_camera_leaves_alone_still_get_their_gradient(name):
    """Nothing else requires grad: every other gradient output of the entry point is NULL (for estimated normals the
    stencil pass is not run at all)."""
    kind, scene, kw, g_image, *_ = _load(name)
    _, grads = _run(kind, scene, kw, g_image, others=False)
    for k, g in grads.items():
        if k in CAMERA:
            assert torch.equal(g, _full(name)[1][k]), k
        else:
            assert g is None, k


@pytest.mark.parametrize("name", ["ar_3x5", "ar_17x9_b3_quartic", "ndc_3x5_l1", "ndc_17x9_b3"])
def test_camera_leaves_keep_their_own_dtype_and_device(name):
    kind, scene, kw, g_image, want, _ = _load(name)
    _, grads = _run(kind, scene, kw, g_image, only_image=True, camera_dtype=torch.float64, camera_device="cpu")
    for k in CAMERA:
        g = grads[k]
        assert g.dtype == torch.float64 and g.device.type == "cpu", k
        assert tuple(g.shape) == np.shape(scene["camera"][k.split(".")[1]]), k
        np.testing.assert_allclose(g.numpy(), want["64"][k], rtol=2e-6, atol=2e-7 * np.abs(want["64"][k]).max(), err_msg=k)


@pytest.mark.parametrize("name", ["ar_3x5", "ar_12x16_s2", "ndc_3x5_l1", "ndc_17x9_b3"])
def test_only_the_image_carries_the_camera(name):
    """A loss on depth, pos and normal alone: a shaded frame gives the camera leaves exact zeros."""
    kind, scene, kw, g_image, *_ = _load(name)
    _, grads = _run(kind, scene, kw, g_image, outputs=("depth", "pos", "normal"))
    for k in CAMERA:
        assert grads[k] is not None and torch.count_nonzero(grads[k]) == 0, k
    assert torch.count_nonzero(grads["disk.pos"]) > 0


@pytest.mark.parametrize("name", ["ar_3x5", "ndc_3x5_l1"])
def test_a_frame_without_lights_leaves_the_camera_without_a_gradient(name):
    """norm_depth_image_only=True: no lights, nothing launched for the camera, .grad stays None as under the reference's
    autograd."""
    kind, scene, kw, g_image, *_ = _load(name)
    sc, leaves = _gpu_scene(scene)
    res = _entry(kind, False)(sc, norm_depth_image_only=True, camera_grad=True, **kw)
    (res["image"].sum() + res["depth"].sum()).backward()
    torch.cuda.synchronize()
    for k in CAMERA:
        assert leaves[k].grad is None, k
    assert leaves["disk.pos"].grad is not None
