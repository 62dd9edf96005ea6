"""GPU: render_splats_NDC / render_splats_NDC_batch (srh_splat_ndc_fwd / srh_splat_ndc_bwd) against the fp64 restatement
tests/splats_ndc_oracle.py, which tests/test_splats_ndc_oracle_cpu.py ties to the reference
(tests/golden/splats_ndc/sn1_*.npz).

Stated tolerances, the project's for kernels that compute the restatement's arithmetic in fp64 and store fp32: outputs
and the gradients the kernel writes (pos, normal) rtol 2e-6, atol 2e-7 max(max|want|, 1); the scene parameters, which
leave as fp32 atomic sums, |got - want| <= 2e-4 max|want| + 1e-6.  No element is excluded: the cases keep every decision
quantity 1e-6 away from its kink.  Against the float32 reference: outputs atol 2e-5 max(max|want|, 1), gradients atol
3e-3 max(max|want|, 1e-6), the figures of tests/test_hip_splats.py."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import splats_ndc_cases as cases
import splats_ndc_oracle as oracle
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIR = os.path.join(GOLDEN_DIR, "splats_ndc")
_GPU_LEAVES = {"disk.pos": ("objects", "disk", "pos"), "disk.normal": ("objects", "disk", "normal"),
               "lights.pos": ("lights", "pos"), "lights.attenuation": ("lights", "attenuation"),
               "lights.ambient": ("lights", "ambient"), "colors": ("colors",), "materials.albedo": ("materials", "albedo"),
               "materials.coeffs": ("materials", "coeffs")}


def _load(name):
    npz = np.load(os.path.join(DIR, f"sn1_{name}.npz"), allow_pickle=False)
    return npz, oracle.unpack(npz), oracle.kwargs_of(npz)


def _gpu_scene(scene, grad=tuple(_GPU_LEAVES), dtype=torch.float32):
    """The scene with GPU leaves (requires_grad for those named in `grad`); returns (scene, leaves)."""
    sc = copy.deepcopy(scene)
    leaves = {}
    for name, path in _GPU_LEAVES.items():
        d = sc
        for p in path[:-1]:
            d = d[p]
        t = torch.tensor(np.asarray(d[path[-1]], dtype=np.float32), device=DEV).to(dtype).requires_grad_(name in grad)
        d[path[-1]] = leaves[name] = t
    sc["lights"]["color_idx"] = torch.as_tensor(np.asarray(sc["lights"]["color_idx"]), device=DEV)
    sc["objects"]["disk"]["material_idx"] = torch.as_tensor(np.asarray(sc["objects"]["disk"]["material_idx"]), device=DEV)
    return sc, leaves


def _render(scene, **kw):
    from surf_renderer_amd import render_splats_NDC, render_splats_NDC_batch
    return (render_splats_NDC_batch if oracle.n_views(scene) else render_splats_NDC)(scene, **kw)


def _hip(scene, up, **kw):
    sc, leaves = _gpu_scene(scene)
    res = _render(sc, **kw)
    loss = sum(torch.sum(res[k] * torch.as_tensor(up[k], dtype=torch.float32, device=DEV)) for k in up)
    loss.backward()
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in res.items()}
    grads = {k: t.grad.cpu().numpy().astype(np.float64) if t.grad is not None else np.zeros(tuple(t.shape))
             for k, t in leaves.items()}
    return out, grads


def _close(got, want, tag):
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-7 * max(np.abs(want).max(), 1.0), err_msg=tag)


def _atomic_close(got, want, tag):
    assert np.all(np.isfinite(want)), tag
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-4 * np.abs(want).max() + 1e-6, err_msg=tag)


def test_the_public_names_render_one_splat():
    import surf_renderer_amd
    npz, scene, kw = _load("1x1")
    sc, _ = _gpu_scene(scene, grad=())
    res = surf_renderer_amd.render_splats_NDC(sc, **kw)
    assert {k: tuple(v.shape) for k, v in res.items()} == {"image": (1, 1, 3), "depth": (1, 1), "pos": (1, 1, 3),
                                                           "normal": (1, 1, 3)}
    res = surf_renderer_amd.render_splats_NDC_batch(_gpu_scene(_load("17x9_b3")[1], grad=())[0])
    assert {k: tuple(v.shape) for k, v in res.items()} == {"image": (3, 9, 17, 3), "depth": (3, 9, 17),
                                                           "pos": (3, 9, 17, 3), "normal": (3, 9, 17, 3)}


@pytest.mark.parametrize("name", cases.NAMES)
def test_forward_and_gradients_match_the_restatement_and_the_reference(name):
    npz, scene, kw = _load(name)
    up = {k: npz["grad_in/" + k] for k in oracle.OUTPUTS}
    got, got_g = _hip(scene, up, **kw)
    want, want_g = oracle.batch_gradients(scene, up, **kw)
    for k in oracle.OUTPUTS:
        _close(got[k], want[k], f"{name} {k}")
    for k in oracle.LEAVES:
        (_close if k in oracle.WRITTEN else _atomic_close)(got_g[k], want_g[k], f"{name} d/d {k}")
    for k in oracle.OUTPUTS:                               # the float32 reference itself
        w = npz["ref32/" + k].astype(np.float64)
        np.testing.assert_allclose(got[k], w, rtol=0, atol=2e-5 * max(np.abs(w).max(), 1.0), err_msg=f"{name} ref32 {k}")
    for k in oracle.LEAVES:
        w = npz["grad32/" + k].astype(np.float64)
        np.testing.assert_allclose(got_g[k], w, rtol=0, atol=3e-3 * max(np.abs(w).max(), 1e-6),
                                   err_msg=f"{name} grad32 {k}")


@pytest.mark.parametrize("name", ["17x9_b3", "17x9_b3_shared"])
def test_a_batch_equals_the_loop_over_its_views(name):
    npz, scene, kw = _load(name)
    up = {k: npz["grad_in/" + k] for k in oracle.OUTPUTS}
    got, got_g = _hip(scene, up, **kw)
    B = oracle.n_views(scene)
    per_view = {"disk.pos": True, "disk.normal": np.ndim(scene["objects"]["disk"]["normal"]) == 3,
                "lights.pos": np.ndim(scene["lights"]["pos"]) == 3}
    loop = [_hip(oracle.view(scene, b), {k: g[b] for k, g in up.items()}, **kw) for b in range(B)]
    for k in oracle.OUTPUTS:
        np.testing.assert_array_equal(got[k], np.stack([r[0][k] for r in loop]), err_msg=f"{name} {k}")
    for k in oracle.LEAVES:
        if per_view.get(k) and k in oracle.WRITTEN:        # written by the lane that owns the splat: bit-identical
            np.testing.assert_array_equal(got_g[k], np.stack([r[1][k] for r in loop]), err_msg=f"{name} d/d {k}")
        elif per_view.get(k):
            _atomic_close(got_g[k], np.stack([r[1][k] for r in loop]), f"{name} d/d {k}")
        else:                                              # a shared leaf: the sum over the views
            _atomic_close(got_g[k], sum(r[1][k] for r in loop), f"{name} d/d {k}")


@pytest.mark.parametrize("name", ["16x17", "17x9_b3"])
def test_written_gradients_are_identical_from_run_to_run(name):
    npz, scene, kw = _load(name)
    up = {k: npz["grad_in/" + k] for k in oracle.OUTPUTS}
    a, b = _hip(scene, up, **kw)[1], _hip(scene, up, **kw)[1]
    for k in oracle.WRITTEN:
        assert np.abs(a[k]).max() > 0
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("pos_cols", [3, 4])
def test_every_output_and_written_gradient_element_is_overwritten(pos_cols):
    """Through the C ABI with torch buffers prefilled with NaN, at 16 x 17: two workgroups, the second with 16 lanes."""
    from surf_renderer_amd import _lib
    lib = _lib.load()
    npz, scene, kw = _load("16x17")
    W, H = oracle.grid(scene["camera"])
    N = W * H
    f = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)  # noqa: E731
    pos = scene["objects"]["disk"]["pos"]
    if pos_cols == 4:
        pos = np.concatenate((pos, np.ones((N, 1), np.float32)), axis=1)
    pos, normal, eye = f(pos), f(scene["objects"]["disk"]["normal"][:, :3]), f(scene["camera"]["eye"][:3])
    lpos, colors = f(scene["lights"]["pos"]), f(scene["colors"])
    att, amb = f(scene["lights"]["attenuation"]), f(scene["lights"]["ambient"])
    albedo, coeffs = f(scene["materials"]["albedo"]), f(scene["materials"]["coeffs"])
    cidx = torch.tensor(scene["lights"]["color_idx"], dtype=torch.int32, device=DEV)
    mat = torch.tensor(scene["objects"]["disk"]["material_idx"], dtype=torch.int32, device=DEV)
    cam = scene["camera"]
    p = _lib.SrhSplatNdcParams(n_views=1, width=W, height=H, pos_cols=pos_cols, shade=1, fovy=cam["fovy"],
                               near_clip=cam["near"], far_clip=cam["far"])
    p.at[:] = [float(v) for v in cam["at"][:3]]
    p.up[:] = [float(v) for v in cam["up"][:3]]
    inp = _lib.SrhSplatNdcInputs(pos=pos.data_ptr(), pos_view_stride=N * pos_cols, normal=normal.data_ptr(),
                                 normal_view_stride=N * 3, eye=eye.data_ptr(), material_idx=mat.data_ptr())
    li = _lib.SrhLights(n_lights=lpos.shape[0], n_colors=colors.shape[0], pos=lpos.data_ptr(), color_idx=cidx.data_ptr(),
                        colors=colors.data_ptr(), attenuation=att.data_ptr(), ambient=amb.data_ptr())
    ma = _lib.SrhMaterials(n_materials=albedo.shape[0], albedo=albedo.data_ptr(), coeffs=coeffs.data_ptr())
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    image, depth, pos_out = nan(H, W, 3), nan(H, W), nan(H, W, 3)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.srh_splat_ndc_fwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), image.data_ptr(),
                                     depth.data_ptr(), pos_out.data_ptr(), stream))
    g_pos, g_normal = nan(N, pos_cols), nan(N, 3)
    ups = [f(npz["grad_in/" + k]) for k in ("image", "depth", "pos")]
    grads = _lib.SrhSplatNdcGrads(pos=g_pos.data_ptr(), normal=g_normal.data_ptr())
    _lib.check(lib.srh_splat_ndc_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), *[u.data_ptr() for u in ups],
                                     C.byref(grads), stream))
    torch.cuda.synchronize()
    for name, t in (("image", image), ("depth", depth), ("pos", pos_out), ("g_pos", g_pos), ("g_normal", g_normal)):
        assert bool(torch.isfinite(t).all()), name
    up = {k: npz["grad_in/" + k] for k in ("image", "depth", "pos")}
    want, want_g = oracle.gradients(scene, up, **kw)
    _close(image.cpu().numpy().astype(np.float64), want["image"], "image")
    _close(g_pos[:, :3].cpu().numpy().astype(np.float64), want_g["disk.pos"], "g_pos")
    _close(g_normal.cpu().numpy().astype(np.float64), want_g["disk.normal"], "g_normal")


def test_a_depth_loss_on_pos_alone_leaves_the_other_leaves_without_gradient():
    npz, scene, kw = _load("3x5")
    sc, leaves = _gpu_scene(scene, grad=("disk.pos",))
    res = _render(sc, **kw)
    assert res["depth"].requires_grad and not res["normal"].requires_grad
    torch.sum(res["depth"] * torch.as_tensor(npz["grad_in/depth"], device=DEV)).backward()
    want = oracle.gradients(scene, {"depth": npz["grad_in/depth"]}, **kw)[1]
    _close(leaves["disk.pos"].grad.cpu().numpy().astype(np.float64), want["disk.pos"], "d depth / d pos")
    assert all(t.grad is None for k, t in leaves.items() if k != "disk.pos")


def test_a_geometry_only_frame_gives_the_shading_leaves_no_gradient():
    npz, scene, kw = _load("3x5_norm_depth")
    sc, leaves = _gpu_scene(scene)
    res = _render(sc, **kw)
    sum(torch.sum(res[k] * torch.as_tensor(npz["grad_in/" + k], device=DEV)) for k in oracle.OUTPUTS).backward()
    assert leaves["disk.pos"].grad is not None and leaves["disk.normal"].grad is not None
    for k in oracle.LEAVES[2:]:
        assert leaves[k].grad is None, k


def test_no_grad_saves_nothing_and_gives_the_same_outputs():
    npz, scene, kw = _load("17x9")
    sc, _ = _gpu_scene(scene)
    with torch.no_grad():
        quiet = _render(sc, **kw)
    loud = _render(sc, **kw)
    for k in oracle.OUTPUTS:
        assert quiet[k].grad_fn is None and not quiet[k].requires_grad, k
        assert loud[k].requires_grad, k
        assert torch.equal(quiet[k], loud[k].detach()), k


@pytest.mark.parametrize("form", ["float64", "slice"])
def test_gradients_come_back_in_the_leaf_s_own_dtype_and_layout(form):
    npz, scene, kw = _load("3x5")
    up = {k: npz["grad_in/" + k] for k in oracle.OUTPUTS}
    _, want = _hip(scene, up, **kw)
    sc, leaves = _gpu_scene(scene, dtype=torch.float64 if form == "float64" else torch.float32)
    if form == "slice":                                    # every other row / column of a wider leaf
        for name, path in (("disk.pos", ("objects", "disk", "pos")), ("disk.normal", ("objects", "disk", "normal"))):
            wide = torch.zeros((30, 6), device=DEV)
            wide[::2, ::2] = leaves[name].detach()
            leaves[name] = wide.requires_grad_(True)
            sc["objects"]["disk"][path[-1]] = leaves[name][::2, ::2]
            assert not sc["objects"]["disk"][path[-1]].is_contiguous()
    res = _render(sc, **kw)
    assert all(v.dtype == torch.float32 for k, v in res.items() if k != "normal")
    sum(torch.sum(res[k] * torch.as_tensor(up[k], device=DEV)) for k in oracle.OUTPUTS).backward()
    for k, t in leaves.items():
        assert t.grad is not None and t.grad.dtype == t.dtype and t.grad.shape == t.shape, k
        g = t.grad[::2, ::2] if (form == "slice" and k in oracle.WRITTEN) else t.grad
        w = want[k]
        if k in oracle.WRITTEN:
            np.testing.assert_array_equal(g.cpu().numpy().astype(np.float64), w, err_msg=k)
        else:
            _atomic_close(g.cpu().numpy().astype(np.float64), w, k)
