"""GPU: render_views under autograd -- the batched analytic HIP backward (srh_render_views_bwd: one backward launch per
chunk of views, the view a grid dimension) against the per-view gradient oracles, shared leaves summed over the views and
per-view leaves kept per view (the definition pinned to the reference by tests/test_views_grad_golden_cpu.py).

Tolerances are the project's: against the fp64 oracle  |got - want| <= 2e-4 * max|want| + 1e-6  per array
(tests/test_hip_backward.py), against the float32 reference fixtures 2e-3 * max|want|.  Frames are 72 x 22: a partial
64-lane workgroup in x, a partial 4-row workgroup in y, partial 16 x 16 tiles."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from grad_cases import (DEV, NP_KEYS, TCH_KEYS, assert_array_close, assert_grads_close, gpu_leaf_scene, gpu_tensor,
                        leaf_grads, masked_loss, to_np, view_winners)
from oracle import np_oracle_tch, torch_oracle
from oracle.golden_io import load_case
from views_cases import (AWAY3, KW3, OWN3, V1_CASES, V1_PER_VIEW, H, W, batch_gradients, batch_upstream, load_v1, ortho_case,
                         oracle_batch_tch, scene3, shadow_case, view_cameras, view_scene, visibility_rows)

pytestmark = pytest.mark.gpu


def _upstream(n, seed, **size):
    return batch_upstream(n, seed, outputs=("image", "depth"), **size)


def _backward(out, g, far=None):
    masked_loss(out, g, far).backward()
    torch.cuda.synchronize()


# ---- 1. the reference's own batch loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V1_CASES)
def test_reference_batch_fixture(case):
    from surf_renderer_amd import render_views
    npz, scene, cams, own, kw = load_v1(case)
    n = len(cams)
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS, skip=V1_PER_VIEW)
    per_view = [{k: gpu_tensor(own[v][k]) for k in V1_PER_VIEW} for v in range(n)]
    cameras = [dict(scene["camera"], **cams[v]) for v in range(n)]
    out = render_views(leaf_scene, cameras, device=DEV, shading="torch", overrides=per_view, batch=3, **kw)
    assert out["image"].requires_grad and out["depth"].requires_grad and not out["nearest"].requires_grad
    far = float(scene["camera"]["far"])
    got_dep, want_dep = to_np(out["depth"]), npz["ref/depth"].astype(np.float64)
    assert np.array_equal(out["nearest"].cpu().numpy(), npz["ref/nearest"])
    hit = want_dep <= far
    assert np.array_equal(got_dep <= far, hit)
    np.testing.assert_allclose(got_dep[hit], want_dep[hit], rtol=2e-5)
    np.testing.assert_allclose(got_dep[~hit], far + 1.0)
    np.testing.assert_allclose(to_np(out["image"]), npz["ref/image"], atol=3e-4)
    _backward(out, {"image": npz["grad_in/image"], "depth": npz["grad_in/depth"]}, far)
    checked = 0
    for key in npz.files:
        if not key.startswith("grad/"):
            continue
        parts = key[5:].split("/")
        want = npz[key].astype(np.float64)
        t = leaves[parts[0]] if len(parts) == 1 else per_view[int(parts[1])][parts[0]]
        assert t.grad is not None, key
        got = to_np(t.grad).reshape(want.shape)
        if parts[0] in ("lights.pos", "plane.pos", "disk.pos"):
            got, want = got[..., :3], want[..., :3]
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-3 * max(np.abs(want).max(), 1e-6), err_msg=key)
        checked += 1
    assert checked == 11 + 2 * n
    for k in V1_PER_VIEW:                                    # the look-away view: zeros, not None
        g = per_view[n - 1][k].grad
        assert g is not None and g.shape == per_view[n - 1][k].shape and not g.any()
    assert not leaves["disk.radius"].grad.any()


# ---- 2. numpy shading, mixed primitives -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["g1_demo_64x48", "g8a_sphere_behind_camera"])
def test_numpy_shading_shared_leaves(case):
    from surf_renderer_amd import render_views
    scene, _, _ = load_case(os.path.join(GOLDEN_DIR, case + ".npz"))
    eye = np.asarray(scene["camera"]["eye"], dtype=np.float64)
    step = 0.05 if case.startswith("g8a") else 0.4
    cameras = view_cameras(scene["camera"], [eye, eye + step * np.array([1.0, 0.5, 0.0, 0.0]),
                                         eye + step * np.array([-0.8, 0.4, 1.0, 0.0])])
    n = len(cameras)
    leaf_scene, leaves = gpu_leaf_scene(scene, NP_KEYS)
    out = render_views(leaf_scene, cameras, device=DEV)
    assert out["image"].requires_grad
    g = _upstream(n, 3)
    _backward(out, g)
    refs = view_winners(out)
    assert all(np.isfinite(r["depth"]).any() for r in refs)
    per_view = [torch_oracle.gradients(view_scene(scene, cameras[v]), g["image"][v].astype(np.float64),
                                       g["depth"][v].astype(np.float64), ref=refs[v]) for v in range(n)]
    want, _ = batch_gradients(per_view, ())
    assert set(want) == set(leaves)
    assert_grads_close(leaf_grads(leaves), want, 2e-4, case)
    assert any(np.abs(w).max() > 0 for w in want.values())
    if "disk.radius" in leaves:
        assert not leaves["disk.radius"].grad.any()
    if "triangle.face" in leaves:
        assert not leaves["triangle.face"].grad[:, 1:, :].any()


# ---- 3. torch shading, everything at once -------------------------------------------------------------------------------
def _run3(scene, cameras, own, grad_own=OWN3, grad_shared=True, batch=2):
    """The batch of case 3; returns (out, shared leaves that require grad, stacked per-view parents)."""
    from surf_renderer_amd import render_views
    n = len(cameras)
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS, skip=OWN3, grad=grad_shared)
    parents = {k: gpu_tensor(own[k], k in grad_own) for k in OWN3}
    overrides = [{k: parents[k][v] for k in OWN3} for v in range(n)]          # slices: not leaves
    out = render_views(leaf_scene, cameras, device=DEV, shading="torch", overrides=overrides, batch=batch, **KW3)
    return out, leaves, parents


@pytest.fixture(scope="module")
def case3():
    scene, cameras, own = scene3()
    n = len(cameras)
    g = _upstream(n, 5)
    out, leaves, parents = _run3(scene, cameras, own)
    far = float(scene["camera"]["far"])
    _backward(out, g, far)
    refs = view_winners(out)
    scenes = [view_scene(scene, cameras[v], {k: own[k][v] for k in OWN3}) for v in range(n)]
    shared, per_view = oracle_batch_tch(scenes, g, refs, OWN3, **KW3)
    got = {k: to_np(t.grad) for k, t in {**leaves, **parents}.items()}
    fwd = {k: out[k].detach().clone() for k in ("image", "depth", "nearest")}
    return dict(scene=scene, cameras=cameras, own=own, g=g, far=far, refs=refs, shared=shared,
                per_view=per_view, got=got, fwd=fwd, leaves=leaves)


def test_torch_shading_everything_at_once(case3):
    c = case3
    n = len(c["cameras"])
    hits = [(r["depth"] <= c["far"]).mean() for r in c["refs"]]
    assert hits[AWAY3] == 0 and all(h > 0.5 for v, h in enumerate(hits) if v != AWAY3)
    for v, ref in enumerate(c["refs"]):                     # the winners are the fp64 oracle's
        sc = view_scene(c["scene"], c["cameras"][v], {k: c["own"][k][v] for k in OWN3})
        assert np.array_equal(ref["nearest"], np_oracle_tch.render(sc, **KW3)["nearest"]), f"view {v}"
    assert len(c["shared"]) == 12 and set(c["shared"]) == set(c["leaves"])
    assert_grads_close(c["got"], c["shared"], 2e-4, "shared")
    for key in OWN3:
        assert c["got"][key].shape[0] == n
        for v in range(n):
            assert_array_close(c["got"][key][v], c["per_view"][key][v], 2e-4, f"{key}[{v}]")
        assert not c["got"][key][AWAY3].any() and all(c["got"][key][v].any() for v in range(n) if v != AWAY3)
    assert not c["got"]["disk.radius"].any()
    assert not c["got"]["triangle.face"][:, 1:, :].any()


# ---- 4. shadow rays ---------------------------------------------------------------------------------------------------
def test_shadow_rays_with_per_view_lights():
    from surf_renderer_amd import render_views
    scene, kw, cameras, lights = shadow_case()
    n = len(cameras)
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS, skip=("lights.pos",))
    parent = gpu_tensor(lights)
    out = render_views(leaf_scene, cameras, device=DEV, shading="torch", shadow=True,
                       overrides=[{"lights.pos": parent[v]} for v in range(n)], **kw)
    assert out["image"].requires_grad and not out["visibility"].requires_grad
    g = _upstream(n, 9)
    far = float(scene["camera"]["far"])
    _backward(out, g, far)
    vis = visibility_rows(out["visibility"].cpu().numpy(), lights.shape[1])
    hit = to_np(out["depth"]) <= far
    shadowed = 1.0 - np.mean([vis[v][:, hit[v].reshape(-1)].mean() for v in range(n)])
    assert 0.01 < shadowed < 0.99                           # the scene does cast shadows
    scenes = [view_scene(scene, cameras[v], {"lights.pos": lights[v]}) for v in range(n)]
    shared, per_view = oracle_batch_tch(scenes, g, view_winners(out), ("lights.pos",), visibility=vis, **kw)
    assert_grads_close(leaf_grads(leaves), shared, 2e-4, "shadow")
    for v in range(n):
        assert_array_close(to_np(parent.grad)[v], per_view["lights.pos"][v], 2e-4, f"shadow lights.pos[{v}]")
    plain, _ = oracle_batch_tch(scenes, g, view_winners(out), ("lights.pos",), **kw)
    assert np.abs(plain["materials.albedo"] - shared["materials.albedo"]).max() > 1e-3 * np.abs(shared["materials.albedo"]).max()


# ---- 5. orthographic views ----------------------------------------------------------------------------------------------
def test_orthographic_views():
    from surf_renderer_amd import render_views
    scene, cameras = ortho_case()
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
    out = render_views(leaf_scene, cameras, device=DEV, shading="torch")
    g = _upstream(2, 13)
    far = float(scene["camera"]["far"])
    _backward(out, g, far)
    refs = view_winners(out)
    assert all((r["depth"] <= far).mean() > 0.3 for r in refs)
    scenes = [view_scene(scene, cam) for cam in cameras]
    want, _ = oracle_batch_tch(scenes, g, refs, ())
    assert set(want) == set(leaves)
    assert_grads_close(leaf_grads(leaves), want, 2e-4, "ortho")


# ---- 6. large runs: the workgroup-merge path of scatter_primitive_grads -----------------------------------------------------
def test_plane_filling_every_workgroup():
    """The plane scene of tests/test_hip_backward.py at 128 x 8.  The frame is 16 : 1, so fovy is 6 degrees: that keeps
    the horizontal field of view near 80 degrees, inside which every ray of both views meets the plane (at that test's 50
    degrees the second view's outer columns run parallel to the plane and miss it)."""
    from surf_renderer_amd import render_views
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)          # noqa: E731
    scene = {"camera": {"viewport": [0, 0, 128, 8], "fovy": float(np.deg2rad(6.0)), "focal_length": 1.0,
                        "eye": [0.3, 2.0, 6.0, 1.0], "at": [0.0, 0.0, 0.0, 1.0], "up": [0.0, 1.0, 0.0, 0.0],
                        "near": 0.1, "far": 1000.0},
             "lights": {"pos": f32([[3, 6, 5, 1], [-4, 5, 3, 1], [0, 8, -2, 1]]), "color_idx": np.array([1, 2, 3])},
             "colors": f32([[0, 0, 0], [.8, .5, .4], [.3, .6, .9], [.5, .9, .3]]),
             "materials": {"albedo": f32([[.7, .6, .5]])},
             "objects": {"plane": {"pos": f32([[0, 0, -30, 1]]), "normal": f32([[0.05, 0.3, 1.0, 0]]),
                                   "material_idx": np.array([0])}},
             "tonemap": {"type": "gamma", "gamma": 0.8}}
    cameras = [dict(scene["camera"], eye=np.array(e, dtype=np.float64)) for e in ([0.3, 2.0, 6.0, 1.0], [-1.0, 1.0, 7.0, 1.0])]
    leaf_scene, leaves = gpu_leaf_scene(scene, NP_KEYS)
    out = render_views(leaf_scene, cameras, device=DEV)
    assert torch.isfinite(out["depth"]).all() and not out["nearest"].any()      # the plane wins every pixel
    g = _upstream(2, 19, h=8, w=128)
    _backward(out, g)
    refs = view_winners(out)
    per_view = [torch_oracle.gradients(view_scene(scene, cameras[v]), g["image"][v].astype(np.float64),
                                       g["depth"][v].astype(np.float64), ref=refs[v]) for v in range(2)]
    want, _ = batch_gradients(per_view, ())
    assert_grads_close(leaf_grads(leaves), want, 2e-4, "plane")
    assert np.abs(want["plane.pos"]).max() > 0 and np.abs(want["plane.normal"]).max() > 0


# ---- 7. partial needs and the plain path -------------------------------------------------------------------------------
def test_only_one_override_requires_grad(case3):
    c = case3
    out, leaves, parents = _run3(c["scene"], c["cameras"], c["own"], grad_own=("lights.pos",), grad_shared=False)
    assert not leaves and out["image"].requires_grad
    assert torch.equal(out["image"], c["fwd"]["image"]) and torch.equal(out["nearest"], c["fwd"]["nearest"])
    _backward(out, c["g"], c["far"])
    assert parents["disk.pos"].grad is None and parents["disk.normal"].grad is None
    got = to_np(parents["lights.pos"].grad)
    for v in range(got.shape[0]):
        assert_array_close(got[v], c["per_view"]["lights.pos"][v], 2e-4, f"lights.pos[{v}] alone")
    # ... and the value of the full case, to the run-to-run spread of the atomic sums
    full = c["got"]["lights.pos"]
    assert np.abs(got - full).max() <= 2e-5 * np.abs(full).max()


def test_plain_path_without_autograd(case3):
    c = case3
    out, leaves, parents = _run3(c["scene"], c["cameras"], c["own"], grad_own=(), grad_shared=False)
    assert not leaves and not any(p.requires_grad for p in parents.values())
    with torch.no_grad():
        quiet, _, _ = _run3(c["scene"], c["cameras"], c["own"])          # leaves require grad, autograd is off
    for res in (out, quiet):
        assert res["image"].grad_fn is None and res["depth"].grad_fn is None
        assert not res["image"].requires_grad and not res["depth"].requires_grad
        for k in ("image", "depth", "nearest"):
            assert torch.equal(res[k], c["fwd"][k]), k


# ---- 8. workspace hygiene ----------------------------------------------------------------------------------------------
def test_second_call_gives_the_same_frames_and_gradients(case3):
    c = case3
    out, leaves, parents = _run3(c["scene"], c["cameras"], c["own"])
    for k in ("image", "depth", "nearest"):
        assert torch.equal(out[k].detach(), c["fwd"][k]), k
    _backward(out, c["g"], c["far"])
    again = {k: to_np(t.grad) for k, t in {**leaves, **parents}.items()}
    assert set(again) == set(c["got"])
    for key, a in again.items():
        b = c["got"][key]
        spread = np.abs(a - b).max()
        print(f"{key}: run-to-run spread {spread:.3g} of max {np.abs(b).max():.4g}")
        assert spread <= 2e-5 * max(np.abs(b).max(), 1e-30), f"{key}: run-to-run spread {spread}"


def test_backward_leaves_the_bin_counters_alone(case3):
    from surf_renderer_amd import _lib
    from surf_renderer_amd import renderer as R
    c = case3
    n = 3
    scene = view_scene(c["scene"])
    buf = R.flatten_scene(scene, DEV)
    cams = [R.camera_struct(cam, "torch") for cam in c["cameras"][:n]]
    kw = dict(shading="torch", **KW3)

    def frames():
        return (torch.empty((n, H, W, 3), dtype=torch.float32, device=DEV), torch.empty((n, H, W), dtype=torch.float32, device=DEV),
                torch.empty((n, H, W), dtype=torch.int32, device=DEV))

    img_a, dep_a, near_a = frames()
    ws = R.render_views_buffers(buf, cams, img_a, dep_a, near_a, **kw)
    state = R._ws_state(ws)
    assert state is not None and state[0] == "clean"
    g_alb = torch.zeros_like(buf.tensors["materials.albedo"])
    g_pos = torch.zeros_like(buf.tensors["disk.pos"])
    grads = (_lib.SrhGrads * n)()
    for v in range(n):
        grads[v].albedo = g_alb.data_ptr()
        grads[v].pos[buf.kinds.index("disk")] = g_pos.data_ptr()
    g_img = torch.as_tensor(c["g"]["image"][:n], device=DEV).contiguous()
    assert R.render_views_bwd_buffers(buf, cams, g_img, None, near_a, dep_a, grads, workspace=ws, **kw) is ws
    assert R._ws_state(ws) == state                          # still noted clean: the next forward clears nothing
    img_b, dep_b, near_b = frames()
    assert R.render_views_buffers(buf, cams, img_b, dep_b, near_b, workspace=ws, **kw) is ws
    torch.cuda.synchronize()
    assert torch.equal(img_a, img_b) and torch.equal(dep_a, dep_b) and torch.equal(near_a, near_b)
    assert g_alb.any() and g_pos.any()
