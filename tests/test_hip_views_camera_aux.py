"""GPU: render_views with the torch backend's normal / pos outputs (srh_render_views_aux) and, under autograd, with camera
leaves and upstream gradients of all four outputs (srh_render_views_bwd_camera: the kAux / kCam instantiations of
k_render_bwd_tch_views, then k_camera_finish_views -- one backward launch and one finish launch per chunk of views),
against render() per view and against the fp64 oracle with the camera in its graph (oracle/torch_oracle.gradients_tch,
camera=True) fed the GPU frames' winners.

Tolerances are the project's own (tests/test_hip_camera_grad.py): per array |got - want| <= 2e-4 * max|want| + 1e-6
against the helper, 2e-5 of the largest entry between two runs of the fp32-atomic scene gradients; the camera gradients
of a batch against render() per view 1e-6 * max|want| (float32 roundings of fp64 sums formed in the same fixed order).
Frames are 72 x 22: a partial 64-lane workgroup in x, a partial 4-row workgroup in y, partial 16 x 16 tiles."""
import copy

import numpy as np
import pytest
import torch

from grad_cases import (CAM, DEV, RUN_TO_RUN, TCH_KEYS, assert_array_close, assert_grads_close, gpu_leaf_scene,
                        gpu_tensor, leaf_grads, masked_loss, to_np, view_winners)
from oracle.torch_oracle import CAMERA_KEYS as CAM_KEYS, OUTPUTS
from views_cases import (AWAY3, EYES3, KW3, OWN3, H, W, batch_upstream, oracle_batch_tch, ortho_case, scene3, shadow_case, view_scene,
                         visibility_rows)

pytestmark = pytest.mark.gpu

def _cam_tensors(cameras, which=None):
    """Per view: float32 GPU tensors of eye / at / up; those named by which(v) (default all three) require grad."""
    out = []
    for v, cam in enumerate(cameras):
        names = CAM if which is None else which(v)
        out.append({k: torch.tensor(np.asarray(cam[k], dtype=np.float64), dtype=torch.float32, device=DEV,
                                    requires_grad=k in names) for k in CAM})
    return out


def _run(scene, cameras, own, cam=None, grad_own=OWN3, grad_shared=True, batch=2, aux=True, kw=KW3, cam_tensors=None, **more):
    """The batch of case 2: per-view overrides as slices of stacked parents, cameras with tensor eye / at / up.  Returns
    (out, shared leaves that require grad, stacked per-view parents, per-view camera tensors)."""
    from surf_renderer_amd import render_views
    n = len(cameras)
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS, skip=tuple(own), grad=grad_shared)
    parents = {k: gpu_tensor(own[k], k in grad_own) for k in own}
    overrides = [{k: parents[k][v] for k in own} for v in range(n)] if own else None
    cams = cam_tensors if cam_tensors is not None else _cam_tensors(cameras, cam)
    out = render_views(leaf_scene, [dict(cameras[v], **cams[v]) for v in range(n)], device=DEV, shading="torch",
                       overrides=overrides, batch=batch, aux=aux, **kw, **more)
    return out, leaves, parents, cams


def _helper(scenes, g, refs, own_keys, **kw):
    """The camera oracle per view -> (shared: summed over the views, own: {key: [per view]}; the camera keys are own)."""
    return oracle_batch_tch(scenes, g, refs, own_keys, camera=True, **kw)


def _cam_grads(cams):
    """{camera key: [per view (4,) float64]}; every tensor that requires grad must have got one, in its own shape."""
    out = {}
    for k in CAM:
        rows = []
        for v, c in enumerate(cams):
            t = c[k]
            if t.requires_grad:
                assert t.grad is not None, f"view {v}: camera.{k} got no gradient"
                assert t.grad.shape == t.shape and t.grad.dtype == t.dtype and t.grad.device == t.device
                rows.append(t.grad.detach().cpu().numpy().astype(np.float64))
            else:
                rows.append(None)
        out["camera." + k] = rows
    return out


def _check_wanted(per_view, away=None):
    """Every wanted array is finite and, outside the look-away view, not all zero."""
    for key, rows in per_view.items():
        for v, w in enumerate(rows):
            assert np.all(np.isfinite(w)), (key, v)
            if v != away:
                assert np.abs(w).max() > 0, (key, v)


def _compare_cameras(got, want, tag, away=None):
    for key in CAM_KEYS:
        for v, w in enumerate(want[key]):
            if got[key][v] is None:
                continue
            assert_array_close(got[key][v], w, 2e-4, f"{tag} {key}[{v}]")
            assert got[key][v][3] == 0.0
            if v == away:
                assert not got[key][v].any(), f"{tag} {key}[{v}]: the look-away view's gradient is not zero"


def _hits(refs, far):
    return [float((r["depth"] <= far).mean()) for r in refs]


# ---- the five-view batch of tests/test_hip_views_backward.py case 3, once per module -----------------------------------------
@pytest.fixture(scope="module")
def base():
    scene, cameras, own = scene3()
    return dict(scene=scene, cameras=cameras, own=own, n=len(cameras), far=float(scene["camera"]["far"]),
                g=batch_upstream(len(cameras), 5),
                scenes=[view_scene(scene, cameras[v], {k: own[k][v] for k in OWN3}) for v in range(len(cameras))])


def _everything(b):
    out, leaves, parents, cams = _run(b["scene"], b["cameras"], b["own"])
    masked_loss(out, b["g"], b["far"]).backward()
    torch.cuda.synchronize()
    got = {k: to_np(t.grad) for k, t in {**leaves, **parents}.items()}
    return out, got, _cam_grads(cams), cams


@pytest.fixture(scope="module")
def case2(base):
    out, got, got_cam, cams = _everything(base)
    refs = view_winners(out)
    shared, per_view = _helper(base["scenes"], base["g"], refs, OWN3, **KW3)
    fwd = {k: out[k].detach().clone() for k in ("image", "depth", "nearest", "normal", "pos")}
    return dict(base, out=out, got=got, got_cam=got_cam, refs=refs, shared=shared, per_view=per_view, fwd=fwd)


# ---- 1. forward aux ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 0])
def test_forward_aux_equals_render_per_view(base, batch):
    from surf_renderer_amd import render, render_views
    b = base
    overrides = [{k: b["own"][k][v] for k in OWN3} for v in range(b["n"])]
    with torch.no_grad():
        plain = render_views(b["scene"], b["cameras"], device=DEV, shading="torch", overrides=overrides, batch=batch, **KW3)
        out = render_views(b["scene"], b["cameras"], device=DEV, shading="torch", overrides=overrides, batch=batch,
                           aux=True, **KW3)
        assert set(plain) == {"image", "depth", "nearest"} and set(out) == set(plain) | {"normal", "pos"}
        for k in plain:
            assert torch.equal(out[k], plain[k]), k
        hits = _hits(view_winners(out), b["far"])
        assert hits[AWAY3] == 0 and all(h > 0.5 for v, h in enumerate(hits) if v != AWAY3)
        for k in ("normal", "pos"):
            assert out[k].shape == (b["n"], H, W, 3) and out[k].dtype == torch.float32
            assert not out[k][AWAY3].any(), k
        for v in range(b["n"]):
            one = render(b["scenes"][v], device=DEV, shading="torch", **KW3)
            for k in ("normal", "pos"):
                assert one[k].any() or v == AWAY3
                assert torch.equal(out[k][v], one[k]), f"view {v} {k}"
            assert torch.equal(out["image"][v], one["image"]) and torch.equal(out["depth"][v], one["depth"])


def test_forward_aux_orthographic_views():
    from surf_renderer_amd import render, render_views
    scene, cameras = ortho_case()
    with torch.no_grad():
        plain = render_views(scene, cameras, device=DEV, shading="torch")
        out = render_views(scene, cameras, device=DEV, shading="torch", aux=True)
        for k in plain:
            assert torch.equal(out[k], plain[k]), k
        for v, cam in enumerate(cameras):
            one = render(view_scene(scene, cam), device=DEV, shading="torch")
            assert float((one["depth"] <= scene["camera"]["far"]).float().mean()) > 0.3
            for k in ("normal", "pos"):
                assert one[k].any() and torch.equal(out[k][v], one[k]), f"view {v} {k}"


# ---- 2. camera gradients, everything at once ---------------------------------------------------------------------------------
def test_camera_gradients_everything_at_once(case2):
    c = case2
    n = c["n"]
    assert all(c["out"][k].requires_grad for k in OUTPUTS) and not c["out"]["nearest"].requires_grad
    hits = _hits(c["refs"], c["far"])
    assert hits[AWAY3] == 0 and all(h > 0.5 for v, h in enumerate(hits) if v != AWAY3)
    _check_wanted(c["per_view"], AWAY3)
    _compare_cameras(c["got_cam"], c["per_view"], "all", AWAY3)
    assert len(c["shared"]) == 12
    assert_grads_close(c["got"], c["shared"], 2e-4, "shared")
    assert any(np.abs(w).max() > 0 for w in c["shared"].values())
    for key in OWN3:
        assert c["got"][key].shape[0] == n
        for v in range(n):
            assert_array_close(c["got"][key][v], c["per_view"][key][v], 2e-4, f"{key}[{v}]")
        assert not c["got"][key][AWAY3].any()
    assert not c["got"]["disk.radius"].any()


# ---- 3. against render per view ------------------------------------------------------------------------------------------------
def test_batch_equals_render_per_view(case2):
    from surf_renderer_amd import render
    c = case2
    sums = {}
    for v in range(c["n"]):
        leaf_scene, leaves = gpu_leaf_scene(c["scenes"][v], TCH_KEYS)
        cam = _cam_tensors([c["cameras"][v]])[0]
        leaf_scene["camera"] = dict(leaf_scene["camera"], **cam)
        res = render(leaf_scene, device=DEV, shading="torch", **KW3)
        for k in ("normal", "pos"):
            assert torch.equal(res[k].detach(), c["fwd"][k][v]), (v, k)
        masked_loss(res, {k: a[v] for k, a in c["g"].items()}, c["far"]).backward()
        torch.cuda.synchronize()
        for k in CAM:
            want = cam[k].grad.cpu().numpy().astype(np.float64)
            got = c["got_cam"]["camera." + k][v]
            assert np.all(np.isfinite(want)) and (v == AWAY3 or np.abs(want).max() > 0)
            err = np.abs(got - want).max()
            print(f"view {v} camera.{k}: bit-equal {np.array_equal(got, want)}, max |delta| {err:.3g} of {np.abs(want).max():.4g}")
            assert err <= 1e-6 * np.abs(want).max(), (v, k)
        for key, t in leaves.items():
            g = to_np(t.grad)
            if key in OWN3:
                want, got = g, c["got"][key][v]
                assert np.abs(got.reshape(want.shape) - want).max() <= RUN_TO_RUN * max(np.abs(want).max(), 1e-30), (v, key)
            else:
                sums[key] = sums.get(key, 0.0) + g
    for key, want in sums.items():
        got = c["got"][key].reshape(want.shape)
        assert np.all(np.isfinite(want))
        spread = np.abs(got - want).max()
        print(f"{key}: batch against the per-view sum {spread:.3g} of max {np.abs(want).max():.4g}")
        assert spread <= RUN_TO_RUN * max(np.abs(want).max(), 1e-30), key


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------
def test_camera_gradients_are_identical_from_run_to_run(case2):
    c = case2
    _, got, got_cam, _ = _everything(c)
    for key in CAM_KEYS:
        for v in range(c["n"]):
            assert np.array_equal(got_cam[key][v], c["got_cam"][key][v]), (key, v)
    assert set(got) == set(c["got"])
    for key, a in got.items():
        b = c["got"][key]
        spread = np.abs(a - b).max()
        print(f"{key}: run-to-run spread {spread:.3g} of max {np.abs(b).max():.4g}")
        assert spread <= RUN_TO_RUN * max(np.abs(b).max(), 1e-30), key


# ---- 5. geometry-only kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [("normal", "pos"), ("depth",)])
def test_geometry_only_losses(case2, outputs):
    c = case2
    g = {k: c["g"][k] for k in outputs}
    out, leaves, parents, cams = _run(c["scene"], c["cameras"], c["own"])
    assert torch.equal(out["image"].detach(), c["fwd"]["image"])
    masked_loss(out, g, c["far"]).backward()
    torch.cuda.synchronize()
    shared, per_view = _helper(c["scenes"], g, c["refs"], OWN3, **KW3)
    _check_wanted({k: per_view[k] for k in CAM_KEYS + ("disk.pos", "disk.normal")}, AWAY3)
    _compare_cameras(_cam_grads(cams), per_view, "+".join(outputs), AWAY3)
    for key, want in shared.items():
        got = to_np(leaves[key].grad)
        if key in TCH_KEYS:                                # they require grad; the geometry-only kernel leaves them alone
            assert not got.any() and not want.any(), key
        else:
            assert_array_close(got, want, 2e-4, f"{'+'.join(outputs)} {key}")
    assert parents["lights.pos"].grad is not None and not parents["lights.pos"].grad.any()
    for key in ("disk.pos", "disk.normal"):
        for v in range(c["n"]):
            assert_array_close(to_np(parents[key].grad)[v], per_view[key][v], 2e-4, f"{'+'.join(outputs)} {key}[{v}]")


# ---- 6. partial wants ----------------------------------------------------------------------------------------------------------
def test_only_two_camera_tensors_require_grad(case2):
    c = case2
    wanted = {1: ("eye",), 3: ("up",)}
    out, leaves, parents, cams = _run(c["scene"], c["cameras"], c["own"], cam=lambda v: wanted.get(v, ()), grad_own=(),
                                      grad_shared=False)
    assert not leaves and not any(p.requires_grad for p in parents.values())
    assert out["image"].requires_grad and out["pos"].requires_grad
    assert torch.equal(out["image"].detach(), c["fwd"]["image"])
    masked_loss(out, c["g"], c["far"]).backward()
    torch.cuda.synchronize()
    for v, cam in enumerate(cams):
        for k in CAM:
            if k in wanted.get(v, ()):
                want = c["got_cam"]["camera." + k][v]
                assert np.abs(want).max() > 0
                got = cam[k].grad.cpu().numpy().astype(np.float64)
                assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (v, k)
            else:
                assert cam[k].grad is None, (v, k)


def test_one_up_vector_shared_by_all_views(case2):
    c = case2
    up3 = torch.tensor(np.asarray(c["scene"]["camera"]["up"], dtype=np.float64)[:3], dtype=torch.float32, device=DEV,
                       requires_grad=True)
    cams = [{"up": up3} for _ in range(c["n"])]
    out, _, _, _ = _run(c["scene"], c["cameras"], c["own"], grad_own=(), grad_shared=False, cam_tensors=cams)
    masked_loss(out, c["g"], c["far"]).backward()
    torch.cuda.synchronize()
    want = sum(c["per_view"]["camera.up"][v][:3] for v in range(c["n"]))
    assert up3.grad is not None and up3.grad.shape == (3,)
    assert np.all(np.isfinite(want)) and np.abs(want).max() > 0
    assert_array_close(to_np(up3.grad), want, 2e-4, "shared up")


def test_eyes_as_rows_of_one_pose_tensor(case2):
    c = case2
    parent = torch.tensor(np.asarray(EYES3, dtype=np.float64), dtype=torch.float32, device=DEV, requires_grad=True)
    cams = [{"eye": parent[v]} for v in range(c["n"])]         # non-leaf slices
    out, _, _, _ = _run(c["scene"], c["cameras"], c["own"], grad_own=(), grad_shared=False, cam_tensors=cams)
    masked_loss(out, c["g"], c["far"]).backward()
    torch.cuda.synchronize()
    assert parent.grad is not None and parent.grad.shape == (c["n"], 4)
    got = to_np(parent.grad)
    for v in range(c["n"]):
        assert_array_close(got[v], c["per_view"]["camera.eye"][v], 2e-4, f"pose row {v}")
    assert not got[AWAY3].any() and all(got[v].any() for v in range(c["n"]) if v != AWAY3)


def test_no_grad_and_numpy_shading_leave_the_cameras_alone(case2):
    from surf_renderer_amd import render_views
    c = case2
    with torch.no_grad():
        out, _, _, cams = _run(c["scene"], c["cameras"], c["own"])
    for k in OUTPUTS + ("nearest",):
        assert not out[k].requires_grad and out[k].grad_fn is None
        assert torch.equal(out[k], c["fwd"][k]), k
    # numpy shading: the camera tensors are read, never attached
    leaf_scene, leaves = gpu_leaf_scene(c["scene"], ("lights.pos",))
    cams = _cam_tensors(c["cameras"])
    cameras = [dict(c["cameras"][v], **cams[v]) for v in range(c["n"])]
    # (the numpy shading takes a camera array at full precision: the plain call gets the tensors' float32 values)
    plain = render_views(c["scene"], [dict(c["cameras"][v], **{k: to_np(t) for k, t in cams[v].items()}) for v in range(c["n"])],
                         device=DEV)
    out = render_views(leaf_scene, cameras, device=DEV)
    assert set(out) == {"image", "depth", "nearest"} and torch.equal(out["image"].detach(), plain["image"])
    out["image"].sum().backward()
    assert leaves["lights.pos"].grad is not None and leaves["lights.pos"].grad.any()
    assert all(t.grad is None for cam in cams for t in cam.values())
    with pytest.raises(ValueError):
        render_views(c["scene"], c["cameras"], device=DEV, aux=True)


# ---- 7. shadows ----------------------------------------------------------------------------------------------------------------
def test_shadow_rays_with_camera_leaves():
    scene, kw, cameras, lights = shadow_case()
    n = len(cameras)
    own = {"lights.pos": lights}
    g = batch_upstream(n, 9)
    out, leaves, parents, cams = _run(scene, cameras, own, grad_own=("lights.pos",), kw=kw, shadow=True)
    assert out["image"].requires_grad and not out["visibility"].requires_grad
    far = float(scene["camera"]["far"])
    masked_loss(out, g, far).backward()
    torch.cuda.synchronize()
    vis = visibility_rows(out["visibility"].cpu().numpy(), lights.shape[1])
    hit = to_np(out["depth"]) <= far
    assert all(h.mean() > 0.1 for h in hit)
    shadowed = 1.0 - np.mean([vis[v][:, hit[v].reshape(-1)].mean() for v in range(n)])
    assert 0.01 < shadowed < 0.99                           # the scene does cast shadows
    scenes = [view_scene(scene, cameras[v], {"lights.pos": own["lights.pos"][v]}) for v in range(n)]
    refs = view_winners(out)
    shared, per_view = _helper(scenes, g, refs, ("lights.pos",), visibility=vis, **kw)
    _check_wanted(per_view)
    _compare_cameras(_cam_grads(cams), per_view, "shadow")
    assert_grads_close(leaf_grads(leaves), shared, 2e-4, "shadow")
    for v in range(n):
        assert_array_close(to_np(parents["lights.pos"].grad)[v], per_view["lights.pos"][v], 2e-4, f"shadow lights.pos[{v}]")
    # The bits are used.  Visibility is a factor on the light terms of the image alone: depth, normal and pos do not
    # depend on it, and with random upstream gradients on them the geometry terms of a camera gradient are hundreds of
    # times its image term, so the comparison is made where the bits act -- the same batch with a loss on the image alone.
    g_i = {"image": g["image"]}
    out_i, _, _, cams_i = _run(scene, cameras, own, grad_own=(), grad_shared=False, kw=kw, shadow=True)
    assert torch.equal(out_i["visibility"], out["visibility"]) and torch.equal(out_i["nearest"], out["nearest"])
    masked_loss(out_i, g_i, far).backward()
    torch.cuda.synchronize()
    _, lit = _helper(scenes, g_i, refs, ("lights.pos",), visibility=vis, **kw)
    _, plain = _helper(scenes, g_i, refs, ("lights.pos",), **kw)
    _check_wanted({k: lit[k] for k in CAM_KEYS})
    _compare_cameras(_cam_grads(cams_i), lit, "shadow, image alone")
    for key in CAM_KEYS:
        a, b = np.stack(lit[key]), np.stack(plain[key])
        print(f"{key}: with / without the bits differ by {np.abs(a - b).max():.3g} of max {np.abs(a).max():.4g}")
        assert np.abs(a - b).max() > 1e-3 * np.abs(a).max(), key


# ---- 8. orthographic -----------------------------------------------------------------------------------------------------------
def test_orthographic_views_with_camera_leaves():
    scene, cameras = ortho_case()
    g = batch_upstream(2, 13)
    out, leaves, _, cams = _run(scene, cameras, {}, kw={})
    far = float(scene["camera"]["far"])
    masked_loss(out, g, far).backward()
    torch.cuda.synchronize()
    refs = view_winners(out)
    assert all(h > 0.3 for h in _hits(refs, far))
    shared, per_view = _helper([view_scene(scene, cam) for cam in cameras], g, refs, ())
    _check_wanted(per_view)
    _compare_cameras(_cam_grads(cams), per_view, "ortho")
    assert set(shared) == set(leaves)
    assert_grads_close(leaf_grads(leaves), shared, 2e-4, "ortho")


# ---- 9. more workgroups than finish rows -----------------------------------------------------------------------------------------
def test_more_workgroups_than_finish_rows(base):
    """136 x 120: 3 x 30 = 90 workgroups per view, more than the finish kernel's 85 rows -- its strided loop takes a
    second round, and view 1's slice of the partial sums starts beyond one round."""
    w, h = 136, 120
    scene = copy.deepcopy(base["scene"])
    cameras = [dict(cam, viewport=[0, 0, w, h]) for cam in base["cameras"][:2]]
    g = batch_upstream(2, 23, h, w)
    out, leaves, _, cams = _run(scene, cameras, {})
    assert out["pos"].shape == (2, h, w, 3)
    masked_loss(out, g, base["far"]).backward()
    torch.cuda.synchronize()
    refs = view_winners(out)
    assert all(hh > 0.3 for hh in _hits(refs, base["far"]))
    shared, per_view = _helper([view_scene(scene, cam) for cam in cameras], g, refs, (), **KW3)
    _check_wanted(per_view)
    _compare_cameras(_cam_grads(cams), per_view, "136x120")
    assert_grads_close(leaf_grads(leaves), shared, 2e-4, "136x120")


# ---- 10. workspace hygiene ---------------------------------------------------------------------------------------------------
def test_backward_leaves_the_bin_counters_alone_and_reads_nothing_stale(base):
    from surf_renderer_amd import _lib
    from surf_renderer_amd import renderer as R
    b = base
    n = 3                                                   # views 0, 1 and the look-away view
    scene = view_scene(b["scene"])
    buf = R.flatten_scene(scene, DEV)
    cams = [R.camera_struct(cam, "torch") for cam in b["cameras"][:n]]
    kw = dict(shading="torch", **KW3)

    def frames():
        return (torch.empty((n, H, W, 3), dtype=torch.float32, device=DEV), torch.empty((n, H, W), dtype=torch.float32, device=DEV),
                torch.empty((n, H, W), dtype=torch.int32, device=DEV), torch.empty((n, H, W, 3), dtype=torch.float32, device=DEV),
                torch.empty((n, H, W, 3), dtype=torch.float32, device=DEV))

    img_a, dep_a, near_a, nrm_a, pos_a = frames()
    ws = R.render_views_buffers(buf, cams, img_a, dep_a, near_a, aux=(nrm_a, pos_a), **kw)
    state = R._ws_state(ws)
    assert state is not None and state[0] == "clean"
    g_alb = torch.zeros_like(buf.tensors["materials.albedo"])
    g_dpos = torch.zeros_like(buf.tensors["disk.pos"])
    grads = (_lib.SrhGrads * n)()
    cam_out = torch.full((n, 3, 4), float("nan"), dtype=torch.float32, device=DEV)
    cgrads = (_lib.SrhCameraGrads * n)()
    for v in range(n):
        grads[v].albedo = g_alb.data_ptr()
        grads[v].pos[buf.kinds.index("disk")] = g_dpos.data_ptr()
        for i, k in enumerate(CAM):
            setattr(cgrads[v], k, cam_out[v, i].data_ptr())
    g = {k: torch.as_tensor(b["g"][k][:n], device=DEV).contiguous() for k in OUTPUTS}
    scratch = buf.ensure_camera_scratch_views(W, H, n)
    scratch.fill_(float("nan"))
    assert R.render_views_bwd_buffers(buf, cams, g["image"], g["depth"], near_a, dep_a, grads, workspace=ws,
                                      g_normals=g["normal"], g_poses=g["pos"], camera_grads=cgrads,
                                      camera_scratch=scratch, **kw) is ws
    assert R._ws_state(ws) == state                          # still noted clean: the next forward clears nothing
    img_b, dep_b, near_b, nrm_b, pos_b = frames()
    assert R.render_views_buffers(buf, cams, img_b, dep_b, near_b, workspace=ws, aux=(nrm_b, pos_b), **kw) is ws
    torch.cuda.synchronize()
    for a, c in ((img_a, img_b), (dep_a, dep_b), (near_a, near_b), (nrm_a, nrm_b), (pos_a, pos_b)):
        assert torch.equal(a, c)
    assert g_alb.any() and g_dpos.any() and bool(torch.isfinite(g_alb).all()) and bool(torch.isfinite(g_dpos).all())
    got = cam_out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    refs = [{"nearest": near_a[v].cpu().numpy(), "depth": dep_a[v].cpu().numpy().astype(np.float64)} for v in range(n)]
    hits = _hits(refs, b["far"])
    assert hits[AWAY3] == 0 and hits[0] > 0.5 and hits[1] > 0.5
    _, per_view = _helper([view_scene(b["scene"], b["cameras"][v]) for v in range(n)], {k: b["g"][k][:n] for k in OUTPUTS},
                          refs, (), **KW3)
    _check_wanted(per_view, AWAY3)
    for i, key in enumerate(CAM_KEYS):
        for v in range(n):
            assert_array_close(got[v, i], per_view[key][v], 2e-4, f"buffers {key}[{v}]")
    assert not got[AWAY3].any()
