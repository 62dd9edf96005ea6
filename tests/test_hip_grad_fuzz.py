"""GPU: the camera, batched and aux backward paths (k_render_bwd_tch<kCam>, k_camera_finish, k_render_bwd_views,
k_render_bwd_tch_views, k_camera_finish_views and the host chunking of render_views) on the random scenes, hazard cameras
and mixed per-view overrides of tests/grad_fuzz_cases.py, against the fp64 oracle fed the GPU frames' winners
(oracle/torch_oracle.gradients_tch, camera=True) and, for the batches, against one render + backward per view.

Tolerances are the project's existing ones: 5e-4 of the largest entry per array + 1e-6 against the oracle (the gradient
fuzzers of tests/test_hip_backward.py and tests/test_hip_aux_grad.py); against render per view the bounds of
tests/test_hip_views_camera_aux.py::test_batch_equals_render_per_view -- forward bit-equal, camera gradients 1e-6 of the
largest entry, own tensors RUN_TO_RUN of theirs, a shared leaf RUN_TO_RUN x the sum over its views of each view's largest
entry (every per-view term carries RUN_TO_RUN of its own maximum), a camera tensor all views share 1e-6 x the sum of
its views' largest entries likewise; the row-slab sums 2e-4 (test_row_slabs_sum_to_the_whole_frame).  The generator
redraws a batch one of whose gradient sums cancels harder than fp32 atomics resolve (cancelling_sums: sum|per-pixel
term| x 2^-23 above the bound), a condition of the fp64 oracle alone.  No GPU result skips a case: the generator redraws
scenes by rules the CPU decides (tests/test_grad_fuzz_cases_cpu.py pins them), and every drawn case and array is compared.
profiles/grad_fuzz.txt records the measured errors."""
import numpy as np
import pytest
import torch

import grad_fuzz_cases as G
from grad_cases import (CAM, DEV, NP_KEYS, RUN_TO_RUN, TCH_KEYS, assert_array_close, camera_leaves, gpu_leaf_scene,
                        gpu_tensor, grad_kwargs, leaf_grads, masked_loss, to_np, view_winners, winners)
from oracle import np_oracle, torch_oracle
from oracle.torch_oracle import CAMERA_KEYS as CAM_KEYS, LEAF_KEYS, gradients_tch
from views_cases import visibility_rows

pytestmark = pytest.mark.gpu

TOL = 5e-4


class _Worst:
    """The largest max err / max|want| seen per array class, for the log."""

    def __init__(self):
        self.worst = {}

    def close(self, cls, got, want, tag, tol=TOL):
        want = np.asarray(want, dtype=np.float64)
        got = np.asarray(got, dtype=np.float64).reshape(want.shape)
        scale = np.abs(want).max()
        if scale > 0:
            ratio = np.abs(got - want).max() / scale
            if ratio >= self.worst.get(cls, (-1.0, ""))[0]:
                self.worst[cls] = (ratio, tag)
        assert_array_close(got, want, tol, tag)

    def note(self, cls, ratio, tag):
        """A figure measured elsewhere (an error over its bound) for the same log."""
        if ratio >= self.worst.get(cls, (-1.0, ""))[0]:
            self.worst[cls] = (float(ratio), tag)

    def report(self, title):
        for cls, (ratio, tag) in sorted(self.worst.items()):
            print(f"[grad fuzz] {title}: worst {cls} max err / max|want| {ratio:.3g} ({tag})")


@pytest.fixture(scope="module")
def camera_cases():
    return G.camera_cases()


@pytest.fixture(scope="module")
def views_cases():
    return G.views_cases()


# ---- one render, camera leaves ------------------------------------------------------------------------------------------
def _plain_vector(it, case):
    """The camera vector a list-typed case hands to the renderer as it is -- a Python list of float64 that float32 does
    not hold, without grad -- while the other two are leaves: the host's own rounding of such a vector is then part of
    a gradient run (with three float32 leaves it would be met in forward-only renders alone).  None for array cameras."""
    return CAM[it % 3] if "lists" in case.get("hazards", ()) else None


def _camera_backward(case, g, rows=None, plain=None):
    """render(shading='torch') with GPU leaves for the scene and eye / at / up (all but `plain`), masked_loss over the
    outputs in g."""
    from surf_renderer_amd import render
    scene = case["scene"]
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
    cam = {k: t for k, t in camera_leaves(scene["camera"]).items() if k != plain}
    assert plain is None or isinstance(scene["camera"][plain], list)
    leaf_scene["camera"] = dict(leaf_scene["camera"], **cam)
    res = render(leaf_scene, device=DEV, shading="torch", rows=rows, shadow=case["shadow"], **case["kw"])
    masked_loss(res, g, scene["camera"]["far"]).backward()
    torch.cuda.synchronize()
    grads = leaf_grads(leaves)
    for k, t in cam.items():
        assert t.grad is not None and t.grad.shape == t.shape, f"camera.{k}"
        grads["camera." + k] = to_np(t.grad)
    return grads, res


def _camera_visibility(case):
    """The GPU frame's own visibility bits as the oracle's (L, N) factors; None without shadow rays."""
    if not case["shadow"]:
        return None
    from surf_renderer_amd import render
    with torch.no_grad():
        plain = render(case["scene"], device=DEV, shading="torch", shadow=True, **case["kw"])
    bits = plain["light_visibility"].cpu().numpy()
    return visibility_rows([bits], np.asarray(case["scene"]["lights"]["pos"]).shape[0])[0]


def _camera_oracle(case, g, res, vis):
    return gradients_tch(case["scene"], **grad_kwargs(g), ref=winners(res), camera=True, visibility=vis, **case["kw"])


def _cls(key):
    return "camera" if key in CAM_KEYS else "shared"


def test_fuzz_camera_gradients(camera_cases):
    """N_CAMERA random scenes (all four primitive kinds; cameras inside the cloud, `at` 0.05 from the eye, `up` within
    5 degrees of the view direction, un-normalised and list-typed vectors, both projections), random double_sided /
    use_quartic / shadow and a random non-empty subset of the outputs in the loss: eye, at, up and every scene leaf
    against the camera oracle.  Every fourth scene is also rendered as two row slabs whose camera gradients must sum to
    the frame's; every sixth has more workgroups than the camera finish kernel has rows."""
    worst = _Worst()
    for it, case in enumerate(camera_cases):
        tag = f"scene {it} {case['kw']} shadow={case['shadow']} {case['outputs']} {sorted(case['hazards'])}"
        plain = _plain_vector(it, case)
        got, res = _camera_backward(case, case["g"], plain=plain)
        same = (res["nearest"].cpu().numpy() == case["ref"]["nearest"]).mean()
        assert same > 0.999, f"{tag}: nearest equals the oracle's on {same:.5f} of the pixels"
        want = _camera_oracle(case, case["g"], res, _camera_visibility(case))
        assert set(want) == set(got) | ({"camera." + plain} if plain else set())
        keys = [k for k in CAM_KEYS if k in got]
        for key in got:
            worst.close(_cls(key), got[key], want[key], f"{tag} {key}")
        for key in keys:
            assert got[key][3] == 0.0
        if case["slab"] is not None:
            r, H = case["slab"], case["scene"]["camera"]["viewport"][3]
            assert r % 4 and 0 < r < H
            top, tres = _camera_backward(case, {k: v[:r] for k, v in case["g"].items()}, rows=(0, r), plain=plain)
            bottom, _ = _camera_backward(case, {k: v[r:] for k, v in case["g"].items()}, rows=(r, H), plain=plain)
            assert tres["image"].shape[0] == r
            for key in keys:                        # test_row_slabs_sum_to_the_whole_frame's bound
                worst.close("camera slabs", top[key] + bottom[key], got[key], f"{tag} slabs at {r} {key}", tol=2e-4)
    worst.report("camera")


@pytest.mark.parametrize("ortho", [False, True])
def test_up_a_tenth_of_a_degree_from_the_view_direction(ortho):
    """Found by the camera fuzz (seed 9101, scene 96: orthographic, `up` 0.74 degrees from the view direction, camera.up
    1.1 % off): k_camera_finish differentiated exact unit vectors where the forward and the reference divide by
    sqrt(|v|^2 + 3e-10).  The g10 / n1 fixture scene with `up` a tenth of a degree from the view direction, at the
    curated tests' 2e-4: the exact-norm chain rule is 1e-3 off on the orthographic camera
    (tests/test_grad_fuzz_cases_cpu.py::test_the_near_parallel_up_case_tells_the_two_norms_apart)."""
    from grad_cases import full_scene, random_upstream
    scene = full_scene(ortho)
    scene["camera"] = G.near_parallel_up_camera(scene["camera"])
    case = dict(scene=scene, shadow=False, kw={})
    g = random_upstream()
    got, res = _camera_backward(case, g)
    want = _camera_oracle(case, g, res, None)
    for key in CAM_KEYS:
        assert np.abs(want[key]).max() > 1.0
        assert_array_close(got[key], want[key], 2e-4, f"up 0.1 degrees from the view, ortho={ortho} {key}")


# ---- batches of views ---------------------------------------------------------------------------------------------------------
def _wants_grad(v, i):
    """Which separate override tensors require grad: all but one in five, by view and key position."""
    return (v + i) % 5 != 0


def _run_views(case, g, shading="torch", keys=None):
    """render_views on the batch with GPU leaves: every shared leaf requires grad; an every-view override in
    flags['stacked'] is a slice of one stacked parent that requires grad, every other override a tensor of its own that
    requires grad unless _wants_grad says otherwise; under torch shading each view has its own eye / at / up leaves,
    except the one tensor flags['shared_camera'] names (so a batch's list-typed camera vectors reach the renderer as
    lists only under numpy shading; the single-render fuzz keeps one of them a list, _plain_vector).  `keys` restricts
    the overrides (numpy shading).  Returns (out,
    shared leaves, {key: {view: (tensor, parent row or None)}}, per-view camera tensors)."""
    from surf_renderer_amd import render_views
    scene, cameras, overrides, batch, flags = case
    n = flags["n"]
    torch_shading = shading == "torch"
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS if torch_shading else NP_KEYS)
    own, ov_tensors = {}, [{} for _ in range(n)]
    for i, key in enumerate(G.leaf_keys(scene)):
        views = [v for v in range(n) if key in overrides[v]]
        if not views or (keys is not None and key not in keys):
            continue
        if key in flags["stacked"]:
            parent = gpu_tensor(np.stack([overrides[v][key] for v in range(n)]))
            own[key] = {v: (parent, v) for v in range(n)}
        else:
            own[key] = {v: (gpu_tensor(overrides[v][key], _wants_grad(v, i)), None) for v in views}
        for v in views:
            t, row = own[key][v]
            ov_tensors[v][key] = t if row is None else t[row]
    cams = [{} for _ in range(n)]
    if torch_shading:
        cams = [camera_leaves(cam) for cam in cameras]
        if flags["shared_camera"] is not None:
            for c in cams[1:]:
                c[flags["shared_camera"]] = cams[0][flags["shared_camera"]]
    more = dict(aux=flags["aux"], shadow=flags["shadow"], **G.shade_kw(flags)) if torch_shading else {}
    out = render_views(leaf_scene, [dict(cameras[v], **cams[v]) for v in range(n)], device=DEV, shading=shading,
                       overrides=ov_tensors, batch=batch, **more)
    far = float(scene["camera"]["far"]) if torch_shading else None
    masked_loss(out, g, far).backward()
    torch.cuda.synchronize()
    return out, leaves, own, cams


def _own_grad(own, key, v):
    """The gradient view v's override of `key` received: ndarray, or None for a tensor that does not require grad."""
    t, row = own[key][v]
    if not t.requires_grad:
        assert t.grad is None, (key, v)
        return None
    assert t.grad is not None and t.grad.shape == t.shape, f"{key}[{v}] got no gradient"
    return to_np(t.grad) if row is None else to_np(t.grad)[row]


def _views_oracle(case, g, out, camera=True):
    """gradients_tch per view on the batch's own winners and visibility bits -> mixed_batch_gradients."""
    scene, cameras, overrides, _, flags = case
    n = flags["n"]
    scenes = G.batch_scenes(scene, cameras, overrides)
    refs = view_winners(out)
    vis = None
    if flags["shadow"]:
        vis = visibility_rows(out["visibility"].cpu().numpy(), np.asarray(scene["lights"]["pos"]).shape[0])
    per_view = [gradients_tch(scenes[v], **grad_kwargs({k: a[v] for k, a in g.items()}), ref=refs[v],
                              visibility=None if vis is None else vis[v], camera=camera, **G.shade_kw(flags))
                for v in range(n)]
    return G.mixed_batch_gradients(per_view, [set(overrides[v]) | set(CAM_KEYS) for v in range(n)])


def _compare_views(case, tag, worst, out, leaves, own, cams, shared, per_view, classes=("shared", "own", "camera"),
                   away="flags"):
    """Every array of the batch against (shared, per_view): shared leaves (zeros for a leaf every view overrides), each
    own tensor per view (None for one that does not require grad, zeros for a view that sees nothing), each camera
    tensor (a shared one: the sum over the views)."""
    scene, _, overrides, _, flags = case
    n = flags["n"]
    away = flags["away"] if away == "flags" else away
    got = leaf_grads(leaves)
    for key, t in leaves.items():
        worst.close(classes[0], got[key], shared.get(key, np.zeros(t.shape)), f"{tag} shared {key}")
    for key, by_view in own.items():
        for v in by_view:
            g = _own_grad(own, key, v)
            if g is not None:
                worst.close(classes[1], g, per_view[key][v], f"{tag} {key}[{v}]")
                if v == away:
                    assert not g.any(), f"{tag} {key}[{v}]: the look-away view's gradient is not zero"
    for k in (CAM if cams[0] else ()):
        if flags["shared_camera"] == k:
            t = cams[0][k]
            assert t.grad is not None and t.grad.shape == t.shape
            worst.close(classes[2], to_np(t.grad), sum(per_view["camera." + k][v] for v in range(n)),
                        f"{tag} camera.{k} shared by {n} views")
            continue
        for v in range(n):
            t = cams[v][k]
            assert t.grad is not None and t.grad.shape == t.shape, f"{tag} camera.{k}[{v}] got no gradient"
            worst.close(classes[2], to_np(t.grad), per_view["camera." + k][v], f"{tag} camera.{k}[{v}]")
            if v == away:
                assert not t.grad.any()


def _compare_with_render_per_view(case, tag, worst, out, leaves, own, cams):
    """The second reference: one render + backward per view on the same device.  `worst` is told each error over its
    bound (1 = at the bound)."""
    from surf_renderer_amd import render
    scene, cameras, overrides, _, flags = case
    n, g = flags["n"], flags["g"]
    far = float(scene["camera"]["far"])
    scenes = G.batch_scenes(scene, cameras, overrides)
    sums, bound, cam_sum, cam_bound = {}, {}, 0.0, 0.0
    for v in range(n):
        leaf_scene, one = gpu_leaf_scene(scenes[v], TCH_KEYS)
        cam = camera_leaves(cameras[v])
        leaf_scene["camera"] = dict(leaf_scene["camera"], **cam)
        res = render(leaf_scene, device=DEV, shading="torch", shadow=flags["shadow"], **G.shade_kw(flags))
        for k in ("image", "depth", "nearest") + (("normal", "pos") if flags["aux"] else ()):
            assert torch.equal(res[k].detach(), out[k][v].detach()), f"{tag} view {v} {k}: batch differs from render()"
        masked_loss(res, {k: a[v] for k, a in g.items()}, far).backward()
        torch.cuda.synchronize()
        for k in CAM:
            want = to_np(cam[k].grad)
            if flags["shared_camera"] == k:
                cam_sum, cam_bound = cam_sum + want, cam_bound + np.abs(want).max()
                continue
            err = np.abs(to_np(cams[v][k].grad) - want).max()
            worst.note("camera / render() bound", err / max(1e-6 * np.abs(want).max(), 1e-300), f"{tag} camera.{k}[{v}]")
            assert err <= 1e-6 * np.abs(want).max(), f"{tag} camera.{k}[{v}]: {err:.3g} of {np.abs(want).max():.4g}"
        for key, want in leaf_grads(one).items():
            if key in overrides[v]:
                got = _own_grad(own, key, v)
                if got is not None:
                    err = np.abs(got.reshape(want.shape) - want).max()
                    worst.note("own / render() bound", err / max(RUN_TO_RUN * np.abs(want).max(), 1e-300), f"{tag} {key}[{v}]")
                    assert err <= RUN_TO_RUN * max(np.abs(want).max(), 1e-30), f"{tag} {key}[{v}]: {err:.3g}"
            else:
                sums[key] = sums.get(key, 0.0) + want
                bound[key] = bound.get(key, 0.0) + np.abs(want).max()
    for key, want in sums.items():
        err = np.abs(to_np(leaves[key].grad).reshape(want.shape) - want).max()
        print(f"{tag} {key}: batch against the per-view sum {err:.3g}, bound {RUN_TO_RUN * bound[key]:.3g}")
        worst.note("shared / render() bound", err / max(RUN_TO_RUN * bound[key], 1e-300), f"{tag} shared {key}")
        assert err <= RUN_TO_RUN * max(bound[key], 1e-30), f"{tag} shared {key}: {err:.3g}"
    if flags["shared_camera"] is not None:
        k = flags["shared_camera"]
        # every view's term is held to 1e-6 of its own largest entry above, so their sum to 1e-6 x the sum of those
        err = np.abs(to_np(cams[0][k].grad) - cam_sum).max()
        worst.note("shared camera / render() bound", err / max(1e-6 * cam_bound, 1e-300), f"{tag} camera.{k} shared by {n} views")
        assert err <= 1e-6 * max(cam_bound, 1e-30), f"{tag} shared camera.{k}: {err:.3g}"


def _numpy_case(case):
    """The batch under numpy shading: overrides of the object leaves and NP_KEYS alone, no shadow, no aux, image + depth."""
    scene, cameras, overrides, batch, flags = case
    keys = [k for k in G.leaf_keys(scene) if k not in TCH_KEYS or k in NP_KEYS]
    overrides = [{k: a for k, a in ov.items() if k in keys} for ov in overrides]
    return (scene, cameras, overrides, batch, dict(flags, aux=False, shadow=False)), keys


def test_fuzz_views_backward(views_cases):
    """N_VIEWS random batches (1 to 7 views, batch = 1, 2, 3, n, n + 3 and round robin, per key no override, one for every
    view or one for a proper subset of the views, shared and own camera tensors, aux / shadow / both projections) through
    render_views(shading='torch') against the oracle per view and against render() per view; the first two perspective
    batches also under numpy shading against torch_oracle.gradients."""
    worst = _Worst()
    for it, case in enumerate(views_cases):
        flags = case[4]
        tag = (f"batch {it} n={flags['n']} batch={flags['batch_kind']} aux={flags['aux']} shadow={flags['shadow']} "
               f"ortho={flags['ortho']} {flags['outputs']}")
        out, leaves, own, cams = _run_views(case, flags["g"])
        assert set(leaves) == set(G.leaf_keys(case[0]))
        shared, per_view = _views_oracle(case, flags["g"], out)
        _compare_views(case, tag, worst, out, leaves, own, cams, shared, per_view)
        _compare_with_render_per_view(case, tag, worst, out, leaves, own, cams)
    for it, case in [(i, c) for i, c in enumerate(views_cases) if not c[4]["ortho"]][:2]:
        case, keys = _numpy_case(case)
        scene, cameras, overrides, _, flags = case
        n = flags["n"]
        W, H = scene["camera"]["viewport"][2:]
        g = G.random_upstream(np.random.RandomState(G.VIEWS_SEED + it), (n, H, W), ("image", "depth"))
        out, leaves, own, cams = _run_views(case, g, shading="numpy", keys=keys)
        refs = view_winners(out)
        scenes = G.batch_scenes(scene, cameras, overrides)
        per_view = [torch_oracle.gradients(scenes[v], g["image"][v], g["depth"][v], ref=refs[v]) for v in range(n)]
        shared, by_view = G.mixed_batch_gradients(per_view, [set(ov) for ov in overrides])
        assert set(leaves) == set(per_view[0])
        # the view that hits nothing does so under the torch backend's semantics; the numpy backend's own camera basis
        # and plane test may find the wall from there, so its zeros are asserted only where the numpy oracle sees none
        away = flags["away"]
        if away is not None and np.isfinite(np_oracle.render(scenes[away])["depth"]).any():
            away = None
        _compare_views(case, f"batch {it} numpy shading", worst, out, leaves, own, cams, shared, by_view,
                       classes=("shared numpy", "own numpy", None), away=away)
    worst.report("views")


# ---- small gradients under large ones ------------------------------------------------------------------------------------
def _object_rows(scene, index):
    """{object leaf key: the one row that may be non-zero when only primitive `index` is in the loss, or None}."""
    kind, row = G.locate(scene, index)
    return {f"{k}.{name}": (row if k == kind else None) for k in scene["objects"] for name in LEAF_KEYS[k]}


def _assert_other_rows_zero(arr, row, tag):
    arr = np.asarray(arr)
    other = np.ones(arr.shape[0], dtype=bool)
    if row is not None:
        other[row] = False
    assert not arr[other].any(), f"{tag}: rows {np.nonzero(arr[other].reshape(other.sum(), -1).any(axis=1))[0][:5]} " \
                                 f"of the other primitives are not zero"


def _print_share(tag, key, row, masked, full):
    top = np.abs(np.asarray(full)).max()
    if row is not None and top > 0:
        print(f"[grad fuzz] {tag} {key}[{row}]: its row is {np.abs(np.asarray(masked)[row]).max() / top:.3g} of the "
              f"unmasked array's largest entry")


def test_fuzz_small_winners_are_not_hidden(camera_cases, views_cases):
    """|got - want| <= 5e-4 max|want| per array lets a primitive whose row is far below the array's largest pass with a
    wholly wrong gradient.  For the three primitives that win the fewest pixels of a frame (winner_masks, from the GPU
    frame) the backward runs again with every upstream zeroed outside that primitive's pixels, on the GPU and in the
    oracle alike: max|want| is then that primitive's own row, and every other object row of the GPU result is exactly
    zero.  First eight camera scenes, first four batches.  tests/test_hip_backward_runs.py holds every entry of every
    leaf to a bound of its own (grad_cases.entry_bounds), numpy shading and the kernels without camera leaves included."""
    worst = _Worst()
    for it, case in enumerate(camera_cases[:G.N_MASKED_CAMERA]):
        scene, far = case["scene"], case["scene"]["camera"]["far"]
        plain = _plain_vector(it, case)
        full, res = _camera_backward(case, case["g"], plain=plain)
        vis = _camera_visibility(case)
        chosen = G.winner_masks(res["nearest"].cpu().numpy(), to_np(res["depth"]), far, k=3)
        assert chosen
        for index, mask in chosen:
            tag = f"scene {it} primitive {index} ({mask.sum()} px)"
            g = G.mask_upstream(case["g"], mask)
            got, again = _camera_backward(case, g, plain=plain)
            assert torch.equal(again["nearest"], res["nearest"])
            want = _camera_oracle(case, g, res, vis)
            for key in got:
                worst.close("masked " + _cls(key), got[key], want[key], f"{tag} {key}")
            for key, row in _object_rows(scene, index).items():
                _assert_other_rows_zero(got[key], row, f"{tag} {key}")
                _print_share(tag, key, row, want[key], full[key])
    for it, case in enumerate(views_cases[:G.N_MASKED_VIEWS]):
        scene, _, overrides, _, flags = case
        n, far = flags["n"], float(scene["camera"]["far"])
        out, leaves, own, _ = _run_views(case, flags["g"])
        full = leaf_grads(leaves)
        chosen = G.winner_masks(out["nearest"].cpu().numpy(), to_np(out["depth"]), far, k=3)
        assert chosen
        for index, mask in chosen:
            tag = f"batch {it} primitive {index} ({mask.sum()} px in views {sorted(set(np.nonzero(mask)[0].tolist()))})"
            g = G.mask_upstream(flags["g"], mask)
            m_out, m_leaves, m_own, m_cams = _run_views(case, g)
            assert torch.equal(m_out["nearest"], out["nearest"])
            shared, per_view = _views_oracle(case, g, m_out)
            _compare_views(case, tag, worst, m_out, m_leaves, m_own, m_cams, shared, per_view,
                           classes=("masked shared", "masked own", "masked camera"))
            got = leaf_grads(m_leaves)
            for key, row in _object_rows(scene, index).items():
                _assert_other_rows_zero(got[key], row, f"{tag} shared {key}")
                if key in shared:
                    _print_share(tag, key, row, shared[key], full[key])
                for v in m_own.get(key, ()):
                    grad = _own_grad(m_own, key, v)
                    if grad is not None:
                        _assert_other_rows_zero(grad, row, f"{tag} {key}[{v}]")
    worst.report("masked")
