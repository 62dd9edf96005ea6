"""GPU: camera_grad=True of depth_to_surfels, projection_renderer_differentiable_fast and projection_reverse_renderer
(srh_depth_to_surfels_bwd_view, srh_projection_bwd_view, srh_reverse_projection_bwd_view) against the fp64 restatement
with camera leaves, tests/camera_chain_oracle.py, on every seeded case of the three layers' case modules;
tests/test_camera_chain_oracle_cpu.py ties that restatement to the layers' own oracles.

Stated tolerance for the camera gradients: the layers' own, rtol 2e-6 with atol 2e-7 max|want| per array
(projection_checks).  It holds for the same reason as for the other gradients: the kernels sum the restatement's fp64
products from the same fp32 inputs without atomics, the chain from the per-view matrix to eye / at / up is fp64 autograd,
and the result is rounded once into the leaf's dtype.

The reduction can break at a partial wave (17x9: N = 153), across waves (12x16: three waves), across workgroups (36x48:
seven workgroups, the only seeded case whose finish kernel adds more than one partial) and at a single lane (1x1);
every property below is checked on 36x48 and on a batched case.  A lift of 132x128 (66 workgroups) is the one place
where a row of the finish kernel adds a second partial before its tree."""
import functools

import numpy as np
import pytest
import torch

import camera_chain_oracle as co
import projection_cases as pc
import projection_oracle as po
import reverse_projection_cases as rc
import reverse_projection_oracle as ro
import surfels_cases as sc
from projection_checks import assert_bit_identical, compare_grads, compare_values, one_view, to_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def leaves(camera, dtype=torch.float32, device=DEV):
    """The camera with eye, at and up as leaves that require grad."""
    return dict(camera, **{k: torch.tensor(np.asarray(camera[k]), dtype=dtype, device=device, requires_grad=True)
                           for k in co.CAMERA_KEYS})


def camera_grads(cameras):
    return {label: {k: to_np(cam[k].grad) for k in co.CAMERA_KEYS
                    if isinstance(cam[k], torch.Tensor) and cam[k].is_leaf} for label, cam in cameras.items()}


def compare_camera(got, want, tag):
    """One camera's eye / at / up gradients under the stated tolerance.  An entry the loss cannot reach but through
    rounding -- camera2['up'] of the reverse layer: row 2 of the matrix is unit(eye - at) -- has a gradient of fp64
    rounding noise in the restatement and in the layer alike (some 1e-16 of the camera's largest gradient), which no
    relative comparison can hold to; such an entry, below 1e-9 of the camera's largest, must be as small here."""
    top = max(np.abs(w).max() for w in want.values())
    live = {k: w for k, w in want.items() if top == 0 or np.abs(w).max() > 1e-9 * top}
    compare_grads({k: got[k] for k in live}, live, tag, nonzero=False)
    for k in set(want) - set(live):
        assert got[k].shape == want[k].shape and np.abs(got[k]).max() <= 1e-9 * top, (tag, k)


def _backward(res, c, shape, only=None):
    loss = sum((res[k].reshape(*shape, -1) * torch.tensor(g, device=DEV).reshape(*shape, -1)).sum()
               for k, g in c["upstream"].items() if only is None or k == only)
    if loss.requires_grad:
        loss.backward()
    torch.cuda.synchronize()


def lift(c, cameras=None, wrt=("depth",), camera_grad=True):
    """(values, gradients, camera gradients) of a lift case; `cameras`: {'camera': the camera to call with}."""
    from surf_renderer_amd import depth_to_surfels
    cameras = cameras or {"camera": leaves(c["camera"])}
    B, H, W = c["shape"]
    d = torch.tensor(c["depth"], device=DEV, requires_grad="depth" in wrt)
    kw = {"camera_grad": True} if camera_grad else {}
    pos = depth_to_surfels(d, cameras["camera"], frame=c["frame"], **kw)
    _backward({"pos": pos}, c, (B, H * W))
    return {"pos": to_np(pos)}, {"depth": to_np(d.grad)}, camera_grads(cameras)


def project(c, cameras=None, wrt=po.INPUTS, camera_grad=True):
    from surf_renderer_amd import projection_renderer_differentiable_fast
    cameras = cameras or {"camera": leaves(c["camera"])}
    B, H, W, D = c["shape"]
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=k in wrt) for k in po.INPUTS if c[k] is not None}
    kw = {"camera_grad": True} if camera_grad else {}
    out, proj_out = projection_renderer_differentiable_fast(x["surfels"], x["rgb"], cameras["camera"],
                                                            x.get("rotated_image"), blur_size=c["blur_size"],
                                                            **c["flags"], **kw)
    res = dict(proj_out, out=out)
    _backward(res, c, (B, H, W))
    return ({k: to_np(v).reshape(B, H, W, -1) for k, v in res.items()}, {k: to_np(t.grad) for k, t in x.items()},
            camera_grads(cameras))


def reverse(c, cameras=None, wrt=None, camera_grad=True):
    from surf_renderer_amd import projection_reverse_renderer
    cameras = cameras or {"camera1": leaves(c["camera1"]), "camera2": leaves(c["camera2"])}
    wrt = c["wrt"] if wrt is None else wrt
    B, H, W, D = c["shape"]
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=k in wrt) for k in ro.INPUTS if c[k] is not None}
    kw = {"camera_grad": True} if camera_grad else {}
    out, proj_out = projection_reverse_renderer(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], cameras["camera1"],
                                                cameras["camera2"], rotated_image=x.get("rotated_image"), **c["flags"],
                                                **kw)
    res = dict(proj_out, out=out)
    _backward(res, c, (B, H, W), c["only"])
    return ({k: to_np(v) for k, v in res.items()}, {k: to_np(t.grad) for k, t in x.items()}, camera_grads(cameras))


@functools.lru_cache(maxsize=None)
def expected(layer, name, variant=None):
    """(values, gradients, camera gradients) of a case from the fp64 restatement with camera leaves, computed once."""
    if layer == "lift":
        c = sc.case(name, variant)
        return co.lift_gradients({"depth": c["depth"]}, c["camera"], c["upstream"], c["frame"])
    if layer == "projection":
        c = pc.case(name, variant)
        return co.project_gradients(pc.inputs(c), c["camera"], c["upstream"], c["blur_size"], **c["flags"])
    c = rc.case(name, variant)
    ups = c["upstream"] if c["only"] is None else {c["only"]: c["upstream"][c["only"]]}
    return co.reverse_gradients(rc.inputs(c), c["camera1"], c["camera2"], ups, wrt=c["wrt"], **c["flags"])


LAYERS = {"lift": (sc, lift, ("depth",), ("camera",)), "projection": (pc, project, po.INPUTS, ("camera",)),
          "reverse": (rc, reverse, ro.INPUTS, ("camera1", "camera2"))}
EVERY = [(layer, n, v) for layer, (m, *_) in LAYERS.items() for n, v in m.ALL]
# a batched case and the one whose finish kernel adds more than one partial, per layer
REDUCTIONS = [(layer, n) for layer in LAYERS for n in ("12x16", "17x9", "36x48")]


def _detached(layer, c):
    """(values, gradients) of the same call without the keyword and with the camera as data."""
    cases, run, inputs, labels = LAYERS[layer]
    return run(c, cameras={k: c[k] for k in labels}, camera_grad=False)[:2]


@pytest.mark.parametrize("layer,name,variant", EVERY)
def test_camera_gradients_match_the_restatement(layer, name, variant):
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case(name, variant)
    tag = f"{layer} {cases.tag(name, variant)}"
    got, got_g, got_cam = run(c)
    want, want_g, want_cam = expected(layer, name, variant)
    compare_values(got, want, tag, exact=("mask",) if layer == "reverse" else ())
    compare_grads({k: g for k, g in got_g.items() if k in want_g}, want_g, tag, nonzero=False)
    for label in labels:
        if layer == "lift" and c["frame"] == "camera":        # does not depend on eye / at / up
            assert all(g is None for g in got_cam[label].values()), tag
            continue
        for k in co.CAMERA_KEYS:
            assert got_cam[label][k].shape == np.asarray(c[label][k]).shape, (tag, label, k)
        # a camera the loss cannot reach (camera2 without a new depth, a loss on the mask) gets exact zeros
        compare_camera(got_cam[label], want_cam[label], f"{tag} {label}")
    if variant is None and layer != "reverse":
        assert all(np.abs(g).max() > 0 for g in want_cam[labels[0]].values()), tag


@pytest.mark.parametrize("layer,name", REDUCTIONS)
def test_outputs_and_the_other_gradients_are_bit_identical_to_the_detached_call(layer, name):
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case(name)
    assert_bit_identical(_detached(layer, c), run(c)[:2])


@pytest.mark.parametrize("layer,name", REDUCTIONS)
def test_two_runs_are_bit_identical_in_the_camera_gradients(layer, name):
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case(name)
    a, b = run(c)[2], run(c)[2]
    for label in labels:
        assert_bit_identical((a[label],), (b[label],))


@pytest.mark.parametrize("layer,name", [(layer, n) for layer in LAYERS for n in ("12x16", "17x9")])
def test_a_batch_equals_its_views_bit_for_bit_in_the_camera_gradients(layer, name):
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case(name)
    whole = run(c)[2]
    for b in range(c["shape"][0]):
        if layer == "lift":
            one = dict(c, depth=c["depth"][b:b + 1], shape=(1, *c["shape"][1:]),
                       upstream={"pos": c["upstream"]["pos"][b:b + 1]},
                       camera=dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in co.CAMERA_KEYS}))
        else:
            one = one_view(c, b, inputs, labels)
        alone = run(one)[2]
        for label in labels:
            assert_bit_identical((whole[label],), (alone[label],), slice(b, b + 1))


@pytest.mark.parametrize("layer,name", [(layer, "36x48") for layer in LAYERS])
def test_the_finish_across_workgroups_is_the_sum_of_the_parts(layer, name):
    """36x48 is seven workgroups per view.  The case's camera gradient is compared above; here the same views stacked
    twice must give each copy the bits of the single view (the view is grid dimension y, the order depends on N only)."""
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case(name)
    twice = dict(c, shape=(2, *c["shape"][1:]), upstream={k: np.concatenate((u, u)) for k, u in c["upstream"].items()},
                 **{k: (np.concatenate((c[k], c[k])) if c[k] is not None else None) for k in inputs},
                 **{label: dict(c[label], **{k: np.concatenate((c[label][k], c[label][k])) for k in co.CAMERA_KEYS})
                    for label in labels})
    one, two = run(c)[2], run(twice)[2]
    for label in labels:
        for b in (0, 1):
            assert_bit_identical((two[label],), (one[label],), slice(b, b + 1))


@pytest.mark.parametrize("layer", list(LAYERS))
def test_camera_only(layer):
    """Nothing else requires grad: the others' .grad stays None, and the camera gradient has the bits it has with them."""
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case("36x48")
    got, got_g, got_cam = run(c, wrt=())
    assert all(g is None for g in got_g.values())
    full = run(c)
    assert_bit_identical((got,), (full[0],))
    for label in labels:
        assert_bit_identical((got_cam[label],), (full[2][label],))


def test_one_tensor_in_both_cameras_gets_the_sum():
    c = rc.case("12x16")
    # camera2 with camera1's eye: first as two leaves of the same value, then as one leaf
    c2 = dict(c, camera2=dict(c["camera2"], eye=c["camera1"]["eye"]))
    separate = reverse(c2, cameras={"camera1": leaves(c2["camera1"]), "camera2": leaves(c2["camera2"])})[2]
    shared = leaves(c2["camera1"])
    both = {"camera1": shared, "camera2": dict(leaves(c2["camera2"]), eye=shared["eye"])}
    got = reverse(c2, cameras=both)[2]
    want = separate["camera1"]["eye"].astype(np.float32) + separate["camera2"]["eye"].astype(np.float32)
    assert np.abs(separate["camera2"]["eye"]).max() > 0
    assert np.array_equal(got["camera1"]["eye"].astype(np.float32), want)
    for k in ("at", "up"):
        assert np.array_equal(got["camera1"][k], separate["camera1"][k])
        assert np.array_equal(got["camera2"][k], separate["camera2"][k])


@pytest.mark.parametrize("layer", ["lift", "projection"])
def test_a_leaf_expanded_over_the_batch_gets_the_sum_over_views(layer):
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case("12x16")
    B = c["shape"][0]
    same = dict(c, camera=dict(c["camera"], **{k: np.repeat(c["camera"][k][:1], B, axis=0) for k in co.CAMERA_KEYS}))
    per_view = run(same)[2]["camera"]
    leaf = {k: torch.tensor(c["camera"][k][:1], device=DEV, requires_grad=True) for k in co.CAMERA_KEYS}
    run(same, cameras={"camera": dict(c["camera"], **{k: t.expand(B, -1) for k, t in leaf.items()})})
    for k in co.CAMERA_KEYS:
        assert leaf[k].grad.shape == (1, 3)
        want = per_view[k].sum(0, keepdims=True)
        np.testing.assert_allclose(to_np(leaf[k].grad), want, rtol=2e-6, atol=2e-7 * np.abs(per_view[k]).max(), err_msg=k)


@pytest.mark.parametrize("layer", list(LAYERS))
def test_fp64_and_cpu_camera_leaves_get_their_gradient_in_their_own_dtype_and_device(layer):
    cases, run, inputs, labels = LAYERS[layer]
    c = cases.case("12x16")
    want_cam = expected(layer, "12x16")[2]
    for dtype, device in ((torch.float64, DEV), (torch.float64, "cpu"), (torch.float32, "cpu")):
        cams = {label: leaves(c[label], dtype, device) for label in labels}
        got_cam = run(c, cameras=cams)[2]
        for label in labels:
            for k in co.CAMERA_KEYS:
                g = cams[label][k].grad
                assert g.dtype == dtype and g.device.type == torch.device(device).type and g.shape == cams[label][k].shape
            compare_camera(got_cam[label], want_cam[label], f"{layer} {label} {dtype} {device}")


def test_the_camera_frame_leaves_the_camera_without_a_gradient():
    c = sc.case("12x16", "camera")
    cams = {"camera": leaves(c["camera"])}
    got, got_g, got_cam = lift(c, cameras=cams)
    assert all(cams["camera"][k].grad is None for k in co.CAMERA_KEYS)
    assert_bit_identical(_detached("lift", c), (got, got_g))


@pytest.mark.parametrize("name", ["3x5", "36x48"])
def test_a_lift_with_depths_at_or_below_zero_still_sends_the_sum_of_g_to_the_eye(name):
    """P_wc = R P_cc + eye: d loss / d eye through column 3 alone is sum_q g_P, dead pixels included.  With every depth
    <= 0 every point is the eye, R carries nothing, and the eye's gradient is exactly that sum."""
    c = sc.case(name)
    assert (c["depth"] <= 0).any()
    got_cam = lift(c)[2]["camera"]
    compare_grads(got_cam, expected("lift", name)[2]["camera"], f"lift {name}")
    dead = dict(c, depth=-np.abs(c["depth"]) - (c["depth"] == 0))
    cam = lift(dead)[2]["camera"]
    want = c["upstream"]["pos"].astype(np.float64).sum(1)
    np.testing.assert_allclose(cam["eye"][:, :3], want, rtol=2e-6, atol=2e-7 * np.abs(want).max())
    assert np.all(cam["at"] == 0) and np.all(cam["up"] == 0)


def test_more_partials_than_the_finish_kernel_has_rows():
    """132 x 128, B = 2: N = 16896 is 66 workgroups per view, so two of the finish kernel's 64 rows add a second partial
    before the tree -- the only place that loop runs twice (36x48 has seven workgroups).  A lift: its restatement is
    cheap at this size.  One depth in sixteen is <= 0."""
    B, H, W = 2, 132, 128
    rng = np.random.RandomState(7100)
    eye, at, up = pc.draw_camera(rng, B)
    depth = rng.uniform(1.5, 3.0, (B, H * W))
    depth[:, ::16] = -depth[:, ::16] * (np.arange(depth[:, ::16].shape[1]) % 2)
    c = {"depth": pc.f32(depth), "frame": "world", "shape": (B, H, W),
         "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY),
                    "focal_length": pc.FOCAL},
         "upstream": {"pos": pc.f32(rng.uniform(-1, 1, (B, H * W, 3)))}}
    want, want_g, want_cam = co.lift_gradients({"depth": c["depth"]}, c["camera"], c["upstream"])
    got, got_g, got_cam = lift(c)
    compare_values(got, want, "lift 132x128")
    compare_grads(got_g, want_g, "lift 132x128")
    compare_camera(got_cam["camera"], want_cam["camera"], "lift 132x128 camera")
    assert_bit_identical(_detached("lift", c), (got, got_g))
    again = lift(c)[2]
    assert_bit_identical((got_cam["camera"],), (again["camera"],))
    for b in range(B):
        one = dict(c, depth=c["depth"][b:b + 1], shape=(1, H, W), upstream={"pos": c["upstream"]["pos"][b:b + 1]},
                   camera=dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in co.CAMERA_KEYS}))
        assert_bit_identical((got_cam["camera"],), (lift(one)[2]["camera"],), slice(b, b + 1))


def test_the_chain_from_a_depth_map_through_two_cameras():
    """depth -> depth_to_surfels(camA) -> projection_renderer_differentiable_fast(camB) -> weighted sum of out, at 12x16
    with B = 2: the gradients of depth, camA and camB against the composed restatement."""
    from surf_renderer_amd import depth_to_surfels, projection_renderer_differentiable_fast
    cl, cp = sc.case("12x16"), pc.case("12x16")
    B, H, W, D = cp["shape"]
    depth = np.abs(cl["depth"]) + (cl["depth"] == 0) * 2.0          # every point in front of camera A
    want, want_g, want_cam = co.chain_gradients(depth, cp["rgb"], cl["camera"], cp["camera"], cp["upstream"]["out"],
                                                cp["blur_size"])
    assert po.decision_margin(co.lift(torch.as_tensor(depth.astype(np.float64)), cl["camera"]).numpy(), cp["rgb"],
                              cp["camera"], None, cp["blur_size"]) >= 1.0
    cam_a, cam_b = leaves(cl["camera"]), leaves(cp["camera"])
    d = torch.tensor(depth, device=DEV, requires_grad=True)
    rgb = torch.tensor(cp["rgb"], device=DEV, requires_grad=True)
    pos = depth_to_surfels(d, cam_a, camera_grad=True)
    out, _ = projection_renderer_differentiable_fast(pos, rgb, cam_b, blur_size=cp["blur_size"], camera_grad=True)
    (out * torch.tensor(cp["upstream"]["out"], device=DEV)).sum().backward()
    torch.cuda.synchronize()
    got_cam = camera_grads({"camera_a": cam_a, "camera_b": cam_b})
    for label in ("camera_a", "camera_b"):
        compare_camera(got_cam[label], want_cam[label], f"chain {label}")
    # (the restatement rounds the surfels between the two layers to fp32, as the layers hand them on)
    compare_grads({"rgb": to_np(rgb.grad)}, {"rgb": want_g["rgb"]}, "chain")
    compare_grads({"depth": to_np(d.grad)}, {"depth": want_g["depth"]}, "chain")
