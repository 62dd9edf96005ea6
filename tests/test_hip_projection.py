"""GPU: projection_renderer_differentiable_fast (srh_projection_keys / _fwd / _bwd) against the fp64 restatement tests/
projection_oracle.py on the same fp32 inputs; tests/test_projection_oracle_cpu.py ties that to the reference's own
function (tests/golden/projection/pr1_*.npz) and asserts that no seeded input sits on a kink, so no element is left out
of any comparison here.

Stated tolerances: the kernels compute the restatement's fp64 arithmetic, sum without float atomics and store fp32, so
values match to rtol 2e-6 with atol 2e-7 max(|want|, 1) and gradients to rtol 2e-6 with atol 2e-7 max|want| per input
array (the standing bound of tests/test_hip_regularizers.py)."""
import numpy as np
import pytest
import torch

import projection_cases as cases
import projection_oracle as po
from projection_checks import assert_bit_identical, compare_grads, compare_values, one_view, to_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hip(c, wrt=po.INPUTS, only=None):
    """({output: [B, H, W, .]}, {input: gradient or None}) of a case from the GPU; `only`: the loss reads one output."""
    from surf_renderer_amd import projection_renderer_differentiable_fast
    B, H, W, D = c["shape"]
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=k in wrt) for k in po.INPUTS if c[k] is not None}
    out, proj_out = projection_renderer_differentiable_fast(x["surfels"], x["rgb"], c["camera"], x.get("rotated_image"),
                                                            blur_size=c["blur_size"], **c["flags"])
    res = dict(proj_out, out=out)
    assert out.shape == x["rgb"].shape and res["image1"].shape == x["rgb"].shape
    assert res["mask"].shape == (*x["rgb"].shape[:-1], 1) and ("depth" in res) == bool(c["flags"].get("compute_new_depth"))
    assert all(v.dtype == torch.float32 and v.device.type == "cuda" for v in res.values())
    if wrt:
        sum((res[k].reshape(B, H, W, -1) * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()
            if only is None or k == only).backward()
    torch.cuda.synchronize()
    return {k: to_np(v).reshape(B, H, W, -1) for k, v in res.items()}, {k: to_np(t.grad) for k, t in x.items()}


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_values_and_gradients_match_the_restatement(name, variant):
    got, got_g = _hip(cases.case(name, variant))
    want, want_g = cases.expected(name, variant)
    compare_values(got, want, cases.tag(name, variant))
    compare_grads(got_g, want_g, cases.tag(name, variant))


@pytest.mark.parametrize("name", ["cluster_8x8", "12x16"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    assert_bit_identical(_hip(c), _hip(c))


@pytest.mark.parametrize("name", ["12x16", "17x9"])
def test_a_batch_equals_its_views_bit_for_bit(name):
    c = cases.case(name)
    whole = _hip(c)
    for b in range(c["shape"][0]):
        assert_bit_identical(whole, _hip(one_view(c, b, po.INPUTS)), slice(b, b + 1))


@pytest.mark.parametrize("wrt", [("surfels",), ("rgb",), ("rotated_image",), ("rgb", "rotated_image")])
def test_inputs_that_do_not_require_grad_get_none(wrt):
    got, got_g = _hip(cases.case("12x16"), wrt=wrt)
    want, want_g = cases.expected("12x16", wrt=wrt)
    compare_values(got, want, "12x16")
    for k in po.INPUTS:
        if k not in wrt:
            assert got_g[k] is None, k
    compare_grads({k: got_g[k] for k in wrt}, want_g, f"12x16 wrt {wrt}")


def test_no_input_requires_grad():
    got, got_g = _hip(cases.case("17x9"), wrt=())
    compare_values(got, cases.expected("17x9")[0], "17x9 forward only")
    assert all(g is None for g in got_g.values())


@pytest.mark.parametrize("only", ["depth", "mask", "image1", "out"])
def test_a_loss_on_one_output_alone_reaches_the_surfels(only):
    _, got_g = _hip(cases.case("12x16"), only=only)
    _, want_g = cases.expected("12x16", only=only)
    assert np.abs(want_g["surfels"]).max() > 0
    want_g = dict(want_g)
    if only != "out":                                   # only `out` reads the rotated image
        assert np.all(want_g.pop("rotated_image") == 0) and np.all(got_g["rotated_image"] == 0)
    if only in ("depth", "mask"):                       # neither reads the values
        assert np.all(want_g.pop("rgb") == 0) and np.all(got_g["rgb"] == 0)
    compare_grads(got_g, want_g, f"12x16 loss on {only}")


def test_other_dtypes_devices_and_layouts_are_converted_and_the_gradient_comes_back_in_the_leafs_own():
    from surf_renderer_amd import projection_renderer_differentiable_fast
    c = cases.case("12x16")
    B, H, W, D = c["shape"]
    surfels = torch.tensor(c["surfels"].astype(np.float64), device=DEV, requires_grad=True)            # fp64 leaf
    rgb_t = torch.tensor(np.ascontiguousarray(c["rgb"].transpose(0, 2, 1, 3)), device=DEV, requires_grad=True)
    rotated = torch.tensor(c["rotated_image"], requires_grad=True)                                     # CPU leaf
    camera = dict(c["camera"], eye=torch.tensor(c["camera"]["eye"], dtype=torch.float64),
                  at=torch.tensor(c["camera"]["at"], device=DEV))
    out, proj_out = projection_renderer_differentiable_fast(surfels, rgb_t.permute(0, 2, 1, 3), camera, rotated,
                                                            blur_size=c["blur_size"], **c["flags"])
    res = dict(proj_out, out=out)
    sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
    want, want_g = cases.expected("12x16")
    compare_values({k: to_np(v) for k, v in res.items()}, want, "12x16 converted")
    assert surfels.grad.dtype == torch.float64 and surfels.grad.shape == surfels.shape
    assert rgb_t.grad.shape == rgb_t.shape and rotated.grad.device.type == "cpu"
    compare_grads({"surfels": to_np(surfels.grad), "rgb": to_np(rgb_t.grad.permute(0, 2, 1, 3)),
                    "rotated_image": to_np(rotated.grad)}, want_g, "12x16 converted")


def test_end_to_end_from_the_renderer_to_a_second_view():
    """One step of the trainers' use: render a scene, lift its pixels to surfels (the `pos` output), re-project them with
    the rendered image into a second camera, and let a loss on `out` move the geometry the first render came from."""
    from grad_cases import gpu_leaf_scene, load, TCH_KEYS
    from surf_renderer_amd import projection_renderer_differentiable_fast, render
    _, scene, kw = load("n1_aux_grad_phong")
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
    res = render(leaf_scene, device=DEV, shading="torch", **kw)
    pos, image = res["pos"], res["image"]
    H, W = image.shape[:2]
    assert pos.requires_grad and pos.shape == (H, W, 3)
    pos.retain_grad()
    image.retain_grad()
    cam = scene["camera"]
    second = {"eye": np.asarray(cam["eye"], dtype=np.float32)[None, :3] + np.float32([[0.35, 0.15, 0.0]]),
              "at": np.asarray(cam["at"], dtype=np.float32)[None, :3], "up": np.asarray(cam["up"], dtype=np.float32)[None, :3],
              "viewport": [0, 0, W, H], "fovy": float(cam["fovy"]), "focal_length": float(cam["focal_length"])}
    out, proj_out = projection_renderer_differentiable_fast(pos.reshape(1, H * W, 3), image[None], second)
    assert float(proj_out["mask"].detach().max()) > 0.1                        # the second camera still sees the scene
    upstream = np.random.RandomState(5).uniform(-1, 1, (1, H, W, 3)).astype(np.float32)
    (out * torch.tensor(upstream, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    # the depth leaves `pos` was computed from: every object's geometry
    geometry = {k: t.grad for k, t in leaves.items() if k not in TCH_KEYS}
    assert geometry and all(g is not None and bool(torch.isfinite(g).all()) for g in geometry.values())
    assert any(float(g.abs().max()) > 0 for g in geometry.values())
    # the oracle fed the same surfels and values
    want, want_g = po.gradients({"surfels": to_np(pos).reshape(1, H * W, 3), "rgb": to_np(image)[None], "rotated_image": None},
                                second, {"out": upstream})
    compare_values({"out": to_np(out)}, {"out": want["out"]}, "e2e")
    compare_grads({"surfels": to_np(pos.grad).reshape(1, H * W, 3), "rgb": to_np(image.grad)[None]}, want_g, "e2e")
