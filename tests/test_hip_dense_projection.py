"""GPU: projection_renderer_differentiable (srh_dense_projection_fwd / _bwd) against the fp64 restatement tests/
dense_projection_oracle.py on the same fp32 inputs; tests/test_dense_projection_oracle_cpu.py ties that to the
reference's own function (tests/golden/dense_projection/dp1_*.npz) and asserts that no seeded surfel sits near Z = 0,
the layer's one kink, so no element is left out of any comparison here.

Stated tolerances: the kernels compute the restatement's fp64 arithmetic (the weight as the product of its two
factors), sum without atomics and store fp32, so values match to rtol 2e-6 with atol 2e-7 max(|want|, 1) and gradients
to rtol 2e-6 with atol 2e-7 max|want| per input array (the standing bound of tests/test_hip_projection.py)."""
import numpy as np
import pytest
import torch

import dense_projection_cases as cases
import dense_projection_oracle as do
from projection_checks import assert_bit_identical, compare_grads, compare_values, one_view, to_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hip(c, wrt=do.INPUTS, only=None, no_grad=False):
    """({output: like the case's}, {input: gradient or None}) of a case from the GPU; `only`: the loss reads one output."""
    from surf_renderer_amd import projection_renderer_differentiable
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=k in wrt) for k in do.INPUTS if c[k] is not None}
    with torch.no_grad() if no_grad else torch.enable_grad():
        out, mask = projection_renderer_differentiable(x["surfels"], x["rgb"], c["camera"], x.get("rotated_image"),
                                                       blur_size=c["blur_size"])
    res = {"out": out, "mask": mask}
    assert out.shape == x["rgb"].shape and mask.shape == (*x["rgb"].shape[:-1], 1)
    assert all(v.dtype == torch.float32 and v.device.type == "cuda" for v in res.values())
    if wrt and not no_grad:
        sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()
            if only is None or k == only).backward()
    torch.cuda.synchronize()
    return {k: to_np(v) for k, v in res.items()}, {k: to_np(t.grad) for k, t in x.items()}


@pytest.mark.parametrize("frame,layout,rotated", cases.ALL)
def test_values_and_gradients_match_the_restatement(frame, layout, rotated):
    got, got_g = _hip(cases.case(frame, layout, rotated))
    want, want_g = cases.expected(frame, layout, rotated)
    compare_values(got, want, cases.tag(frame, layout, rotated))
    compare_grads(got_g, want_g, cases.tag(frame, layout, rotated))


@pytest.mark.parametrize("frame,rotated", [("35x37", False), ("12x16", True)])
def test_two_runs_are_bit_identical(frame, rotated):
    c = cases.case(frame, "grid", rotated)
    assert_bit_identical(_hip(c), _hip(c))


@pytest.mark.parametrize("frame,layout,rotated", [("17x9", "flat", False), ("36x48", "grid", True)])
def test_a_batch_equals_its_views_bit_for_bit(frame, layout, rotated):
    c = cases.case(frame, layout, rotated)
    whole = _hip(c)
    for b in range(c["shape"][0]):
        assert_bit_identical(whole, _hip(one_view(c, b, do.INPUTS)), slice(b, b + 1))


@pytest.mark.parametrize("wrt", [("surfels",), ("rgb",), ("rotated_image",), ("surfels", "rgb"), ("rgb", "rotated_image"),
                                 ("surfels", "rotated_image")])
def test_inputs_that_do_not_require_grad_get_none(wrt):
    got, got_g = _hip(cases.case("12x16", "grid", True), wrt=wrt)
    want, want_g = cases.expected("12x16", "grid", True, wrt=wrt)
    compare_values(got, want, "12x16")
    for k in do.INPUTS:
        if k not in wrt:
            assert got_g[k] is None, k
    compare_grads({k: got_g[k] for k in wrt}, want_g, f"12x16 wrt {wrt}")


def test_no_input_requires_grad_and_a_forward_under_no_grad():
    want = cases.expected("17x9")[0]
    got, got_g = _hip(cases.case("17x9"), wrt=())
    compare_values(got, want, "17x9 forward only")
    assert all(g is None for g in got_g.values())
    got, got_g = _hip(cases.case("17x9"), no_grad=True)
    compare_values(got, want, "17x9 under no_grad")
    assert all(g is None for g in got_g.values())


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("only", ["out", "mask"])
def test_a_loss_on_one_output_alone_reaches_the_surfels(only, rotated):
    _, got_g = _hip(cases.case("12x16", "grid", rotated), only=only)
    _, want_g = cases.expected("12x16", "grid", rotated, only=only)
    assert np.abs(want_g["surfels"]).max() > 0
    want_g = dict(want_g)
    if only == "mask":                                  # the mask reads neither the values nor the rotated image
        for k in ("rgb", "rotated_image")[:1 + rotated]:
            assert np.all(want_g.pop(k) == 0) and np.all(got_g[k] == 0)
    compare_grads(got_g, want_g, f"12x16 loss on {only}")


def test_other_dtypes_devices_and_layouts_are_converted_and_the_gradient_comes_back_in_the_leafs_own():
    from surf_renderer_amd import projection_renderer_differentiable
    c = cases.case("12x16", "grid", True)
    surfels = torch.tensor(c["surfels"].astype(np.float64), device=DEV, requires_grad=True)            # fp64 leaf
    rgb_t = torch.tensor(np.ascontiguousarray(c["rgb"].transpose(0, 2, 1, 3)), device=DEV, requires_grad=True)
    rotated = torch.tensor(c["rotated_image"], requires_grad=True)                                     # CPU leaf
    camera = dict(c["camera"], eye=torch.tensor(c["camera"]["eye"], dtype=torch.float64),
                  at=torch.tensor(c["camera"]["at"], device=DEV))
    out, mask = projection_renderer_differentiable(surfels, rgb_t.permute(0, 2, 1, 3), camera, rotated,
                                                   blur_size=c["blur_size"])
    res = {"out": out, "mask": mask}
    sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
    want, want_g = cases.expected("12x16", "grid", True)
    compare_values({k: to_np(v) for k, v in res.items()}, want, "12x16 converted")
    assert surfels.grad.dtype == torch.float64 and surfels.grad.shape == surfels.shape
    assert rgb_t.grad.shape == rgb_t.shape and rotated.grad.device.type == "cpu"
    compare_grads({"surfels": to_np(surfels.grad), "rgb": to_np(rgb_t.grad.permute(0, 2, 1, 3)),
                    "rotated_image": to_np(rotated.grad)}, want_g, "12x16 converted")


def test_the_two_layouts_of_one_image_differ_by_the_sigma_quirk():
    """sigma = blur_size * rgb.shape[-2] / 6: the same surfels and values give another image as [B, N, D] (sigma from
    N) than as [B, H, W, D] (sigma from W), and the flat call with blur_size scaled by W / N gives the grid's."""
    grid, flat = cases.case("3x5", "grid"), cases.case("3x5", "flat")
    B, H, W, D = grid["shape"]
    v_grid, _ = _hip(grid, wrt=())
    v_flat, _ = _hip(flat, wrt=())
    assert np.abs(v_flat["mask"].reshape(-1) - v_grid["mask"].reshape(-1)).max() > 0.1 * np.abs(v_grid["mask"]).max()
    # blur_size / H is not the same float as blur_size * W / N in general, so this is a comparison to the bound
    v_same, _ = _hip(dict(flat, blur_size=grid["blur_size"] * W / (H * W)), wrt=())
    compare_values({k: v.reshape(v_grid[k].shape) for k, v in v_same.items()}, cases.expected("3x5")[0], "3x5 flat, sigma of the grid")
