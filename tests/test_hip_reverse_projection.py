"""GPU: projection_reverse_renderer (srh_reverse_projection_fwd / _keys / _bwd) against the fp64 restatement tests/
reverse_projection_oracle.py on the same fp32 inputs; tests/test_reverse_projection_oracle_cpu.py ties that to the
reference's own function (tests/golden/reverse_projection/rp1_*.npz) and asserts that no seeded input sits near a
decision, so the mask is compared exactly and no element is left out of any comparison here.

Stated tolerances: the kernels compute the restatement's fp64 arithmetic, sum without float atomics and store fp32, so
values match to rtol 2e-6 with atol 2e-7 max(|want|, 1) and gradients to rtol 2e-6 with atol 2e-7 max|want| per input
array (the bounds of tests/test_hip_projection.py for the same arithmetic regime)."""
import numpy as np
import pytest
import torch

import reverse_projection_cases as cases
import reverse_projection_oracle as ro
from projection_checks import assert_bit_identical, to_np
from projection_checks import compare_grads as _grads, compare_values as _values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _call(c, x, **more):
    from surf_renderer_amd import projection_reverse_renderer
    out, proj_out = projection_reverse_renderer(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], c["camera1"], c["camera2"],
                                                rotated_image=x.get("rotated_image"), **c["flags"], **more)
    res = dict(proj_out, out=out)
    B, H, W, D = c["shape"]
    assert out.shape == (B, H, W, D) and res["image1"].shape == (B, H, W, D) and res["mask"].shape == (B, H, W, 1)
    assert ("depth" in res) == bool(c["flags"]["compute_new_depth"])
    assert all(v.dtype == torch.float32 and v.device.type == "cuda" for v in res.values())
    return res


def _hip(c):
    """({output: [B, H, W, .]}, {input: gradient or None}) of a case from the GPU, under the case's `wrt` and `only`."""
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=k in c["wrt"]) for k in ro.INPUTS if c[k] is not None}
    res = _call(c, x)
    if c["wrt"]:
        sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()
            if c["only"] is None or k == c["only"]).backward()
    torch.cuda.synchronize()
    return {k: to_np(v) for k, v in res.items()}, {k: to_np(t.grad) for k, t in x.items()}


def _compare_values(got, want, tag):
    _values(got, want, tag, exact=("mask",))          # no seeded input sits near a decision: the mask is exact


def _compare_grads(got, want, tag):
    _grads(got, want, tag, nonzero=False)             # a variant's loss leaves some inputs out: their gradient is 0


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_values_and_gradients_match_the_restatement(name, variant):
    c = cases.case(name, variant)
    got, got_g = _hip(c)
    want, want_g = cases.expected(name, variant)
    _compare_values(got, want, cases.tag(name, variant))
    _compare_grads(got_g, want_g, cases.tag(name, variant))
    for k in ro.INPUTS:                              # an input that does not require grad gets None
        if c[k] is not None and k not in c["wrt"]:
            assert got_g[k] is None, k


def test_a_loss_on_the_mask_alone_gives_zero_gradients():
    _, got_g = _hip(cases.case("12x16", "only_mask"))
    for k in ro.INPUTS:
        assert got_g[k] is not None and np.all(got_g[k] == 0), k


def test_no_input_requires_grad():
    c = dict(cases.case("17x9"), wrt=())
    got, got_g = _hip(c)
    _compare_values(got, cases.expected("17x9")[0], "17x9 forward only")
    assert all(g is None for g in got_g.values())


@pytest.mark.parametrize("name", ["cluster_8x8", "12x16", "36x48"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    assert_bit_identical(_hip(c), _hip(c))


@pytest.mark.parametrize("name", ["12x16", "17x9"])
def test_a_batch_equals_its_views_bit_for_bit(name):
    c = cases.case(name)
    whole = _hip(c)
    for b in range(c["shape"][0]):
        assert_bit_identical(whole, _hip(cases.view(c, b)), slice(b, b + 1))


def test_mask_dropout_scales_the_kept_mask_and_follows_the_seed():
    c = cases.case("12x16")
    plain = cases.expected("12x16")[0]["mask"]
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        x = {k: torch.tensor(c[k], device=DEV, requires_grad=True) for k in ro.INPUTS}
        res = _call(c, x, mask_dropout=0.5)
        sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
        runs.append(({k: to_np(v) for k, v in res.items()}, {k: to_np(t.grad) for k, t in x.items()}))
    (v, g), (v2, g2) = runs
    mask = v["mask"]
    assert np.all(np.isin(mask, (0.0, 2.0))) and np.all(mask[plain == 0] == 0)
    assert (mask == 2).any() and (mask[plain == 1] == 0).any()
    # `out` from the returned tensors, in the fp32 the kernel stored them in
    want_out = mask * v["image1"] + (1 - mask) * c["rotated_image"].astype(np.float64)
    np.testing.assert_allclose(v["out"], want_out, rtol=2e-6, atol=2e-7 * max(np.abs(want_out).max(), 1.0))
    assert_bit_identical((v, g), (v2, g2))
    # and the whole call against the oracle handed the same keep plane
    keep = np.where(plain == 1, mask, 2.0)              # where the mask is 0 anyway the plane's value does not matter
    want, want_g = ro.gradients(cases.inputs(c), c["camera1"], c["camera2"], c["upstream"], keep=keep, **c["flags"])
    _compare_values(v, want, "12x16 dropout")
    _compare_grads(g, want_g, "12x16 dropout")


def test_other_dtypes_and_layouts_are_converted_and_the_gradient_comes_back_in_the_leafs_own():
    c = cases.case("12x16")
    rgb_t = torch.tensor(np.ascontiguousarray(c["rgb"].transpose(0, 2, 1, 3)), device=DEV, requires_grad=True)
    in_pos = torch.tensor(c["in_pos_wc"].astype(np.float64), device=DEV, requires_grad=True)            # fp64 leaf
    out_pos_t = torch.tensor(np.ascontiguousarray(c["out_pos_wc"].transpose(0, 2, 1)), device=DEV, requires_grad=True)
    rotated = torch.tensor(c["rotated_image"].astype(np.float64), requires_grad=True)                   # fp64 CPU leaf
    x = {"rgb": rgb_t.permute(0, 2, 1, 3), "in_pos_wc": in_pos, "out_pos_wc": out_pos_t.permute(0, 2, 1),
         "rotated_image": rotated}
    assert not x["rgb"].is_contiguous() and not x["out_pos_wc"].is_contiguous()
    camera1 = dict(c["camera1"], eye=torch.tensor(c["camera1"]["eye"], dtype=torch.float64),
                   at=torch.tensor(c["camera1"]["at"], device=DEV))
    res = _call(dict(c, camera1=camera1), x)
    sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
    want, want_g = cases.expected("12x16")
    _compare_values({k: to_np(v) for k, v in res.items()}, want, "12x16 converted")
    assert in_pos.grad.dtype == torch.float64 and rotated.grad.dtype == torch.float64
    assert rotated.grad.device.type == "cpu"
    assert rgb_t.grad.shape == rgb_t.shape and out_pos_t.grad.shape == out_pos_t.shape
    _compare_grads({"rgb": to_np(rgb_t.grad.permute(0, 2, 1, 3)), "in_pos_wc": to_np(in_pos.grad),
                    "out_pos_wc": to_np(out_pos_t.grad.permute(0, 2, 1)), "rotated_image": to_np(rotated.grad)}, want_g,
                   "12x16 converted")
