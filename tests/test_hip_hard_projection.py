"""GPU: projection_renderer (srh_hard_projection_keys / _fwd / _bwd) against the fp64 restatement tests/
hard_projection_oracle.py on the same fp32 inputs; tests/test_hard_projection_oracle_cpu.py ties that to the reference's
own function (tests/golden/hard_projection/hp1_*.npz) and asserts that no seeded surfel sits near a rounding tie, so the
mask and the counts are compared exactly and no element is left out of any comparison here.

Stated tolerances: the kernels sum in fp64 in ascending surfel index and store fp32, so every mean and every gradient
entry is held to its own bound |got - ref| <= 2^-24 |ref| + 2^-40 A + 2^-149, A = (sum of |v|) / count for a mean and
|g_out| / count for a gradient entry (tests/entry_checks.py, hard_projection_oracle.magnitudes).  A float32 sum of a
pixel's surfels does not meet that bound where many land on one pixel; the gradient is one division, correctly rounded
in either precision, so no bound tells the two apart there (tests/test_entry_checks_cpu.py).  The older array-scale
comparison stays beside it: rtol 2e-6 with atol 2e-7 max(|want|, 1) for values and 2e-7 max|want| for the gradient
(projection_checks)."""
import numpy as np
import pytest
import torch

import entry_checks as ec
import hard_projection_cases as cases
import hard_projection_oracle as ho
from entry_checks import to_np
from projection_checks import assert_bit_identical, compare_grads, compare_values, one_view

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hip(c, wrt=("rgb",)):
    """({'out', 'mask'}, {input: gradient or None}) of a case from the GPU."""
    from surf_renderer_amd import projection_renderer
    x = {k: torch.tensor(c[k], device=DEV, requires_grad=k in wrt) for k in ho.INPUTS}
    out, mask = projection_renderer(x["surfels"], x["rgb"], c["camera"])
    assert out.shape == mask.shape == c["rgb"].shape and out.dtype == torch.float32 and mask.dtype == torch.bool
    assert out.device.type == "cuda" and mask.device.type == "cuda" and not mask.requires_grad
    if wrt:
        (out * torch.tensor(c["upstream"]["out"], device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return {"out": to_np(out), "mask": mask.cpu().numpy()}, {k: to_np(t.grad) for k, t in x.items()}


def _compare_values(got, want, tag, A=None):
    """`A`: the restatement's magnitudes of `out` (None: those of the seeded case `tag` names)."""
    ec.check_all({"out": got["out"]}, {"out": want["out"]}, A or cases.magnitudes(tag.split()[0])[0], tag + " values")
    compare_values({"out": got["out"]}, {"out": want["out"]}, tag)
    assert got["mask"].dtype == np.bool_ and np.array_equal(got["mask"], want["mask"]), tag      # a decision: exact


def _given(pair):
    """(values, the gradients that are there): the surfels' is None by design."""
    return pair[0], {k: g for k, g in pair[1].items() if g is not None}


def _counts(c):
    """The kernel's own counts [B, N], which the public call keeps to itself."""
    from surf_renderer_amd import _lib, hard_projection as hp
    from surf_renderer_amd._projection import flat, upload_view
    surfels, rgb, (B, H, W, D), view, fovy, focal = hp._validate(torch.tensor(c["surfels"]), torch.tensor(c["rgb"]),
                                                                  c["camera"])
    pos, val = flat((surfels, rgb), B, H * W, torch.device(DEV))
    params = _lib.SrhHardProjectionParams(n_views=B, width=W, height=H, channels=D, fovy=fovy, focal_length=focal)
    _, mask, count = hp._HardFunction.apply(params, upload_view(view, torch.device(DEV)), pos, val)
    assert np.array_equal(mask.cpu().numpy(), count.cpu().numpy() == 0)
    return count.cpu().numpy()


@pytest.mark.parametrize("name", cases.NAMES)
def test_values_mask_counts_and_gradients_match_the_restatement(name):
    c = cases.case(name)
    got, got_g = _hip(c)
    want, want_g = cases.expected(name)
    _compare_values(got, want, name)
    assert np.array_equal(_counts(c), want["count"])
    ec.check_all(got_g, want_g, cases.magnitudes(name)[1], name + " gradients")
    compare_grads({"rgb": got_g["rgb"]}, want_g, name)
    assert got_g["surfels"] is None
    dropped = want["index"] == want["index"].shape[1]
    assert np.all(got_g["rgb"].reshape(*dropped.shape, -1)[dropped] == 0)
    assert np.all(got["out"][got["mask"]] == 0)


def test_surfels_that_require_grad_get_none():
    c = cases.case("12x16")
    got, got_g = _hip(c, wrt=("surfels", "rgb"))
    assert got_g["surfels"] is None and got_g["rgb"] is not None
    _compare_values(got, cases.expected("12x16")[0], "12x16")
    got, got_g = _hip(c, wrt=())
    assert got_g["rgb"] is None


@pytest.mark.parametrize("name", ["cluster_8x8", "12x16", "36x48"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    assert_bit_identical(_given(_hip(c)), _given(_hip(c)))


@pytest.mark.parametrize("name", ["12x16", "17x9"])
def test_a_batch_equals_its_views_bit_for_bit(name):
    c = cases.case(name)
    whole = _hip(c)
    for b in range(c["shape"][0]):
        assert_bit_identical(_given(whole), _given(_hip(one_view(c, b, ho.INPUTS))), slice(b, b + 1))


def test_outputs_are_overwritten_not_accumulated(monkeypatch):
    """The kernels write every element: with torch.empty handing out NaN-filled buffers the results do not change."""
    c = cases.case("17x9")
    want = _hip(c)
    empty, empty_like = torch.empty, torch.empty_like

    def nan_filled(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(123)

    monkeypatch.setattr(torch, "empty", lambda *a, **k: nan_filled(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: nan_filled(empty_like(*a, **k)))
    assert_bit_identical(_given(want), _given(_hip(c)))


def test_the_gradient_goes_through_an_rgb_given_as_b_n_d_and_other_dtypes_and_devices():
    from surf_renderer_amd import projection_renderer
    c = cases.case("12x16")
    B, H, W, D = c["shape"]
    want, want_g = cases.expected("12x16")
    for leaf in (torch.tensor(c["rgb"].reshape(B, H * W, D), device=DEV, requires_grad=True),          # [B, N, D]
                 torch.tensor(c["rgb"].astype(np.float64), device=DEV, requires_grad=True),            # fp64 GPU leaf
                 torch.tensor(c["rgb"].astype(np.float64), requires_grad=True)):                       # fp64 CPU leaf
        surfels = torch.tensor(c["surfels"].astype(np.float64))                                       # fp64 on the CPU
        out, mask = projection_renderer(surfels, leaf, c["camera"])
        assert out.shape == mask.shape == leaf.shape and out.device.type == "cuda" and out.dtype == torch.float32
        (out * torch.tensor(c["upstream"]["out"], device=DEV).reshape(out.shape)).sum().backward()
        assert leaf.grad.dtype == leaf.dtype and leaf.grad.device == leaf.device and leaf.grad.shape == leaf.shape
        _compare_values({"out": to_np(out).reshape(B, H, W, D), "mask": mask.cpu().numpy().reshape(B, H, W, D)}, want,
                        "12x16 converted")
        ec.check_all({"rgb": ec.narrowed(to_np(leaf.grad)).reshape(B, H, W, D)}, want_g, cases.magnitudes("12x16")[1],
                     "12x16 converted gradients")
        compare_grads({"rgb": to_np(leaf.grad).reshape(B, H, W, D)}, want_g, "12x16 converted")
