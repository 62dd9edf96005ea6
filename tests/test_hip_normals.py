"""GPU: the plane-fit layer (srh_normals_fwd / _bwd) against the fp64 restatement tests/normals_oracle.py on the same fp32
inputs, and against the reference's own float32 record (tests/golden/normals/nm1_*.npz); tests/test_normals_oracle_cpu.py
ties the restatement to the reference's float64 record.

Stated tolerance: the kernels compute the restatement's fp64 arithmetic and store fp32 once, so every element of the
normals and of pos.grad is held to |got - ref| <= 2^-24 |ref| + NORMALS_C64 max|ref| + 2^-149 (entry_checks.
check_plane_fit: the fit's determinant cancels, so the scale is the array's largest entry and the coefficient is the one
measured on the device, capped at 2^-36; an entry on which the restatement's two summation orders disagree by a quarter
of the cap keeps the array-scale tolerance, and the seeded cases have none).  The same arithmetic in float32 does not
meet that bound (tests/test_entry_checks_cpu.py).  The older comparison stays beside it: rtol 2e-6 with atol 2e-7
max(|want|, 1) for normals and 2e-7 max|want| for pos.grad (projection_checks).  The reference's float32 record is
compared under those older figures only; it is itself within 0.64 of them from its float64 record."""
import os

import numpy as np
import pytest
import torch

import entry_checks as ec
import normals_cases as cases
from conftest import GOLDEN_DIR
from entry_checks import to_np
from projection_checks import assert_bit_identical, compare_grads, compare_values, one_view

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hip(c, pos=None, wrt=True, camera=True):
    """({'normal': like pos}, {'pos': gradient or None}) of a case from the GPU."""
    from surf_renderer_amd import estimate_surface_normals_plane_fit_batched as fit
    p = torch.tensor(c["pos"], device=DEV, requires_grad=wrt) if pos is None else pos
    n = fit(p, c["camera"] if camera else None, frame=c["frame"])
    assert n.shape == p.shape and n.dtype == torch.float32 and n.device.type == "cuda"
    if p.requires_grad:
        (n * torch.tensor(c["upstream"]["normal"], device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return {"normal": to_np(n)}, {"pos": to_np(p.grad) if p.is_leaf else None}


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_values_and_gradients_match_the_restatement_and_the_float32_reference(name, variant):
    c = cases.case(name, variant)
    got, got_g = _hip(c)
    want, want_g = cases.expected(name, variant)
    again, again_g = cases.turned(name, variant)
    ec.check_plane_fit(got["normal"], want["normal"], again["normal"], cases.tag(name, variant) + " normal")
    ec.check_plane_fit(got_g["pos"], want_g["pos"], again_g["pos"], cases.tag(name, variant) + " grad pos")
    compare_values(got, want, cases.tag(name, variant))
    compare_grads(got_g, want_g, cases.tag(name, variant))
    npz = np.load(os.path.join(GOLDEN_DIR, "normals", "nm1_" + cases.tag(name, variant) + ".npz"), allow_pickle=False)
    compare_values(got, {"normal": npz["ref32/normal"].astype(np.float64)}, cases.tag(name, variant) + " ref32")
    compare_grads(got_g, {"pos": npz["ref32/grad/pos"].astype(np.float64)}, cases.tag(name, variant) + " ref32")
    if name in cases.UNSEEN_ROWS:
        r0, r1 = cases.UNSEEN_ROWS[name]
        assert np.all(got_g["pos"][:, r0 + 1:r1 - 1] == 0)


def test_pos_that_does_not_require_grad_gets_no_gradient_no_buffer_and_no_backward_launch(monkeypatch):
    from surf_renderer_amd import _layer, normals
    calls = []
    for helper in ("scratch", "grad_buffers"):      # the backward's buffers: asked for only when it launches
        monkeypatch.setattr(normals, helper, lambda *a, _f=getattr(_layer, helper), **k: calls.append(_f) or _f(*a, **k))
    got, got_g = _hip(cases.case("17x9"), wrt=False)
    ec.check_plane_fit(got["normal"], cases.expected("17x9")[0]["normal"], cases.turned("17x9")[0]["normal"], "17x9 forward only")
    compare_values(got, cases.expected("17x9")[0], "17x9 forward only")
    assert got_g["pos"] is None and not calls
    _hip(cases.case("3x5"))
    assert calls == [_layer.grad_buffers, _layer.scratch]


@pytest.mark.parametrize("name", ["12x16", "36x48"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    assert_bit_identical(_hip(c), _hip(c))


@pytest.mark.parametrize("name", ["12x16", "17x9"])
def test_a_view_alone_equals_the_view_in_its_batch_bit_for_bit(name):
    c = cases.case(name)
    whole = _hip(c)
    for b in range(c["shape"][0]):
        assert_bit_identical(whole, _hip(one_view(c, b, ("pos",))), slice(b, b + 1))


def test_the_unbatched_entry_points_equal_the_batched_one_at_one_view_bit_for_bit():
    from surf_renderer_amd import estimate_surface_normals, estimate_surface_normals_plane_fit
    c = cases.case(cases.UNBATCHED)
    want = _hip(c)
    up = torch.tensor(c["upstream"]["normal"][0], device=DEV)
    for call in (lambda p: estimate_surface_normals_plane_fit(p, 3), lambda p: estimate_surface_normals_plane_fit(p),
                 lambda p: estimate_surface_normals(p, kernel_size=5, method="plane")):
        p = torch.tensor(c["pos"][0], device=DEV, requires_grad=True)
        n = call(p)
        assert n.shape == p.shape
        (n * up).sum().backward()
        assert_bit_identical(want, ({"normal": to_np(n)[None]}, {"pos": to_np(p.grad)[None]}))


def test_flat_points_equal_the_grid_bit_for_bit_and_the_gradient_has_their_shape():
    c, f = cases.case("12x16"), cases.case("12x16", "flat")
    grid = _hip(c)
    p = torch.tensor(f["pos"], device=DEV, requires_grad=True)
    flat = _hip(f, pos=p)
    assert p.grad.shape == f["pos"].shape
    assert_bit_identical(grid, tuple({k: v.reshape(c["pos"].shape) for k, v in d.items()} for d in flat))
    assert_bit_identical(grid, _hip(c, camera=False))            # a grid in the camera frame needs no camera


def test_a_float64_leaf_that_is_not_contiguous_gets_its_gradient_in_its_own_dtype_and_layout():
    c = cases.case("12x16")
    want, want_g = cases.expected("12x16")
    for leaf in (torch.tensor(np.ascontiguousarray(c["pos"].astype(np.float64).transpose(0, 2, 1, 3)), device=DEV,
                              requires_grad=True),                                                   # fp64, GPU
                 torch.tensor(np.ascontiguousarray(c["pos"].astype(np.float64).transpose(0, 2, 1, 3)),
                              requires_grad=True)):                                                  # fp64, CPU
        p = leaf.permute(0, 2, 1, 3)
        assert not p.is_contiguous()
        got = _hip(c, pos=p)
        assert leaf.grad.dtype == torch.float64 and leaf.grad.device == leaf.device and leaf.grad.shape == leaf.shape
        assert leaf.grad.stride() == leaf.stride()
        again, again_g = cases.turned("12x16")
        ec.check_plane_fit(got[0]["normal"], want["normal"], again["normal"], "12x16 converted normal")
        ec.check_plane_fit(ec.narrowed(to_np(leaf.grad.permute(0, 2, 1, 3))), want_g["pos"], again_g["pos"], "12x16 converted grad pos")
        compare_values(got[0], want, "12x16 converted")
        compare_grads({"pos": to_np(leaf.grad.permute(0, 2, 1, 3))}, want_g, "12x16 converted")


def test_backward_overwrites_every_element_of_a_buffer_filled_through_the_c_abi():
    """srh_normals_bwd on a grad_pos and a workspace pre-filled with a sentinel (NaN): no element keeps it, and the result
    is the layer's, bit for bit."""
    from surf_renderer_amd import _lib
    lib = _lib.load()
    c = cases.case("36x48")
    B, H, W = c["shape"]
    want = _hip(c)
    pos = torch.tensor(c["pos"], device=DEV)
    up = torch.tensor(c["upstream"]["normal"], device=DEV)
    out = torch.full_like(pos, float("nan"))
    grad = torch.full_like(pos, float("nan"))
    n_bytes = lib.srh_normals_workspace_bytes(B, W, H)
    ws = torch.full((n_bytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.srh_normals_fwd(B, W, H, None, pos.data_ptr(), out.data_ptr(), st))
    _lib.check(lib.srh_normals_bwd(B, W, H, None, pos.data_ptr(), up.data_ptr(), ws.data_ptr(), n_bytes, grad.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.isfinite(ws).all()
    assert_bit_identical(want, ({"normal": to_np(out)}, {"pos": to_np(grad)}))
