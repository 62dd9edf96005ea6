"""nearest_points, hausdorff and hausdorff_batched on the GPU against the reference's recorded hausdorff
(tests/golden/pointsets, float64) and the fp64 oracle (tests/pointsets_oracle.py) on the regular cases: values within one
float32 ulp, indices exact, every gradient entry within 2^-23 |ref| + 2^-40 S (tests/pointsets_checks.py derives both);
determinism, batch = views, [N, D] = B = 1, directed, squared, dtype and device of the gradients, and the autograd
plumbing of each output alone.  Run with -s for the worst measured ratios."""
import functools
import os

import numpy as np
import pytest
import torch

import pointsets_cases as cases
import pointsets_oracle as oracle
from conftest import GOLDEN_DIR
from pointsets_checks import DEV, check_grads, check_values, leaf, run, view_oracle

pytestmark = pytest.mark.gpu
ALL = range(len(cases.REGULAR))
# a few shapes for the properties that do not depend on the size: the ragged ones and the two-workgroup one
SOME = [1, 3, 5, 8]


@functools.lru_cache(maxsize=None)
def fixture(k):
    return dict(np.load(os.path.join(GOLDEN_DIR, "pointsets", "ps1_" + cases.tag(k) + ".npz")))


@functools.lru_cache(maxsize=None)
def truth(k, squared=False):
    """per view the oracle's values and its gradients under the case's g_u, g_v"""
    c = cases.regular(k)
    return [view_oracle(c["u"][b], c["v"][b], c["g_u"][b], c["g_v"][b], squared) for b in range(cases.VIEWS)]


@functools.lru_cache(maxsize=None)
def hausdorff_truth(k):
    """per view the oracle's gradients under the fixture's loss g . (sym, uv, vu)"""
    c, out = cases.regular(k), []
    for b in range(cases.VIEWS):
        r = oracle.nearest(c["u"][b], c["v"][b])
        g_u, g_v = oracle.hausdorff_upstreams(r, c["g"][b].astype(np.float64))
        out.append(oracle.gradients(c["u"][b], c["v"][b], r["idx_u"], r["idx_v"], g_u, g_v))
    return out


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_hausdorff_is_within_one_ulp_of_the_reference_and_its_gradients_within_their_bounds(k):
    from surf_renderer_amd import hausdorff, hausdorff_batched
    z, H = fixture(k), hausdorff_truth(k)
    u, v = leaf(z["in/u"]), leaf(z["in/v"])
    out = torch.stack(hausdorff_batched(u, v), dim=-1)                       # [B, 3]
    assert out.shape == (cases.VIEWS, 3) and out.dtype == torch.float32
    (out * torch.tensor(z["grad_in/g"], device=DEV)).sum().backward()
    worst_v = check_values(out.detach().cpu().numpy(), z["ref64/out"], "batched")
    worst_g = 0.0
    for b in range(cases.VIEWS):
        ub, vb = leaf(z["in/u"][b]), leaf(z["in/v"][b])
        one = torch.stack(hausdorff(ub, vb))
        assert one.shape == (3,) and torch.equal(one, out[b].detach())       # a batch equals its views
        (one * torch.tensor(z["grad_in/g"][b], device=DEV)).sum().backward()
        assert torch.equal(ub.grad, u.grad[b]) and torch.equal(vb.grad, v.grad[b])
        for side, t in (("u", u), ("v", v)):
            worst_g = max(worst_g, check_grads(t.grad[b].cpu().numpy(), z["ref64/grad/" + side][b], H[b]["S_" + side],
                                               f"view {b} grad_{side}"))
    print(f"{cases.tag(k)}: hausdorff values {worst_v:.3g} ulp; gradients {worst_g:.3g} of their bound")


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_nearest_points_has_the_oracles_indices_values_and_gradients(k):
    c, T = cases.regular(k), truth(k)
    got = run(c["u"], c["v"], c["g_u"], c["g_v"])
    assert got["idx_u"].dtype == np.int64 and got["dist_u"].dtype == np.float32
    worst_v = worst_g = 0.0
    for b in range(cases.VIEWS):
        for side in "uv":
            assert np.array_equal(got["idx_" + side][b], T[b]["idx_" + side]), (b, side)
            worst_v = max(worst_v, check_values(got["dist_" + side][b], T[b]["dist_" + side], f"view {b} dist_{side}"))
            worst_g = max(worst_g, check_grads(got["grad_" + side][b], T[b]["grad_" + side], T[b]["S_" + side],
                                               f"view {b} grad_{side}"))
    print(f"{cases.tag(k)}: dist {worst_v:.3g} ulp; gradients {worst_g:.3g} of their bound")


@pytest.mark.parametrize("k", [6, 7], ids=cases.tag)
def test_squared_and_directed_on_two_regular_shapes(k):
    c, T = cases.regular(k), truth(k, squared=True)
    full = run(c["u"], c["v"], c["g_u"], c["g_v"])
    sq = run(c["u"], c["v"], c["g_u"], c["g_v"], squared=True)
    for b in range(cases.VIEWS):
        for side in "uv":
            assert np.array_equal(sq["idx_" + side][b], T[b]["idx_" + side])
            check_values(sq["dist_" + side][b], T[b]["dist_" + side], "squared dist_" + side)
            check_grads(sq["grad_" + side][b], T[b]["grad_" + side], T[b]["S_" + side], "squared grad_" + side)
    # The square roots of the squared distances are the unsquared ones: the stored square is within 2^-24 relative of
    # d2, its fp64 root within 2^-25 of the distance, and one more rounding away: the same float32 or its neighbour.
    # Not always the same one, whatever the kernel does: with exact fp64 values (the oracle's) float32(sqrt(float32(d2)))
    # differs from float32(sqrt(d2)) by one ulp in 506 of 3846 entries of 257x1025x3 and 727 of 6000 of 1300x700x4.
    for side in "uv":
        check_values(full["dist_" + side], np.sqrt(sq["dist_" + side].astype(np.float64)), "sqrt of squared")
    # directed: the u side of the full call bit for bit, and the gradients of a loss on dist_u alone
    only_u = run(c["u"], c["v"], c["g_u"], None)
    di = run(c["u"], c["v"], c["g_u"], None, directed=True)
    assert di["dist_v"] is None and di["idx_v"] is None
    assert np.array_equal(di["dist_u"], full["dist_u"]) and np.array_equal(di["idx_u"], full["idx_u"])
    assert np.array_equal(di["grad_u"], only_u["grad_u"]) and np.array_equal(di["grad_v"], only_u["grad_v"])
    di_sq = run(c["u"], c["v"], c["g_u"], None, directed=True, squared=True)
    assert np.array_equal(di_sq["dist_u"], sq["dist_u"])


@pytest.mark.parametrize("k", SOME, ids=cases.tag)
def test_runs_are_bit_identical_and_a_batch_equals_its_views_and_a_single_view_equals_b_1(k):
    c = cases.regular(k)
    a, again = run(c["u"], c["v"], c["g_u"], c["g_v"]), run(c["u"], c["v"], c["g_u"], c["g_v"])
    for key in a:
        assert np.array_equal(a[key], again[key]), key
    for b in range(cases.VIEWS):
        one = run(c["u"][b], c["v"][b], c["g_u"][b], c["g_v"][b])                   # [N, D]
        b1 = run(c["u"][b:b + 1], c["v"][b:b + 1], c["g_u"][b:b + 1], c["g_v"][b:b + 1])
        for key in a:
            assert one[key].shape == a[key].shape[1:], key
            assert np.array_equal(one[key], a[key][b]) and np.array_equal(b1[key][0], a[key][b]), (key, b)


@pytest.mark.parametrize("k", SOME, ids=cases.tag)
def test_a_loss_on_each_output_alone_gives_the_oracles_gradients(k):
    from surf_renderer_amd import hausdorff_batched
    c, H = cases.regular(k), hausdorff_truth(k)
    for g_u, g_v in ((c["g_u"], None), (None, c["g_v"])):
        got = run(c["u"], c["v"], g_u, g_v)
        for b in range(cases.VIEWS):
            T = view_oracle(c["u"][b], c["v"][b], None if g_u is None else g_u[b], None if g_v is None else g_v[b])
            for side in "uv":
                check_grads(got["grad_" + side][b], T["grad_" + side], T["S_" + side], f"view {b} grad_{side}")
    u, v = leaf(c["u"]), leaf(c["v"])
    hausdorff_batched(u, v)[0].sum().backward()                              # sym alone
    for b in range(cases.VIEWS):
        r = oracle.nearest(c["u"][b], c["v"][b])
        g_u, g_v = oracle.hausdorff_upstreams(r, np.array([1.0, 0.0, 0.0]))
        T = oracle.gradients(c["u"][b], c["v"][b], r["idx_u"], r["idx_v"], g_u, g_v)
        for side, t in (("u", u), ("v", v)):
            check_grads(t.grad[b].cpu().numpy(), T["grad_" + side], T["S_" + side], f"sym: view {b} grad_{side}")


def test_gradients_come_back_in_the_leafs_own_dtype_layout_and_device():
    from surf_renderer_amd import nearest_points
    c = cases.regular(3)
    want = run(c["u"], c["v"], c["g_u"], c["g_v"])
    u = leaf(c["u"], dtype=torch.float64, device="cpu")                                  # float64 on the CPU
    v = leaf(np.ascontiguousarray(c["v"].transpose(0, 2, 1)), device=DEV)                # a transposed view on the GPU
    r = nearest_points(u, v.transpose(1, 2))
    assert r.dist_u.device.type == "cuda" and r.dist_u.dtype == torch.float32 and not r.idx_u.requires_grad
    ((r.dist_u * torch.tensor(c["g_u"], device=DEV)).sum() + (r.dist_v * torch.tensor(c["g_v"], device=DEV)).sum()).backward()
    assert u.grad.dtype == torch.float64 and u.grad.device.type == "cpu" and u.grad.shape == u.shape
    assert v.grad.dtype == torch.float32 and v.grad.device.type == "cuda" and v.grad.shape == v.shape
    assert np.array_equal(u.grad.numpy(), want["grad_u"].astype(np.float64))
    assert np.array_equal(v.grad.cpu().numpy().transpose(0, 2, 1), want["grad_v"])


def test_only_the_inputs_that_require_grad_get_one():
    from surf_renderer_amd import nearest_points
    c = cases.regular(3)
    want = run(c["u"], c["v"], c["g_u"], c["g_v"])
    for need_u, need_v in ((True, False), (False, True)):
        u, v = leaf(c["u"], requires_grad=need_u), leaf(c["v"], requires_grad=need_v)
        r = nearest_points(u, v)
        ((r.dist_u * torch.tensor(c["g_u"], device=DEV)).sum() + (r.dist_v * torch.tensor(c["g_v"], device=DEV)).sum()).backward()
        assert (u.grad is None) == (not need_u) and (v.grad is None) == (not need_v)
        if need_u:
            assert np.array_equal(u.grad.cpu().numpy(), want["grad_u"])
        else:
            assert np.array_equal(v.grad.cpu().numpy(), want["grad_v"])
    u, v = leaf(c["u"], requires_grad=False), leaf(c["v"], requires_grad=False)
    assert not nearest_points(u, v).dist_u.requires_grad
