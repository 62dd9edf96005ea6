"""tests/pointsets_oracle.py against the fixtures of the reference's own hausdorff in float64 (tests/golden/pointsets):
the three values to 2^-49 relative (both are within (D + 2) 2^-53 of exact; the summation order over D may differ), the
gradients to 2^-40 S per entry, and the indices against the argmins of a float64 torch composition."""
import os

import numpy as np
import pytest
import torch

import pointsets_cases as cases
import pointsets_oracle as oracle
from conftest import GOLDEN_DIR


def fixture(k):
    return np.load(os.path.join(GOLDEN_DIR, "pointsets", "ps1_" + cases.tag(k) + ".npz"))


@pytest.mark.parametrize("k", range(len(cases.REGULAR)), ids=cases.tag)
def test_values_and_gradients_agree_with_the_reference_in_float64(k):
    z = fixture(k)
    worst_v, worst_g = 0.0, 0.0
    for b in range(cases.VIEWS):
        u, v, g = z["in/u"][b], z["in/v"][b], z["grad_in/g"][b].astype(np.float64)
        r = oracle.nearest(u, v)
        got, ref = np.array(oracle.hausdorff(r)), z["ref64/out"][b]
        worst_v = max(worst_v, (np.abs(got - ref) / np.abs(ref)).max())
        assert (np.abs(got - ref) <= 2.0 ** -49 * np.abs(ref)).all()
        g_u, g_v = oracle.hausdorff_upstreams(r, g)
        G = oracle.gradients(u, v, r["idx_u"], r["idx_v"], g_u, g_v)
        for side in "uv":
            err, bound = np.abs(G["grad_" + side] - z["ref64/grad/" + side][b]), 2.0 ** -40 * G["S_" + side]
            assert (err <= bound).all(), side
            worst_g = max(worst_g, (err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    print(f"{cases.tag(k)}: values {worst_v:.3g} relative (bound {2.0 ** -49:.3g}); gradients {worst_g:.3g} of their bound")


@pytest.mark.parametrize("k", range(len(cases.REGULAR)), ids=cases.tag)
def test_indices_are_the_argmins_of_a_float64_torch_composition(k):
    c = cases.regular(k)
    for b in range(cases.VIEWS):
        u, v = torch.tensor(c["u"][b], dtype=torch.float64), torch.tensor(c["v"][b], dtype=torch.float64)
        D = torch.sqrt(torch.sum((u[:, None, :] - v[None]) ** 2, dim=-1))
        r = oracle.nearest(c["u"][b], c["v"][b])
        assert np.array_equal(r["idx_u"], D.argmin(dim=1).numpy()) and np.array_equal(r["idx_v"], D.argmin(dim=0).numpy())
        torch.testing.assert_close(torch.tensor(r["dist_u"]), D.min(dim=1).values, rtol=2.0 ** -49, atol=0)
        torch.testing.assert_close(torch.tensor(r["dist_v"]), D.min(dim=0).values, rtol=2.0 ** -49, atol=0)


def test_squared_and_directed_and_the_zero_gradient_rules():
    c = {e["name"]: e for e in cases.edges()}["coincident_pair"]
    r = oracle.nearest(c["u"], c["v"])
    sq = oracle.nearest(c["u"], c["v"], squared=True)
    assert np.array_equal(sq["idx_u"], r["idx_u"]) and np.array_equal(np.sqrt(sq["dist_u"]), r["dist_u"])
    G = oracle.gradients(c["u"], c["v"], r["idx_u"], r["idx_v"], c["g_u"], None)
    assert (G["grad_u"][7] == 0).all() and (G["S_u"][7] == 0).all()             # dist_u[7] = 0: the subgradient 0
    others = np.arange(40) != 7
    assert (np.abs(G["grad_u"][others]).sum(axis=1) > 0).all()
    # a unit direction times g; under `squared` 2 (u - v) g
    np.testing.assert_allclose(np.linalg.norm(G["grad_u"][others], axis=1), np.abs(c["g_u"][others]), rtol=1e-12)
    G2 = oracle.gradients(c["u"], c["v"], r["idx_u"], None, c["g_u"], None, squared=True)
    want = 2.0 * c["g_u"][:, None] * (c["u"].astype(np.float64) - c["v"].astype(np.float64)[r["idx_u"]])
    np.testing.assert_allclose(G2["grad_u"], want, rtol=1e-15)
    # every gradient of v is the fan-in of the u side: the sums agree
    np.testing.assert_allclose(G["grad_v"].sum(axis=0), -G["grad_u"].sum(axis=0), rtol=1e-12)
    dead = {e["name"]: e for e in cases.edges()}["all_nan_targets"]
    r = oracle.nearest(dead["u"], dead["v"])
    G = oracle.gradients(dead["u"], dead["v"], r["idx_u"], r["idx_v"], dead["g_u"], dead["g_v"])
    assert all((G[k] == 0).all() for k in G)
