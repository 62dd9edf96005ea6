"""nearest_points on the GPU on the inputs the reference answers with NaN or leaves open (tests/pointsets_cases.edges),
against the fp64 oracle alone: exact ties go to the lowest index, a coincident pair has distance 0 and gradient exactly
0, a NaN or infinite coordinate never wins and never leaks into another point's result, magnitudes from 1e-40 to 3e38
neither underflow nor overflow, and a 1300-term fan-in is summed within its bound.  Run with -s for the measured
ratios."""
import numpy as np
import pytest

import pointsets_cases as cases
from pointsets_checks import check_grads, check_values, run, view_oracle

pytestmark = pytest.mark.gpu
EDGES = cases.edges()


# every case plain and squared, but for the magnitudes whose squared distance (1e77) has no float32
RUNS = [(c, sq) for c in EDGES for sq in (False, True) if not (sq and c["name"] == "extreme_magnitudes")]


@pytest.mark.parametrize("c,squared", RUNS, ids=lambda p: p["name"] if isinstance(p, dict) else ("squared" if p else "dist"))
def test_an_edge_case_has_the_oracles_indices_values_and_gradients(c, squared):
    T = view_oracle(c["u"], c["v"], c["g_u"], c["g_v"], squared)
    got = run(c["u"], c["v"], c["g_u"], c["g_v"], squared=squared)
    worst_v = worst_g = 0.0
    for side in "uv":
        assert np.array_equal(got["idx_" + side], T["idx_" + side]), side
        worst_v = max(worst_v, check_values(got["dist_" + side], T["dist_" + side], "dist_" + side))
        worst_g = max(worst_g, check_grads(got["grad_" + side], T["grad_" + side], T["S_" + side], "grad_" + side))
        dead = c.get("dead_" + side, [])
        assert np.isposinf(got["dist_" + side][dead]).all() and (got["idx_" + side][dead] == 0).all()
        assert (got["grad_" + side][dead] == 0).all()                       # nothing reaches a dead point
    print(f"{c['name']}{' squared' if squared else ''}: dist {worst_v:.3g} ulp; gradients {worst_g:.3g} of their bound")


def test_a_coincident_pair_has_distance_zero_and_the_subgradient_zero():
    c = {e["name"]: e for e in EDGES}["coincident_pair"]
    got = run(c["u"], c["v"], c["g_u"], None)                               # the own terms of u alone
    assert got["idx_u"][7] == 4 and got["dist_u"][7] == 0 and (got["grad_u"][7] == 0).all()
    assert (got["dist_u"][np.arange(40) != 7] > 0).all() and (np.abs(got["grad_u"][np.arange(40) != 7]).sum(axis=1) > 0).all()
    same = {e["name"]: e for e in EDGES}["identical_sets"]
    got = run(same["u"], same["v"], same["g_u"], same["g_v"])
    assert (got["dist_u"] == 0).all() and (got["dist_v"] == 0).all() and got["idx_u"].tolist() == list(range(40))
    assert (got["grad_u"] == 0).all() and (got["grad_v"] == 0).all()


def test_the_directed_call_on_the_fan_in_sums_every_query_into_the_one_target():
    c = {e["name"]: e for e in EDGES}["fan_in"]
    T = view_oracle(c["u"], c["v"], c["g_u"], None)
    got = run(c["u"], c["v"], c["g_u"], None, directed=True)
    assert (got["idx_u"] == 0).all() and got["dist_v"] is None
    ratio = check_grads(got["grad_v"], T["grad_v"], T["S_v"], "grad_v")
    check_grads(got["grad_u"], T["grad_u"], T["S_u"], "grad_u")
    print(f"fan_in: grad_v[0] = {got['grad_v'][0]}, S = {T['S_v'][0]}, {ratio:.3g} of its bound")
