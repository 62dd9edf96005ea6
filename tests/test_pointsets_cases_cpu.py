"""tests/pointsets_cases.py: the generator is pinned, its regular cases are comparable with the reference (every nearest
point and every outer maximum wins by a relative margin of at least 1e-6, and no pair coincides), the fixtures hold the
cases' inputs, and the edge cases hold what their names say."""
import os

import numpy as np
import pytest

import pointsets_cases as cases
import pointsets_oracle as oracle
from conftest import GOLDEN_DIR

REGULAR_SUMS = {'1x1x3': 'c70295cddf87085d', '1x5x3': 'bd03770934d9355b', '5x1x3': '81397b272464cb2d',
                '63x65x3': 'dc50edb372855dab', '64x64x1': 'b53134ba4e3c8f18', '65x63x2': 'a9514e7df252a8e1',
                '257x1025x3': '5043f7ee5b59b432', '1300x700x4': '938dbf45a115def1', '257x9x3': '37ffc0008e5ad4bd'}
EDGE_SUMS = {'tie_lattice': '6454564d1c97d2d8', 'tie_duplicated_targets': 'b9b138791dec9681',
             'tie_integer_grid': '6c414ec1709c03f2', 'coincident_pair': '7e3dac9803227596',
             'identical_sets': 'a8d4727100d9e086', 'nan_target': '0810513934f1c91e', 'nan_query': 'ff1f22f0100a3f68',
             'inf_coordinates': '3aaf69bb8ebefe6d', 'all_nan_targets': '7d6dcd76dcb51964',
             'extreme_magnitudes': 'ffcfd708b4660c6b', 'fan_in': 'd3479ade5856cf0c'}
MARGIN = 1e-6


def test_the_generator_is_pinned():
    assert cases.REGULAR[:8] == [(1, 1, 3), (1, 5, 3), (5, 1, 3), (63, 65, 3), (64, 64, 1), (65, 63, 2), (257, 1025, 3),
                                 (1300, 700, 4)]
    assert cases.REGULAR[8] == (cases.QUERIES_PER_WORKGROUP + 1, cases.UNROLL + 1, 3) and len(cases.REGULAR) == 9
    assert {cases.tag(k): cases.checksum(cases.regular(k)) for k in range(len(cases.REGULAR))} == REGULAR_SUMS
    assert {e["name"]: cases.checksum(e) for e in cases.edges()} == EDGE_SUMS


def test_the_constants_are_the_kernels():
    from surf_renderer_amd import build
    text = open(os.path.join(build.CSRC, "srh_pointsets.h")).read()
    assert "kPsBlock = 64;" in text and "kPsQ = 4;" in text and "kPsQueries = kPsBlock * kPsQ;" in text
    assert "kPsUnroll = %d;" % cases.UNROLL in text and cases.QUERIES_PER_WORKGROUP == 64 * 4


def _runner_up_margin(best_row):
    """the relative margin of the largest entry over the second largest (inf for a single entry)"""
    if len(best_row) < 2:
        return np.inf
    top = np.sort(best_row)[-2:]
    return (top[1] - top[0]) / top[1]


@pytest.mark.parametrize("k", range(len(cases.REGULAR)), ids=cases.tag)
def test_a_regular_case_is_comparable_with_the_reference(k):
    c = cases.regular(k)
    smallest = {"nearest": np.inf, "outer": np.inf}
    for b in range(cases.VIEWS):
        for q, t in ((c["u"][b], c["v"][b]), (c["v"][b], c["u"][b])):
            d2 = oracle.pair_d2(q, t)
            assert np.isfinite(d2).all() and (d2 > 0).all()                     # no coincident pair
            if d2.shape[1] > 1:
                two = np.partition(d2, 1, axis=1)[:, :2]
                smallest["nearest"] = min(smallest["nearest"], ((two[:, 1] - two[:, 0]) / two[:, 1]).min())
            smallest["outer"] = min(smallest["outer"], _runner_up_margin(np.sqrt(d2.min(axis=1))))
    print(f"{c['name']}: smallest relative margins: nearest {smallest['nearest']:.3g}, outer maximum {smallest['outer']:.3g}")
    assert smallest["nearest"] >= MARGIN and smallest["outer"] >= MARGIN


@pytest.mark.parametrize("k", range(len(cases.REGULAR)), ids=cases.tag)
def test_the_fixture_holds_the_case(k):
    c = cases.regular(k)
    z = np.load(os.path.join(GOLDEN_DIR, "pointsets", "ps1_" + c["name"] + ".npz"))
    for key, name in (("in/u", "u"), ("in/v", "v"), ("grad_in/g", "g"), ("grad_in/g_u", "g_u"), ("grad_in/g_v", "g_v")):
        assert z[key].dtype == np.float32 and np.array_equal(z[key], c[name]), key
    N, M, D = cases.REGULAR[k]
    for p, dt in (("ref64", np.float64), ("ref32", np.float32)):
        assert z[p + "/out"].shape == (cases.VIEWS, 3) and z[p + "/out"].dtype == dt
        assert z[p + "/grad/u"].shape == (cases.VIEWS, N, D) and z[p + "/grad/v"].shape == (cases.VIEWS, M, D)
        assert np.isfinite(z[p + "/out"]).all() and np.isfinite(z[p + "/grad/u"]).all() and np.isfinite(z[p + "/grad/v"]).all()


def test_the_edge_cases_hold_what_their_names_say():
    e = {c["name"]: c for c in cases.edges()}
    r = oracle.nearest(e["tie_lattice"]["u"], e["tie_lattice"]["v"])
    assert r["idx_u"].tolist() == [0, 0] and r["idx_v"].tolist() == [0, 0] and r["dist_u"].tolist() == [1.0, 1.0]
    r = oracle.nearest(e["tie_duplicated_targets"]["u"], e["tie_duplicated_targets"]["v"])
    assert r["idx_u"].max() < 9                                             # the copies at 9.. never win
    r = oracle.nearest(e["tie_integer_grid"]["u"], e["tie_integer_grid"]["v"])
    d2 = oracle.pair_d2(e["tie_integer_grid"]["u"], e["tie_integer_grid"]["v"])
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 2).any() and (r["dist_u"] == np.sqrt(0.5)).all()
    c = e["coincident_pair"]
    r = oracle.nearest(c["u"], c["v"])
    assert r["idx_u"][7] == 4 and r["dist_u"][7] == 0 and r["dist_v"][4] == 0 and r["dist_v"][30] == 0
    assert (r["dist_u"][np.arange(40) != 7] > 0).all()
    r = oracle.nearest(e["identical_sets"]["u"], e["identical_sets"]["v"])
    assert (r["dist_u"] == 0).all() and r["idx_u"].tolist() == list(range(40))
    for name in ("nan_target", "nan_query", "inf_coordinates", "all_nan_targets"):
        c = e[name]
        r = oracle.nearest(c["u"], c["v"])
        for side in "uv":
            dead = np.zeros(len(c[side]), bool)
            dead[c.get("dead_" + side, [])] = True
            assert np.isinf(r["dist_" + side][dead]).all() and (r["idx_" + side][dead] == 0).all(), name
            assert np.isfinite(r["dist_" + side][~dead]).all(), name
            assert dead.any() or "dead_" + side not in c
    c = e["extreme_magnitudes"]
    assert np.abs(c["u"]).max() > 2.9e38 and 0 < np.abs(c["u"])[c["u"] != 0].min() < 1.1e-40
    r = oracle.nearest(c["u"], c["v"])
    assert np.isfinite(r["dist_u"]).all() and (r["dist_u"] > 0).all() and r["dist_u"].min() < 1e-39
    c = e["fan_in"]
    assert c["u"].shape == (1300, 3) and c["v"].shape == (1, 3)
