"""GPU: projection_renderer on the edge inputs of tests/hard_projection_edge_cases.py against the fp64 restatement tests/
hard_projection_oracle.py; tests/test_hard_projection_edge_cases_cpu.py shows that each case reaches the branch it is
named for and pins the restatement to the reference's own record on the two tie cases.

Tolerances are those of tests/test_hip_hard_projection.py (every entry within 2^-24 |ref| + 2^-40 A + 2^-149 of the
restatement, tests/entry_checks.py; beside it projection_checks: rtol 2e-6, atol 2e-7 max(|want|, 1) for values and 2e-7
max|want| for the gradient); mask, counts and the zeros of dropped surfels are decisions and compared
exactly.  No element is left out: the only non-finite numbers are inputs the results must not depend on (nonfinite_4x6),
so every `want` is finite."""
import numpy as np
import pytest

import entry_checks as ec
import hard_projection_edge_cases as edges
import hard_projection_oracle as ho
from projection_checks import assert_bit_identical, compare_grads, one_view
from test_hip_hard_projection import _compare_values, _counts, _given, _hip

pytestmark = pytest.mark.gpu


def _check(name):
    """Values, mask, counts and the gradient of a case against the restatement; returns what the GPU gave."""
    c = edges.case(name)
    got, got_g = _hip(c)
    want, want_g = edges.expected(name)
    A, A_g = ho.magnitudes({"surfels": c["surfels"], "rgb": c["rgb"]}, c["camera"], c["upstream"])
    _compare_values(got, want, name, A)
    ec.check_all(got_g, want_g, A_g, name + " gradients")
    assert np.array_equal(_counts(c), want["count"]), name
    compare_grads({"rgb": got_g["rgb"]}, want_g, name, nonzero=bool(np.abs(want_g["rgb"]).max() > 0))
    assert got_g["surfels"] is None
    dropped = want["index"] == want["index"].shape[1]
    assert np.all(got_g["rgb"].reshape(*dropped.shape, -1)[dropped] == 0)
    assert np.all(got["out"][got["mask"]] == 0)
    return c, got, got_g


@pytest.mark.parametrize("name,index", [("tie_4x6", 14), ("tie_6x4", 10)])
def test_ties_round_to_the_even_pixel(name, index):
    c, got, got_g = _check(name)
    B, H, W, D = c["shape"]
    counts = _counts(c)
    want = edges.expected(name)[0]
    assert counts[0, index] == want["count"][0, index] >= 3            # the three surfels on the axis, behind and at Z = 0
    assert not got["mask"].reshape(H * W, D)[index].any()
    up = c["upstream"]["out"].astype(np.float64).reshape(H * W, D)
    np.testing.assert_allclose(got_g["rgb"].reshape(H * W, D)[:3], np.tile(up[index] / counts[0, index], (3, 1)), rtol=2e-6)


def test_border_pixels_are_entered_from_outside_the_pixel_centres():
    c, got, got_g = _check("edges_5x7")
    B, H, W, D = c["shape"]
    assert np.all(got_g["rgb"].reshape(H * W, D)[:8] != 0)             # the eight band surfels are counted


def test_non_finite_surfels_are_dropped_and_no_nan_leaks():
    c, got, got_g = _check("nonfinite_4x6")
    B, H, W, D = c["shape"]
    counts = _counts(c)
    for a in (got["out"], got_g["rgb"]):
        assert not np.isnan(a).any() and np.all(np.isfinite(a))
    assert got["mask"].dtype == np.bool_ and counts.min() >= 0 and 0 < counts.sum() <= H * W - 8
    assert np.all(got_g["rgb"].reshape(H * W, D)[:8] == 0)
    assert np.all(counts[0, list(edges.NONFINITE_UPSTREAM)] == 0)


def test_a_view_of_nothing_but_dropped_surfels():
    c, got, got_g = _check("all_dropped_3x5")
    assert np.all(got["out"] == 0) and got["mask"].all() and np.all(got_g["rgb"] == 0) and np.all(_counts(c) == 0)
    c, got, got_g = _check("all_dropped_b2")
    assert np.all(got["out"][0] == 0) and got["mask"][0].all() and np.all(got_g["rgb"][0] == 0)
    assert not got["mask"][1].all() and np.abs(got_g["rgb"][1]).max() > 0
    whole = _given((got, got_g))
    for b in range(2):                                                 # the ordinary view is what it is alone
        assert_bit_identical(whole, _given(_hip(one_view(c, b, ho.INPUTS))), slice(b, b + 1))


@pytest.mark.parametrize("name,pixel", [("cluster_last_8x8", 63), ("cluster_first_8x8", 0)])
def test_a_run_at_either_end_of_the_ordered_keys(name, pixel):
    c, got, got_g = _check(name)
    counts = _counts(c)
    assert counts[0, pixel] == 64 and counts.sum() == 64
    assert np.all(got_g["rgb"] != 0)
    assert_bit_identical(_given((got, got_g)), _given(_hip(c)))
