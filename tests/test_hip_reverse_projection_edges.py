"""GPU: projection_reverse_renderer on the edge inputs of tests/reverse_projection_edge_cases.py against the fp64
restatement tests/reverse_projection_oracle.py; tests/test_reverse_projection_edge_cases_cpu.py shows that each case
reaches what it is named for and pins the restatement to the reference's own record on the two one-pixel axes.

Tolerances are the standing ones of tests/test_hip_reverse_projection.py (projection_checks: rtol 2e-6, atol 2e-7
max(|want|, 1) for values and 2e-7 max|want| per gradient array); the mask, the rotated image passed through where the
mask is 0, and the zero gradients of samples off the frame are compared exactly.  No element is left out."""
import numpy as np
import pytest

import camera_chain_oracle as co
import reverse_projection_edge_cases as edges
from projection_checks import assert_bit_identical, compare_grads, compare_values
from test_hip_camera_warp import compare_camera, reverse
from test_hip_reverse_projection import _hip

pytestmark = pytest.mark.gpu
ZERO_BY_CONSTRUCTION = {"all_outside_3x5": ("rgb", "in_pos_wc", "out_pos_wc")}       # no sample reaches a texel


def _compare_grads(got_g, want_g, name):
    """Every gradient within the tolerance; those that are 0 by construction exactly 0 on both sides."""
    zero = ZERO_BY_CONSTRUCTION.get(name, ())
    compare_grads({k: g for k, g in got_g.items() if k not in zero}, {k: w for k, w in want_g.items() if k not in zero}, name)
    for k in zero:
        assert np.all(want_g[k] == 0) and np.all(got_g[k] == 0), (name, k)


@pytest.mark.parametrize("name", edges.NAMES)
def test_values_and_gradients_match_the_restatement(name):
    c = edges.case(name)
    got, got_g = _hip(c)
    want, want_g = edges.expected(name)
    compare_values(got, want, name, exact=("mask",))
    _compare_grads(got_g, want_g, name)
    if not got["mask"].any():                          # row_1x5, col_5x1, lane_1x257, all_outside_3x5
        assert name != "block_16x16"
        assert np.array_equal(got["out"], c["rotated_image"].astype(np.float64))
        assert np.array_equal(got_g["rotated_image"], c["upstream"]["out"].astype(np.float64))
    if name == "all_outside_3x5":
        assert np.all(got["image1"] == 0) and np.all(got["depth"] == 0)


@pytest.mark.parametrize("name", ["lane_1x257", "block_16x16"])
def test_two_runs_are_bit_identical(name):
    c = edges.case(name)
    assert_bit_identical(_hip(c), _hip(c))


@pytest.mark.parametrize("name", ["lane_1x257", "all_outside_3x5"])
def test_camera_gradients_match_the_restatement(name):
    """camera_grad=True: lane_1x257 reduces a second workgroup of one live lane; in all_outside_3x5 no sample reaches a
    texel, so neither camera moves the loss."""
    c = edges.case(name)
    got, got_g, got_cam = reverse(c)
    want, want_g, want_cam = co.reverse_gradients(edges.inputs(c), c["camera1"], c["camera2"], c["upstream"],
                                                  wrt=c["wrt"], **c["flags"])
    compare_values(got, want, name, exact=("mask",))
    _compare_grads(got_g, want_g, name)
    for label in ("camera1", "camera2"):
        compare_camera(got_cam[label], want_cam[label], f"{name} {label}")
        if name == "all_outside_3x5":
            for k in co.CAMERA_KEYS:
                assert np.all(want_cam[label][k] == 0) and np.all(got_cam[label][k] == 0), (label, k)
        else:
            assert max(np.abs(g).max() for g in want_cam[label].values()) > 0, label
    # values and the other gradients are those of the call without camera leaves, bit for bit
    detached = reverse(c, cameras={"camera1": c["camera1"], "camera2": c["camera2"]}, camera_grad=False)[:2]
    assert_bit_identical(detached, (got, got_g))
    again = reverse(c)[2]
    for label in ("camera1", "camera2"):
        assert_bit_identical((got_cam[label],), (again[label],))
