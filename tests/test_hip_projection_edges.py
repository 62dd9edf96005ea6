"""GPU: projection_renderer_differentiable_fast on the edge inputs of tests/projection_edge_cases.py against the fp64
restatement tests/projection_oracle.py; tests/test_projection_edge_cases_cpu.py shows that each case reaches the branch
it is named for and pins the restatement to the reference's own record on five of them.

Tolerances are the standing ones of tests/test_hip_projection.py (projection_checks: rtol 2e-6, atol 2e-7 max(|want|, 1)
for values and 2e-7 max|want| per gradient array).  The zeros of dropped surfels' gradient rows, the mask of an empty
view and the untouched rotated image where the mask is 0 are decisions and compared exactly.  No element is left out: the
only non-finite numbers are inputs the results must not depend on (nonfinite_4x6), so every `want` is finite, and no
output or gradient may hold a NaN."""
import numpy as np
import pytest

import camera_chain_oracle as co
import projection_edge_cases as edges
import projection_oracle as po
from projection_checks import assert_bit_identical, compare_grads, compare_values, one_view
from test_hip_camera_warp import compare_camera, project
from test_hip_projection import _hip

pytestmark = pytest.mark.gpu
ZERO_BY_CONSTRUCTION = {"all_dropped_3x5": ("surfels", "rgb")}       # the oracle's gradient is exactly 0: no surfel lands


def _check(name):
    """Values and gradients of a case against the restatement, the zero rows of its dropped surfels; returns what the
    GPU gave."""
    c = edges.case(name)
    B, H, W, D = c["shape"]
    got, got_g = _hip(c)
    want, want_g = edges.expected(name)
    for a in list(got.values()) + list(got_g.values()):
        assert not np.isnan(a).any() and np.all(np.isfinite(a)), name
    compare_values(got, want, name)
    zero = ZERO_BY_CONSTRUCTION.get(name, ())
    compare_grads({k: g for k, g in got_g.items() if k not in zero}, {k: w for k, w in want_g.items() if k not in zero}, name)
    for k in zero:
        assert np.all(want_g[k] == 0) and np.all(got_g[k] == 0), (name, k)
    dropped = ~edges.live(c)
    assert np.all(got_g["surfels"][dropped] == 0) and np.all(got_g["rgb"].reshape(B, H * W, D)[dropped] == 0), name
    return c, got, got_g


@pytest.mark.parametrize("name", [n for n in edges.NAMES if n != "nonfinite_4x6"])
def test_values_and_gradients_match_the_restatement(name):
    c, got, got_g = _check(name)
    if name.startswith("all_dropped"):                                 # an empty view: the rotated image, untouched
        assert np.all(got["mask"][0] == 0) and np.all(got["image1"][0] == 0) and np.all(got["depth"][0] == 0)
        assert np.array_equal(got["out"][0], c["rotated_image"].astype(np.float64)[0])
        assert np.array_equal(got_g["rotated_image"][0], c["upstream"]["out"].astype(np.float64)[0])


def test_non_finite_and_huge_surfels_get_zero_rows_and_no_nan_leaks():
    """Values against the restatement on the case as it is; gradients against the restatement on the case with the nine
    named surfels moved to a finite point far off the frame and the NaN rgb row set to 0 (projection_edge_cases.
    sanitized): the same function of every other input.  Surfel 8 is finite with a depth weight exp(800) = inf."""
    c, got, got_g = _check("nonfinite_4x6")
    B, H, W, D = c["shape"]
    named = list(c["named"])
    assert named == list(range(9)) and not edges.live(c)[0, :9].any()
    assert np.all(got_g["surfels"][0, named] == 0) and np.all(got_g["rgb"].reshape(H * W, D)[named] == 0)
    assert np.abs(got_g["surfels"][0, 9:]).max() > 0


def test_the_unblurred_rotated_image_passes_through_bit_for_bit_where_the_mask_is_0():
    c = edges.case("half0_raw_5x7")
    got, _ = _hip(c, wrt=())
    empty = got["mask"][..., 0] == 0
    assert empty.any() and not empty.all()
    assert np.array_equal(got["out"][empty], c["rotated_image"].astype(np.float64)[empty])


def test_with_one_tap_the_blur_is_the_identity():
    """half0_5x7 at its default blur_size 0.15 and at 0.05 and 0.39, which floor to half 0 as well: taps [1]."""
    c = edges.case("half0_5x7")
    H = c["shape"][1]
    base, base_g = _hip(c)
    for blur_size in (0.05, 0.39):
        assert po.blur_kernel(blur_size, H)[0] == 0
        got, got_g = _hip(dict(c, blur_size=blur_size))
        compare_values(got, base, f"half0_5x7 at blur_size {blur_size}")
        compare_grads(got_g, base_g, f"half0_5x7 at blur_size {blur_size}")


def _twice(c):
    return dict(c, shape=(2, *c["shape"][1:]), upstream={k: np.concatenate((u, u)) for k, u in c["upstream"].items()},
                camera=dict(c["camera"], **{k: np.concatenate((c["camera"][k], c["camera"][k])) for k in co.CAMERA_KEYS}),
                **{k: (np.concatenate((c[k], c[k])) if c[k] is not None else None) for k in po.INPUTS})


@pytest.mark.parametrize("name", ["lane_1x257", "all_dropped_b2", "corner_last_8x8"])
def test_two_runs_are_bit_identical_and_a_batch_equals_its_views(name):
    c = edges.case(name)
    first = _hip(c)
    assert_bit_identical(first, _hip(c))
    whole, c2 = (first, c) if c["shape"][0] > 1 else (_hip(_twice(c)), _twice(c))          # one view: stacked twice
    for b in range(2):
        assert_bit_identical(whole, _hip(one_view(c2, b, po.INPUTS)), slice(b, b + 1))


@pytest.mark.parametrize("name", ["lane_1x257", "all_dropped_b2", "half0_5x7", "nonfinite_4x6"])
def test_camera_gradients_match_the_restatement(name):
    """camera_grad=True: lane_1x257 reduces a second workgroup of one live lane, all_dropped_b2 a view that brings
    nothing but zeros, and the dropped surfels of nonfinite_4x6 must bring zeros and not 0 * inf (the restatement is
    taken on the sanitised case, which has the same values bit for bit)."""
    c = edges.case(name)
    got, got_g, got_cam = project(c)
    s = edges.sanitized(c) if name == "nonfinite_4x6" else c
    want, want_g, want_cam = co.project_gradients(edges.inputs(s), s["camera"], s["upstream"], s["blur_size"], **s["flags"])
    for a in list(got_g.values()) + list(got_cam["camera"].values()):
        assert np.all(np.isfinite(a)), name
    compare_values(got, want, name)
    compare_grads(got_g, want_g, name)
    compare_camera(got_cam["camera"], want_cam["camera"], f"{name} camera")
    assert all(np.abs(g).max() > 0 for g in want_cam["camera"].values())
    if name == "all_dropped_b2":                                       # the dropped view's camera does not move the loss
        for k in co.CAMERA_KEYS:
            assert np.all(want_cam["camera"][k][0] == 0) and np.all(got_cam["camera"][k][0] == 0), k
    # values and the other gradients are those of the call without camera leaves, bit for bit
    assert_bit_identical(project(c, cameras={"camera": c["camera"]}, camera_grad=False)[:2], (got, got_g))
    assert_bit_identical((got_cam["camera"],), (project(c)[2]["camera"],))
