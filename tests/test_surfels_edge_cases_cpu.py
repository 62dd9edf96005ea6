"""Each case of tests/surfels_edge_cases.py reaches the branch it is named for, shown with the fp64 restatement
(tests/surfels_oracle.py) alone: the special depths are the bit patterns they claim to be, the restatement treats them as
the kernels' header says (d = max(depth, 0), a NaN stays a NaN and passes its gradient through), and the long single rows
and columns need a second, partly empty workgroup.  Runs without a GPU."""
import numpy as np
import pytest

import surfels_edge_cases as edges
import surfels_oracle as so
from projection_checks import ATOL_SCALE

BLOCK = 256                        # kSurfBlock


def test_the_special_depths_are_the_bit_patterns_they_are_named_for():
    d = edges.SPECIAL
    assert d.dtype == np.float32 and d.shape == (9,)
    bits = d.view(np.uint32)
    assert bits[0] == 0 and bits[1] == 0x80000000                      # +0.0, -0.0
    assert bits[2] == 1 and d[2] > 0                                   # the smallest subnormal
    assert d[3] == np.finfo(np.float32).tiny and bits[3] == 0x00800000  # the smallest normal
    assert d[4] == np.inf and d[5] == -np.inf and np.isnan(d[7]) and d[6] == np.float32(1e30) and d[8] == 2.0
    assert [q for q in range(9) if not d[q] > 0 and not np.isnan(d[q])] == list(edges.DEAD)
    assert [q for q in range(9) if not np.isfinite(d[q]) and not d[q] < 0] == list(edges.NONFINITE)
    for name in ("special_3x3", "special_3x3_camera"):
        assert np.array_equal(edges.case(name)["depth"].view(np.uint32), bits.reshape(1, 9))
    # +inf sits on the optical axis of the odd grid: both grid coordinates are exactly 0 there
    gx, gy = so.pixel_grid(edges.case("special_3x3")["camera"])
    assert gx[1] == 0 and gy[1] == 0 and 4 == 1 * 3 + 1 and np.all(gx[[0, 2]] != 0) and np.all(gy[[0, 2]] != 0)


@pytest.mark.parametrize("name", ["special_3x3", "special_3x3_camera"])
def test_the_restatement_takes_every_special_depth_the_way_the_header_says(name):
    c = edges.case(name)
    val, grad = edges.expected(name)
    pos, g = val["pos"][0], grad["depth"][0]
    full = edges.full_gradient(c)[0]
    tol = ATOL_SCALE * np.abs(full).max()
    rest = np.asarray(c["camera"]["eye"], np.float64)[0] if c["frame"] == "world" else np.zeros(3)
    for q in edges.DEAD:                                               # +0.0, -0.0, -inf: the relu's flat side
        assert np.array_equal(pos[q], rest) and g[q] == 0, q
    assert np.all(np.isfinite(g))
    for q in range(9):
        assert np.isfinite(pos[q]).all() == (q not in edges.NONFINITE), q
        assert not np.isfinite(pos[q]).any() or q not in edges.NONFINITE, q       # every component, not only some
        if q not in edges.DEAD:                                        # the full gradient, far above the tolerance
            np.testing.assert_allclose(g[q], full[q], rtol=1e-12, atol=0, err_msg=str(q))
            assert abs(full[q]) > 100 * tol, (q, full[q], tol)
    assert np.isnan(pos[7]).all()                                      # a NaN stays a NaN
    if c["frame"] == "camera":                                         # inf * 0 = NaN next to -inf
        assert np.isnan(pos[4, :2]).all() and pos[4, 2] == -np.inf
    # the subnormal and the smallest normal are alive, though their points do not leave the eye in fp32
    assert np.all(pos[2] != rest) or c["frame"] == "world"
    assert np.abs(pos[6]).max() > 1e29 and np.abs(pos[6]).max() < np.finfo(np.float32).max


@pytest.mark.parametrize("name", ["row_1x300", "column_300x1"])
def test_a_single_row_or_column_needs_a_second_partly_empty_workgroup(name):
    c = edges.case(name)
    B, H, W = c["shape"]
    N = H * W
    assert B == 2 and min(H, W) == 1 and BLOCK < N < 2 * BLOCK
    gx, gy = so.pixel_grid(c["camera"])
    half_w, half_h = so.frame_extent(c["camera"])
    if H == 1:                                                         # linspace(1, -1, 1) is its start point
        assert gy.shape == (1,) and gy[0] == np.float64(np.float32(half_h)) and len(np.unique(gx)) == W
    else:
        assert gx.shape == (1,) and gx[0] == np.float64(np.float32(-half_w)) and len(np.unique(gy)) == H
    dead = c["depth"] <= 0
    assert dead[:, :BLOCK].any() and dead[:, BLOCK:].any() and not dead[:, N - 1].any()
    assert (c["depth"] == 0).any() and (c["depth"] < 0).any() and np.abs(c["depth"][~dead]).min() >= 1.5
    val, grad = edges.expected(name)
    full = edges.full_gradient(c)
    assert np.all(grad["depth"][dead] == 0)
    np.testing.assert_allclose(grad["depth"][~dead], full[~dead], rtol=1e-12)
    eye = np.broadcast_to(np.asarray(c["camera"]["eye"], np.float64)[:, None], (B, N, 3))
    assert np.array_equal(val["pos"][dead], eye[dead])


def test_five_views_of_one_pixel():
    c = edges.case("b5_1x1")
    assert c["shape"] == (5, 1, 1) and c["depth"].shape == (5, 1)
    assert c["depth"][1, 0] == 0 and c["depth"][3, 0] == -1 and np.all(c["depth"][[0, 2, 4], 0] >= 1.5)
    val, grad = edges.expected("b5_1x1")
    assert np.all(grad["depth"][[1, 3]] == 0) and np.all(grad["depth"][[0, 2, 4]] != 0)
    assert len({tuple(e) for e in c["camera"]["eye"]}) == 5            # five cameras of their own
