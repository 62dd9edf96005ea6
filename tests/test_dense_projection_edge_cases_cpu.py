"""Each case of tests/dense_projection_edge_cases.py reaches what it is named for, shown with the fp64 restatement (tests/
dense_projection_oracle.py) alone; and the restatement against the reference's own projection_renderer_differentiable on
the RECORDED cases (tests/golden/dense_projection/dp2_*.npz, tools/gen_dense_projection_golden.py) under the bound tests/
test_dense_projection_oracle_cpu.py holds the float64 fixtures to.  The fixtures carry the prefix dp2_ because that
module holds the dp1_ files to exactly the seeded frames.  Runs without a GPU."""
import os

import numpy as np
import pytest

import dense_projection_edge_cases as edges
import dense_projection_oracle as do
from conftest import GOLDEN_DIR
from test_dense_projection_oracle_cpu import CAMERA, MEASURED

DIR = os.path.join(GOLDEN_DIR, "dense_projection")


@pytest.mark.parametrize("name,layout,rotated", edges.ALL)
def test_every_case_is_clear_of_the_kink_and_every_want_is_finite(name, layout, rotated):
    c = edges.case(name, layout, rotated)
    assert do.z_margin(c["surfels"], c["camera"]) >= edges.Z_MARGIN
    assert np.isfinite(c["surfels"]).all() and c["surfels"].dtype == np.float32
    B, H, W, D = c["shape"]
    assert edges.sigma(c) == pytest.approx(edges._SPEC[name][4] * (1 if layout == "grid" else H), rel=1e-6)
    val, grad = edges.expected(name, layout, rotated)
    assert set(grad) == {k for k in do.INPUTS if c[k] is not None}
    for a in list(val.values()) + list(grad.values()):
        assert np.all(np.isfinite(a))


@pytest.mark.parametrize("name,layout,rotated", edges.ALL)
def test_the_separable_form_is_the_dense_form(name, layout, rotated):
    """The spread between the restatement's two formulations, per array over its maximum: what a third formulation of
    the same sum -- the kernels' -- may differ by before the fp32 store.  Largest measured 7.9e-15 (grad rgb of
    tile_33x33_flat); the sigma extremes stay below 2.7e-15."""
    want, want_g = edges.expected(name, layout, rotated)
    got, got_g = edges.expected(name, layout, rotated, fn=do.project_separable)
    for k, w in list(want.items()) + [("grad " + k, g) for k, g in want_g.items()]:
        g = got_g[k[5:]] if k.startswith("grad ") else got[k]
        scale = np.abs(w).max()
        if scale == 0:                             # one_1x1: the pixel scales are 0, no coordinate moves
            assert name == "one_1x1" and np.all(g == 0), k
            continue
        print(f"{edges.tag(name, layout, rotated)} {k}: spread {np.abs(g - w).max() / scale:.3g}")
        assert np.abs(g - w).max() <= 1e-12 * scale, (k, np.abs(g - w).max() / scale)


@pytest.mark.parametrize("name,axes", [("row_1x5", (1,)), ("col_5x1", (0,)), ("one_1x1", (0, 1))])
def test_an_axis_of_one_pixel_has_the_coordinate_exactly_at_the_pixel_centre(name, axes):
    c = edges.case(name)
    p = edges.pixels(c)
    for a in axes:
        assert np.all(p[..., a] == 0.5)
    for a in {0, 1} - set(axes):
        assert len(np.unique(p[..., a])) == p.shape[1]
    val, grad = edges.expected(name)
    if name == "one_1x1":                          # weight exp(0) on the one pixel, and nothing the surfel could move
        assert val["mask"].item() == 1.0 and np.all(grad["surfels"] == 0) and np.abs(grad["rgb"]).max() > 0
        assert np.all(edges.expected(name, "grid", True)[1]["rotated_image"] == 0)           # 1 - mask = 0
    else:
        assert np.abs(grad["surfels"]).max() > 0


def test_far_9x7_weighs_exactly_0_on_every_pixel_and_overflows_the_recurrence():
    for layout in edges.LAYOUTS:
        c = edges.case("far_9x7", layout)
        B, H, W, D = c["shape"]
        assert c["named"] == edges.FAR and np.isfinite(c["surfels"][0, :12]).all()
        p = edges.pixels(c)[0]
        u, v = p[:12, 0] - 0.5, p[:12, 1] - 0.5
        beyond = np.maximum(np.maximum(-u, u - (W - 1)), np.maximum(-v, v - (H - 1)))
        # the fp32 rounding of a world coordinate of 1e11 moves the 1e12 ones to some 1e9 pixels, on either side
        assert np.all(beyond[[0, 3, 6, 9]] > 0.99e3) and np.all(beyond[[1, 4, 7, 10]] > 0.99e6) and np.all(beyond[[2, 5, 8, 11]] > 1e9)
        assert (u < -1e3).any() and (u > 1e3).any() and (v < -1e3).any() and (v > 1e3).any()
        h = 1.0 / (2 * edges.sigma(c) ** 2)
        gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        with np.errstate(over="ignore"):
            w = np.exp(-((u[:, None, None] - gx) ** 2 + (v[:, None, None] - gy) ** 2) * h)
            assert np.all(w == 0)                                                  # at every pixel, in fp64
            # k_dproj_fwd's outward factor exp((2 |d| - 1) h) at the tile's nearest column: inf for every one of them
            # as a grid (sigma 0.9), and from 1e6 pixels on in the flat layout (sigma 8.1)
            factor = np.exp((2.0 * beyond - 1.0) * h)
            assert np.all(factor[1::3] == np.inf) and np.all(factor[2::3] == np.inf)
            assert np.all(factor[0::3] == np.inf) == (layout == "grid")
        val, grad = edges.expected("far_9x7", layout)
        assert np.all(grad["surfels"][0, :12] == 0) and np.all(grad["rgb"].reshape(H * W, D)[:12] == 0)
        assert np.abs(grad["surfels"][0, 12:]).min(axis=0).max() > 0 and val["mask"].min() > 0.1
        near = np.setdiff1d(np.arange(H * W), edges.FAR)
        assert np.abs(p[near, 0]).max() < 20 and np.abs(p[near, 1]).max() < 20


def test_the_sigma_extremes_reach_denormal_weights_and_a_mask_of_60():
    tiny = np.finfo(np.float64).tiny
    m = edges.expected("sigma_0p1_9x7")[0]["mask"]
    assert m.min() < 1e-30 and m.max() > 0.5 and np.exp(-1 / 0.1 ** 2) < 1e-43
    m = edges.expected("sigma_0p03_9x7")[0]["mask"]
    assert (m == 0).any() or ((m > 0) & (m < tiny)).any()                          # underflowed, or denormal
    assert (m < 1e-10).sum() > m.size // 2 and m.max() > 0.5 and np.exp(-1 / 0.03 ** 2) == 0.0
    out = edges.expected("sigma_0p03_9x7")[0]["out"]
    assert np.abs(out).max() <= 1.0 + 1e-9                                         # S / (m + 1e-10) stays a mean
    m = edges.expected("sigma_12_9x7")[0]["mask"]
    assert 50 < m.min() and m.max() < 63
    for name in ("sigma_0p1_9x7", "sigma_0p03_9x7", "sigma_12_9x7"):
        assert np.abs(edges.expected(name)[1]["surfels"]).max() > 0


def test_tile_33x33_has_a_second_tile_of_one_pixel_in_both_directions():
    c = edges.case("tile_33x33")
    B, H, W, D = c["shape"]
    tile = 32                                                                      # kDProjTile of srh_dense_projection.h
    assert (H - 1) // tile == 1 and (W - 1) // tile == 1 and H - tile == 1 and W - tile == 1 and D == 1
    val, grad = edges.expected("tile_33x33")
    assert val["mask"][0, 32, :, 0].min() > 0 and val["mask"][0, :, 32, 0].min() > 0
    assert np.abs(grad["surfels"]).max() > 0


@pytest.mark.parametrize("name,layout", edges.RECORDED)
def test_the_restatement_matches_the_recorded_reference(name, layout):
    path = os.path.join(DIR, f"dp2_{edges.tag(name, layout)}.npz")
    npz, c = np.load(path, allow_pickle=False), edges.case(name, layout)
    assert str(npz["in/precision"]) == "float64" and "in/rotated_image" not in npz.files
    for k in ("surfels", "rgb"):
        assert np.array_equal(npz["in/" + k], c[k]), k
    for k in CAMERA:
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert float(npz["in/blur_size"]) == c["blur_size"]
    for k, g in c["upstream"].items():
        assert np.array_equal(npz["grad_in/" + k], g), k
    val, grad = edges.expected(name, layout)
    for k, got in list(val.items()) + [("grad/" + k, g) for k, g in grad.items()]:
        want = npz[k if k.startswith("grad/") else "ref/" + k]
        assert want.dtype == np.float64 and want.shape == got.shape and np.all(np.isfinite(want)), (name, k)
        err = np.abs(got - want).max() / np.abs(got).max()
        print(f"{name} {k}: max|ref - oracle| / max|oracle| = {err:.3g}")
        assert err <= 4 * MEASURED[k], (name, k, err)
    if name == "far_9x7":                          # the reference gives the far surfels exact zeros as well
        B, H, W, D = c["shape"]
        assert np.all(npz["grad/surfels"][0, :12] == 0) and np.all(npz["grad/rgb"].reshape(H * W, D)[:12] == 0)
    largest = max(os.path.getsize(os.path.join(DIR, f)) for f in os.listdir(DIR) if f.startswith("dp1_"))
    assert os.path.getsize(path) <= largest


def test_the_recorded_fixtures_are_the_recorded_cases():
    have = sorted(f[4:-4] for f in os.listdir(DIR) if f.startswith("dp2_") and f.endswith(".npz"))
    assert have == sorted(edges.tag(n, layout) for n, layout in edges.RECORDED)
