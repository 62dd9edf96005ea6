"""Each case of tests/projection_edge_cases.py reaches the branch it is named for, shown with the fp64 restatement (tests/
projection_oracle.py) alone; and the restatement against the reference's own projection_renderer_differentiable_fast on
the RECORDED cases (tests/golden/projection/pr2_*.npz, tools/gen_projection_golden.py) under the bound tests/
test_projection_oracle_cpu.py holds the float32 fixtures to: that record is what pins half-width 0, the axes of one
pixel and the Z = 0 arm of the restatement to the reference.  The fixtures carry the prefix pr2_ because test_projection_
oracle_cpu.py holds the pr1_ files to exactly the seeded cases.  Runs without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import projection_edge_cases as edges
import projection_oracle as po
from conftest import GOLDEN_DIR
from test_projection_oracle_cpu import CAMERA, MEASURED

DIR = os.path.join(GOLDEN_DIR, "projection")


@pytest.mark.parametrize("name", edges.NAMES)
def test_the_margin_holds_the_half_width_is_as_named_and_every_want_is_finite(name):
    c = edges.case(name)
    B, H, W, D = c["shape"]
    assert edges.margin(c) >= 1.0
    assert po.blur_kernel(c["blur_size"], H)[0] == edges.HALF[name]
    assert c["flags"]["compute_new_depth"] and all(c[k] is None or c[k].dtype == np.float32 for k in po.INPUTS)
    val, grad = edges.expected(name)
    assert set(val) == set(po.OUTPUTS) and set(grad) == {k for k in po.INPUTS if c[k] is not None}
    for a in list(val.values()) + list(grad.values()):
        assert np.all(np.isfinite(a))


def test_the_half_widths_cover_0_and_the_cap():
    assert sorted(set(edges.HALF.values())) == [0, 1, 3, 64]
    cap = 64                                                     # kProjMaxHalf of srh_projection.h
    assert po.blur_kernel(8.01, 16)[0] == cap and po.blur_kernel(8.2, 16)[0] == cap + 1
    half, taps = po.blur_kernel(0.15, 5)
    assert half == 0 and taps.tolist() == [1.0]                  # one tap: the blur is the identity
    assert po.blur_kernel(0.15, 13)[0] == 0 and po.blur_kernel(0.15, 14)[0] == 1


def test_half0_blurs_nothing_and_raw_passes_the_rotated_image_through():
    c, raw = edges.case("half0_5x7"), edges.case("half0_raw_5x7")
    B, H, W, D = c["shape"]
    assert D == 4 and 2 * D + 1 == 9 and raw["flags"]["blur_rotated_image"] is False
    for k in po.INPUTS:
        assert raw[k] is c[k]
    val, _ = edges.expected("half0_5x7")
    val_raw, _ = edges.expected("half0_raw_5x7")
    for k in val:                                                 # with one tap the switch changes nothing
        assert np.array_equal(val[k], val_raw[k]), k
    mask = val["mask"][..., 0]
    assert (mask == 0).any() and (mask > 1).any() and ((mask > 0) & (mask < 1)).any()
    assert np.array_equal(val_raw["out"][mask == 0], c["rotated_image"].astype(np.float64)[mask == 0])


def test_half64_is_a_window_much_taller_than_the_frame():
    c = edges.case("half64_16x4")
    B, H, W, D = c["shape"]
    half, taps = po.blur_kernel(c["blur_size"], H)
    assert half == 64 and 2 * half + 1 > 8 * H and D == 1
    mask = edges.expected("half64_16x4")[0]["mask"]
    assert mask.min() > 0 and mask.max() < 1


@pytest.mark.parametrize("name,axes", [("row_1x9", (1,)), ("col_9x1", (0,)), ("one_1x1", (0, 1)), ("lane_1x257", (1,))])
def test_an_axis_of_one_pixel_has_the_coordinate_and_the_fraction_exactly_0(name, axes):
    c = edges.case(name)
    B, H, W, D = c["shape"]
    assert [W, H][axes[0]] == 1
    cell, frac = edges.cells(c)
    for a in axes:
        assert np.all(cell[..., a] == 0) and np.all(frac[..., a] == 0)
    for a in {0, 1} - set(axes):
        assert np.all(frac[..., a] > 0)
    mask = edges.expected(name)[0]["mask"]
    if name == "one_1x1":
        assert 1e-4 <= 1 - mask.item() <= 1e-2
    else:
        assert (mask > 1).any() and (mask < 1).any()


@pytest.mark.parametrize("name,n", [("block_16x16", 256), ("lane_1x257", 257)])
def test_the_workgroup_cases_have_the_surfel_counts_they_are_named_for(name, n):
    c = edges.case(name)
    assert c["surfels"].shape == (1, n, 3) and n % 256 == (0 if name == "block_16x16" else 1)
    assert edges.live(c)[0, -1]                                          # the lone lane of the second workgroup carries a gradient
    assert np.abs(edges.expected(name)[1]["surfels"][0, -1]).max() > 0


def test_the_all_dropped_views_hold_nothing_but_dropped_surfels():
    for name in ("all_dropped_3x5", "all_dropped_b2"):
        c = edges.case(name)
        val, grad = edges.expected(name)
        assert not edges.live(c)[0].any()
        z = edges.pixels(c)[0, :, 2]
        assert (z < 0).any() and (z > 0).any()                         # behind the camera and in front of it
        assert np.all(val["mask"][0] == 0) and np.all(val["image1"][0] == 0) and np.all(val["depth"][0] == 0)
        assert np.array_equal(val["out"][0], c["rotated_image"].astype(np.float64)[0])          # half 0: not blurred either
        assert np.all(grad["surfels"][0] == 0) and np.all(grad["rgb"][0] == 0)
        assert np.array_equal(grad["rotated_image"][0], c["upstream"]["out"].astype(np.float64)[0])
    c = edges.case("all_dropped_b2")
    val, grad = edges.expected("all_dropped_b2")
    assert edges.live(c)[1].sum() > 10 and val["mask"][1].max() > 0.5 and np.abs(grad["surfels"][1]).max() > 0


def test_exact_5x7_sits_on_the_integers_and_on_z_0():
    c = edges.case("exact_5x7")
    B, H, W, D = c["shape"]
    assert W % 2 == 1 and H % 2 == 1
    p = edges.pixels(c)[0]
    cell, frac = edges.cells(c)
    for s in edges.ON_AXIS:
        assert tuple(cell[0, s]) == (W // 2, H // 2) and tuple(frac[0, s]) == (0.0, 0.0)
        betas = [(1 - frac[0, s, 0] if dx == 0 else frac[0, s, 0]) * (1 - frac[0, s, 1] if dy == 0 else frac[0, s, 1])
                 for dx in (0, 1) for dy in (0, 1)]
        assert betas == [1.0, 0.0, 0.0, 0.0]
    assert p[0, 2] > 1.9 and p[2, 2] == 0.0                           # -Z: in front; the origin has Z = 0 too
    assert p[edges.Z_ZERO, 2] == 0.0 and tuple(cell[0, edges.Z_ZERO]) == (2, 2)           # divided by 1: in the frame
    assert np.all(frac[0, edges.Z_ZERO] > 0)
    assert frac[0, edges.FX_ZERO, 0] == 0.0 and cell[0, edges.FX_ZERO, 0] == W // 2 and frac[0, edges.FX_ZERO, 1] > 0
    assert frac[0, edges.FY_ZERO, 1] == 0.0 and cell[0, edges.FY_ZERO, 1] == H // 2 and frac[0, edges.FY_ZERO, 0] > 0
    assert edges.live(c)[0, :5].all()
    _, grad = edges.expected("exact_5x7")
    assert np.all(np.abs(grad["surfels"][0, :5]).max(axis=-1) > 0) and np.all(np.abs(grad["rgb"].reshape(H * W, D)[:5]).max(axis=-1) > 0)
    # at Z = 0 the quotient's divisor is the constant 1: Z gets the depth's gradient alone, which (X, Y) do not enter
    assert np.all(grad["surfels"][0, edges.Z_ZERO] != 0)


@pytest.mark.parametrize("name,cell,pixel", [("corner_first_8x8", (-1, -1), 0), ("corner_last_8x8", (7, 7), 63)])
def test_the_corner_clusters_enter_the_frame_by_one_corner(name, cell, pixel):
    c = edges.case(name)
    B, H, W, D = c["shape"]
    got, _ = edges.cells(c)
    assert np.all(got[0] == cell) and edges.live(c).all()
    inside = [(0 <= cell[0] + dx < W) and (0 <= cell[1] + dy < H) for dx in (0, 1) for dy in (0, 1)]
    assert inside == ([False, False, False, True] if pixel == 0 else [True, False, False, False])
    t = {k: torch.as_tensor(c[k].astype(np.float64)) for k in ("surfels", "rgb")}
    _, pre, _, _ = po.scattered(t["surfels"], t["rgb"], c["camera"])
    pre = pre.numpy().reshape(H * W)
    assert pre[pixel] > 0 and np.count_nonzero(pre) == 1               # before the blur, one pixel holds everything
    val, grad = edges.expected(name)
    assert (val["mask"] == 0).any() and val["mask"].reshape(-1)[pixel] == val["mask"].max()
    assert np.all(np.abs(grad["surfels"][0]).max(axis=-1) > 0)


def test_nonfinite_4x6_drops_every_named_surfel_and_the_values_do_not_see_them():
    c = edges.case("nonfinite_4x6")
    B, H, W, D = c["shape"]
    s = c["surfels"][0]
    assert np.isnan(s[:8]).any() and (s[:8] == np.inf).any() and (s[:8] == -np.inf).any()
    assert (np.abs(s[:8]) == np.float32(1e30)).any() and (np.abs(s[:8]) == np.float32(3e38)).any()
    assert not np.isfinite(s[:8]).all(axis=-1).all() and np.isfinite(s[8:]).all()
    assert np.isnan(c["rgb"].reshape(H * W, D)[0]).all() and np.isfinite(c["rgb"].reshape(H * W, D)[1:]).all()
    live = edges.live(c)[0]
    assert not live[:9].any() and live[9:].sum() > 8
    p = edges.pixels(c)[0, 8]
    with np.errstate(over="ignore"):
        assert p[2] < -399.0 and np.exp(-2.0 * p[2]) == np.inf          # its depth weight overflows
    clean = edges.sanitized(c)
    assert np.isfinite(clean["surfels"]).all() and np.isfinite(clean["rgb"]).all() and not edges.live(clean)[0, :9].any()
    assert edges.margin(clean) >= 1.0
    # the values are those of the case as it is, and the sanitised case has the same, bit for bit
    val, grad = edges.expected("nonfinite_4x6")
    val_clean, _ = po.gradients(edges.inputs(clean), clean["camera"], clean["upstream"], clean["blur_size"], **clean["flags"])
    for k in val:
        assert np.array_equal(val[k], val_clean[k]), k
    # the gradient of the case as it is holds NaN in the restatement: every dropped surfel shares the dump slot
    _, raw = po.gradients(edges.inputs(c), c["camera"], c["upstream"], c["blur_size"], **c["flags"])
    assert np.isnan(raw["surfels"]).any()
    assert np.all(grad["surfels"][0, :9] == 0) and np.all(grad["rgb"].reshape(H * W, D)[:9] == 0)
    assert np.abs(grad["surfels"][0, 9:]).max() > 0


@pytest.mark.parametrize("name", edges.RECORDED)
def test_the_restatement_matches_the_recorded_reference(name):
    path = os.path.join(DIR, f"pr2_{name}.npz")
    npz, c = np.load(path, allow_pickle=False), edges.case(name)
    for k in po.INPUTS:
        assert (c[k] is None) == ("in/" + k not in npz.files)
        if c[k] is not None:
            assert np.array_equal(npz["in/" + k], c[k]), k
    for k in CAMERA:
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert json.loads(str(npz["in/flags"])) == c["flags"] and float(npz["in/blur_size"]) == c["blur_size"]
    for k, g in c["upstream"].items():
        assert np.array_equal(npz["grad_in/" + k], g), k
    val, grad = edges.expected(name)
    assert set(val) == {k[len("ref/"):] for k in npz.files if k.startswith("ref/")}
    for k, got in list(val.items()) + [("grad/" + k, g) for k, g in grad.items()]:
        want = npz[k if k.startswith("grad/") else "ref/" + k]
        assert want.dtype == np.float32 and want.shape == got.shape and np.all(np.isfinite(want)), (name, k)
        scale = np.abs(got).max()
        if scale == 0:                                     # a view of dropped surfels: the reference has zeros there too
            assert name == "all_dropped_3x5" and np.all(want == 0), (name, k)
            continue
        err = np.abs(got - want.astype(np.float64)).max() / scale
        print(f"{name} {k}: max|ref - oracle| / max|oracle| = {err:.3g}")
        assert err <= 4 * MEASURED[k], (name, k, err)
    largest = max(os.path.getsize(os.path.join(DIR, f)) for f in os.listdir(DIR) if f.startswith("pr1_"))
    assert os.path.getsize(path) <= largest


def test_the_recorded_fixtures_are_the_recorded_cases():
    have = sorted(f[4:-4] for f in os.listdir(DIR) if f.startswith("pr2_") and f.endswith(".npz"))
    assert have == sorted(edges.RECORDED)
