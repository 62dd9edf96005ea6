"""Each case of tests/reverse_projection_edge_cases.py reaches what it is named for, shown with the fp64 restatement
(tests/reverse_projection_oracle.py) alone; and the restatement against the reference's own projection_reverse_renderer
on the RECORDED cases (tests/golden/reverse_projection/rp2_*.npz, tools/gen_reverse_projection_golden.py) under the bound
tests/test_reverse_projection_oracle_cpu.py holds the float32 fixtures to, the mask exactly.  The fixtures carry the
prefix rp2_ because that module holds the rp1_ files to exactly the seeded cases.  Runs without a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import reverse_projection_edge_cases as edges
import reverse_projection_oracle as ro
from conftest import GOLDEN_DIR
from test_reverse_projection_oracle_cpu import CAMERA, MEASURED

DIR = os.path.join(GOLDEN_DIR, "reverse_projection")


def _projections(c):
    t = {k: torch.tensor(c[k].astype(np.float64)) for k in ("in_pos_wc", "out_pos_wc")}
    return [x.numpy() for x in ro.depths(t["in_pos_wc"], t["out_pos_wc"], c["camera1"], c["camera2"])]


@pytest.mark.parametrize("name", edges.NAMES)
def test_the_conditions_hold_and_every_want_is_finite(name):
    c = edges.case(name)
    assert edges.margin(c) >= 1.0
    assert c["rotated_image"] is not None and c["flags"] == {"compute_new_depth": True, "depth_epsilon": 0.1}
    assert c["camera1"]["fovy"] != c["camera2"]["fovy"] and all(c[k].dtype == np.float32 for k in ro.INPUTS)
    val, grad = edges.expected(name)
    assert set(val) == set(ro.OUTPUTS) and set(grad) == set(ro.INPUTS)
    for a in list(val.values()) + list(grad.values()):
        assert np.all(np.isfinite(a))


@pytest.mark.parametrize("name,axis", [("row_1x5", 1), ("col_5x1", 0), ("lane_1x257", 1)])
def test_along_an_axis_of_one_pixel_the_coordinate_is_exactly_a_half_and_the_mask_0(name, axis):
    c = edges.case(name)
    B, H, W, D = c["shape"]
    assert [W, H][axis] == 1
    c1, c2, d, d_out = _projections(c)
    assert np.all(c1[..., axis] == 0.5) and np.all(c2[..., axis] == 0.5)
    val, grad = edges.expected(name)
    assert np.all(val["mask"] == 0) and np.array_equal(val["out"], c["rotated_image"].astype(np.float64))
    # image1 and the new depth are sampled all the same: full weight on the one row (column), and both move with out_pos_wc
    assert np.abs(val["image1"]).max() > 0.3 and np.count_nonzero(val["image1"]) > val["image1"].size // 2
    assert np.abs(val["depth"]).max() > 1.0
    for k in ("rgb", "in_pos_wc", "out_pos_wc"):
        assert np.abs(grad[k]).max() > 0, k
    assert np.array_equal(grad["rotated_image"], c["upstream"]["out"].astype(np.float64))
    # some samples would pass the depth test and the other axis' bounds: the single axis alone zeroes their mask
    other = c1[..., 1 - axis]
    inside = (other >= 0.5) & (other < [W, H][1 - axis] - 0.5)
    assert (inside & ((d <= d_out + 0.1)[..., 0])).any()


def test_all_outside_3x5_samples_nothing():
    c = edges.case("all_outside_3x5")
    B, H, W, D = c["shape"]
    c1, c2, _, _ = _projections(c)
    u, v = c1[..., 0] - 0.5, c1[..., 1] - 0.5
    assert np.all((u <= -1) | (u >= W) | (v <= -1) | (v >= H))            # no bilinear tap reaches a texel
    assert (u <= -1).any() and (u >= W).any() and (v <= -1).any() and (v >= H).any()
    assert ((c2[..., 0] > 0.5) & (c2[..., 0] < W - 0.5)).any()            # in_pos_wc is ordinary
    val, grad = edges.expected("all_outside_3x5")
    assert np.all(val["image1"] == 0) and np.all(val["mask"] == 0) and np.all(val["depth"] == 0)
    assert np.array_equal(val["out"], c["rotated_image"].astype(np.float64))
    for k in ("rgb", "in_pos_wc", "out_pos_wc"):
        assert np.all(grad[k] == 0), k
    assert np.array_equal(grad["rotated_image"], c["upstream"]["out"].astype(np.float64))


@pytest.mark.parametrize("name,n", [("block_16x16", 256), ("lane_1x257", 257)])
def test_the_workgroup_cases_have_the_pixel_counts_they_are_named_for(name, n):
    c = edges.case(name)
    B, H, W, D = c["shape"]
    assert H * W == n and c["out_pos_wc"].shape == (1, n, 3)             # the kernels' workgroup is 256 lanes
    val, grad = edges.expected(name)
    assert np.abs(grad["out_pos_wc"][0, -1]).max() > 0                   # the last lane carries a gradient
    if name == "block_16x16":
        assert 0.1 < val["mask"].mean() < 0.9 and np.all(np.isin(val["mask"], (0.0, 1.0)))


@pytest.mark.parametrize("name", edges.RECORDED)
def test_the_restatement_matches_the_recorded_reference(name):
    path = os.path.join(DIR, f"rp2_{name}.npz")
    npz, c = np.load(path, allow_pickle=False), edges.case(name)
    for k in ro.INPUTS:
        assert np.array_equal(npz["in/" + k], c[k]), k
    for cam in ("camera1", "camera2"):
        for k in CAMERA:
            assert np.array_equal(npz[f"in/{cam}/{k}"], np.asarray(c[cam][k])), (cam, k)
    assert json.loads(str(npz["in/flags"])) == c["flags"]
    assert set(c["upstream"]) == {k[len("grad_in/"):] for k in npz.files if k.startswith("grad_in/")}
    for k, g in c["upstream"].items():
        assert np.array_equal(npz["grad_in/" + k], g), k
    val, grad = edges.expected(name)
    assert set(val) == {k[len("ref/"):] for k in npz.files if k.startswith("ref/")}
    assert np.array_equal(val["mask"], npz["ref/mask"]) and np.all(npz["ref/mask"] == 0)
    assert np.array_equal(npz["ref/out"], c["rotated_image"])             # the reference passes it through as well
    for k, got in list(val.items()) + [("grad/" + k, g) for k, g in grad.items()]:
        if k == "mask":
            continue
        want = npz[k if k.startswith("grad/") else "ref/" + k]
        assert want.dtype == np.float32 and want.shape == got.shape and np.all(np.isfinite(want)), (name, k)
        err = np.abs(got - want.astype(np.float64)).max() / np.abs(got).max()
        print(f"{name} {k}: max|ref - oracle| / max|oracle| = {err:.3g}")
        assert err <= 4 * MEASURED[k], (name, k, err)
    largest = max(os.path.getsize(os.path.join(DIR, f)) for f in os.listdir(DIR) if f.startswith("rp1_"))
    assert os.path.getsize(path) <= largest


def test_the_recorded_fixtures_are_the_recorded_cases():
    have = sorted(f[4:-4] for f in os.listdir(DIR) if f.startswith("rp2_") and f.endswith(".npz"))
    assert have == sorted(edges.RECORDED)
