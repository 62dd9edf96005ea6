"""tests/hard_projection_oracle.py against the reference's own projection_renderer, recorded in float64 and in float32
(tests/golden/hard_projection/hp1_*.npz, tools/gen_hard_projection_golden.py): the pixel index of every surfel, the mask,
the counts, the values and the gradient to rgb, every element.

The pixel a surfel lands on is a decision, and the seeded cases keep every decision clear of its threshold (tests/
hard_projection_cases.py), so indices, masks and counts must be EXACTLY equal to the records, in both precisions.  Values
and gradients: the restatement against ref64 at 1e-9 of each array's largest magnitude (the same sums in the same
precision), ref32 against ref64 at the layers' stated tolerance (projection_checks.RTOL / ATOL_SCALE).

Also the conditions on every seeded case, which are what lets the GPU comparison (tests/test_hip_hard_projection.py) leave
no element out, and that a batch equals its views in the restatement."""
import glob
import os

import numpy as np
import pytest
import torch

import hard_projection_cases as cases
import hard_projection_oracle as ho
import projection_oracle as po
from conftest import GOLDEN_DIR
from projection_checks import ATOL_SCALE, RTOL, one_view

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "hard_projection", "hp1_*.npz")))
CAMERA = ("eye", "at", "up", "viewport", "fovy", "focal_length")


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "hard_projection", name + ".npz"), allow_pickle=False)


def _counts(index, N):
    return np.stack([np.bincount(row, minlength=N + 1)[:N] for row in index])


def test_the_fixtures_are_there():
    assert FIXTURES == sorted("hp1_" + n for n in cases.NAMES)
    for name in FIXTURES:
        npz = _load(name)
        assert npz["in/surfels"].dtype == np.float32 and npz["in/rgb"].dtype == np.float32
        assert npz["grad_in/out"].dtype == np.float32
        for k in ("out", "grad/rgb"):
            assert npz["ref64/" + k].dtype == np.float64 and npz["ref32/" + k].dtype == np.float32, (name, k)
        for p in ("ref64/", "ref32/"):
            assert npz[p + "mask"].dtype == np.bool_ and npz[p + "index"].dtype == np.int64, (name, p)


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_fixture_holds_the_inputs_of_its_seeded_case(name):
    npz, c = _load("hp1_" + name), cases.case(name)
    for k in ho.INPUTS:
        assert c[k].dtype == np.float32 and np.array_equal(npz["in/" + k], c[k]), k              # as the GPU sees them
    for k in CAMERA:
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert np.array_equal(npz["grad_in/out"], c["upstream"]["out"])


@pytest.mark.parametrize("name", cases.NAMES)
def test_indices_masks_and_counts_equal_the_records(name):
    npz = _load("hp1_" + name)
    v, _ = cases.expected(name)
    N = v["index"].shape[1]
    for p in ("ref64/", "ref32/"):
        assert np.array_equal(v["index"], npz[p + "index"]), (name, p)
        assert v["mask"].dtype == np.bool_ and np.array_equal(v["mask"], npz[p + "mask"]), (name, p)
        assert np.array_equal(v["count"], _counts(npz[p + "index"], N)), (name, p)


@pytest.mark.parametrize("name", cases.NAMES)
def test_values_and_gradients_match_the_float64_reference(name):
    npz = _load("hp1_" + name)
    v, g = cases.expected(name)
    for k, got in (("out", v["out"]), ("grad/rgb", g["rgb"])):
        want = npz["ref64/" + k]
        assert want.shape == got.shape and np.all(np.isfinite(want)), (name, k)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name} {k}: max|ref64 - restatement| / max|ref64| = {err:.3g}")
        assert err <= 1e-9, (name, k, err)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_float32_reference_meets_the_stated_tolerance(name):
    npz = _load(name)
    for k in ("out", "grad/rgb"):
        got, want = npz["ref32/" + k].astype(np.float64), npz["ref64/" + k]
        scale = max(np.abs(want).max(), 1.0) if k == "out" else np.abs(want).max()
        share = (np.abs(got - want) / (ATOL_SCALE * scale + RTOL * np.abs(want))).max()
        print(f"{name} {k}: the reference's float32 error is {share:.3g} of the tolerance")
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL_SCALE * scale, err_msg=f"{name} {k}")


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_drawn_input_meets_the_kink_condition(name):
    c = cases.case(name)
    assert ho.kink_margin(c["surfels"], c["camera"]) >= 1.0
    px = po.pixel_coordinates(torch.tensor(c["surfels"].astype(np.float64)), c["camera"]).numpy()
    assert np.abs(px[..., :2] - np.round(px[..., :2])).min() >= 1e-4 and np.abs(px[..., 2]).min() >= 1e-3


def test_the_cases_reach_what_they_are_there_for():
    # 17x9: surfels off every edge and behind the camera; dropped ones get no gradient
    c = cases.case("17x9")
    px = po.pixel_coordinates(torch.tensor(c["surfels"].astype(np.float64)), c["camera"]).numpy()
    u, v, z = px[..., 0] - 0.5, px[..., 1] - 0.5, px[..., 2]
    assert (u < -0.5).any() and (u > 8.5).any() and (v < -0.5).any() and (v > 16.5).any() and (z < 0).any()
    val, g = cases.expected("17x9")
    dropped = val["index"] == 17 * 9
    assert dropped.any() and np.all(g["rgb"][dropped] == 0) and np.all(g["rgb"][~dropped] != 0)
    # cluster_8x8: one run of 64, every other pixel empty
    val, g = cases.expected("cluster_8x8")
    assert np.array_equal(np.unique(val["index"]), [3 * 8 + 3]) and val["count"].max() == 64
    assert val["mask"].sum() == 63 * 3 and not val["mask"].reshape(64, 3)[27].any()
    assert np.all(val["out"][val["mask"]] == 0)
    c = cases.case("cluster_8x8")
    np.testing.assert_allclose(val["out"].reshape(64, 3)[27], c["rgb"].astype(np.float64).reshape(64, 3).mean(0), rtol=1e-14)
    # several surfels on one pixel, empty pixels and dropped surfels elsewhere too
    for name in ("12x16", "36x48"):
        val, _ = cases.expected(name)
        assert val["count"].max() >= 2 and val["mask"].any() and not val["mask"].all()
    assert cases.case("36x48")["shape"][1] * cases.case("36x48")["shape"][2] > 4 * 256           # several workgroups
    assert cases.case("2x2")["shape"][3] == 1 and cases.case("3x5")["shape"][3] == 4
    assert cases.case("17x9")["rgb"].ndim == 3 and cases.case("12x16")["rgb"].ndim == 4


def test_rounding_to_the_nearest_pixel_and_the_reference_quirks():
    """On hand-made coordinates: the nearest pixel (not the cell floor gives), Z = 0 is divided by 1, a surfel behind the
    camera lands like any other, a NaN and a pixel outside the frame are dropped.  (An exact tie cannot be placed
    through a camera in floating point; the cases stay 1e-4 clear of them.)"""
    W, H = 4, 2
    camera = {"eye": np.array([[0.0, 0.0, 0.0]]), "at": np.array([[0.0, 0.0, -1.0]]), "up": np.array([[0.0, 1.0, 0.0]]),
              "viewport": [0, 0, W, H], "fovy": 0.7, "focal_length": 0.5}
    h = np.tan(0.35) * 2 * 0.5
    w = h * W / H
    sx, sy = -(W - 1) / w * 0.5, (H - 1) / h * 0.5          # pixel coordinate = s X / Z + (W, H) / 2

    def at(px, py, Z):
        d = Z if Z != 0 else 1.0
        return [(px - W / 2) / sx * d, (py - H / 2) / sy * d, Z]

    surfels = torch.tensor([[at(1.1, 0.9, -2.0),        # (px, py) - 1/2 = (0.6, 0.4) -> (1, 0)
                             at(1.9, 1.1, -2.0),        # (1.4, 0.6) -> (1, 1)
                             at(3.0, 2.1, -2.0),        # (2.5, 1.6) -> row 2: below the frame, dropped
                             at(3.2, 1.25, 2.0),        # behind the camera: (2.7, 0.75) -> (3, 1)
                             at(0.75, 0.75, 0.0),       # Z = 0: (0.25, 0.25) -> (0, 0)
                             [float("nan"), 0.0, -1.0], at(-0.25, 0.75, -2.0), at(4.75, 0.75, -2.0)]], dtype=torch.float64)
    idx, _ = ho.pixel_index(surfels, camera)
    assert idx[0].tolist() == [1, W + 1, 8, W + 3, 0, 8, 8, 8]
    assert torch.round(torch.tensor([0.5, 1.5, 2.5, -0.5])).tolist() == [0.0, 2.0, 2.0, -0.0]     # ties to even


def test_a_batch_is_its_views():
    for name in ("12x16", "17x9"):
        c = cases.case(name)
        whole, whole_g = cases.expected(name)
        for b in range(c["shape"][0]):
            one = one_view(c, b, ho.INPUTS)
            v, g = ho.gradients({k: one[k] for k in ho.INPUTS}, one["camera"], one["upstream"])
            for k in whole:
                assert np.array_equal(v[k], whole[k][b:b + 1]), k
            assert np.array_equal(g["rgb"], whole_g["rgb"][b:b + 1])
