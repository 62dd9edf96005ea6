"""tests/reverse_projection_oracle.py against the reference's own projection_reverse_renderer, recorded in float32
(tests/golden/reverse_projection/rp1_*.npz, tools/gen_reverse_projection_golden.py): values and input gradients, every
element.

The mask is a decision, and the seeded cases keep every decision clear of its threshold (tests/
reverse_projection_cases.py), so it must be EXACTLY equal on every fixture.  Everything else is fp64 restatement against
float32 reference.  Measured over all ten fixtures, max|ref - oracle| / max|oracle| per array (torch 2.x CPU build,
default thread count):
    out 3.94e-6   image1 6.36e-6   depth 4.45e-6
    grad rgb 4.01e-6   grad in_pos_wc 2.46e-6   grad out_pos_wc 6.48e-6   grad rotated_image 0 (a 0/1 weight: exact)
The bound asserted is 4x the measured value, as for the forward re-projection.  It is tight enough to see a wrong
convention (checked once by hand): with align_corners=True in the oracle 367 mask elements differ and every other array
misses its bound by a factor above 2e4 (image1 0.594 against 2.5e-5, grad in_pos_wc 0.732 against 9.8e-6).

Also the conditions on every seeded case, which are what lets the GPU comparison (tests/
test_hip_reverse_projection.py) leave no element out, and that a batch equals its views in the oracle."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import reverse_projection_cases as cases
import reverse_projection_oracle as ro
from conftest import GOLDEN_DIR

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "reverse_projection", "rp1_*.npz")))
MEASURED = {"out": 3.94e-6, "mask": 0.0, "image1": 6.36e-6, "depth": 4.45e-6, "grad/rgb": 4.01e-6,
            "grad/in_pos_wc": 2.46e-6, "grad/out_pos_wc": 6.48e-6, "grad/rotated_image": 0.0}
CAMERA = ("eye", "at", "up", "viewport", "fovy", "focal_length")


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "reverse_projection", name + ".npz"), allow_pickle=False)


def _oracle(npz):
    cameras = [{k: npz[f"in/{cam}/{k}"] for k in CAMERA} for cam in ("camera1", "camera2")]
    inputs = {k: (npz["in/" + k] if "in/" + k in npz.files else None) for k in ro.INPUTS}
    upstream = {k[len("grad_in/"):]: npz[k] for k in npz.files if k.startswith("grad_in/")}
    return ro.gradients(inputs, *cameras, upstream, **json.loads(str(npz["in/flags"])))


def test_the_fixtures_are_there():
    assert FIXTURES == sorted("rp1_" + cases.tag(n, v) for n, v in cases.FIXTURES)
    for name in FIXTURES:
        npz = _load(name)
        for k in npz.files:
            if k.startswith(("in/rgb", "in/in_pos_wc", "in/out_pos_wc", "in/rotated_image", "grad_in/", "ref/", "grad/")):
                assert npz[k].dtype == np.float32, (name, k)


@pytest.mark.parametrize("name", FIXTURES)
def test_values_and_gradients_match_the_reference(name):
    npz = _load(name)
    values, grads = _oracle(npz)
    assert set(values) == {k[len("ref/"):] for k in npz.files if k.startswith("ref/")}
    assert np.array_equal(values["mask"], npz["ref/mask"]), name
    for k, got in list(values.items()) + [("grad/" + k, g) for k, g in grads.items()]:
        want = npz[k if k.startswith("grad/") else "ref/" + k].astype(np.float64)
        assert np.all(np.isfinite(want)) and want.shape == got.shape, (name, k)
        scale = np.abs(got).max()
        if scale == 0:                     # the 1x1 frame's coordinates do not move; a mask that is 0 everywhere
            assert np.all(want == 0), (name, k)
            continue
        err = np.abs(got - want).max() / scale
        print(f"{name} {k}: max|ref - oracle| / max|oracle| = {err:.3g}")
        assert err <= 4 * MEASURED[k], (name, k, err)


@pytest.mark.parametrize("name,variant", cases.FIXTURES)
def test_a_fixture_holds_the_inputs_of_its_seeded_case(name, variant):
    npz, c = _load("rp1_" + cases.tag(name, variant)), cases.case(name, variant)
    for k in ro.INPUTS:
        assert (c[k] is None) == ("in/" + k not in npz.files)
        if c[k] is not None:
            assert c[k].dtype == np.float32 and np.array_equal(npz["in/" + k], c[k]), k      # as the GPU sees them
    for cam in ("camera1", "camera2"):
        for k in CAMERA:
            assert np.array_equal(npz[f"in/{cam}/{k}"], np.asarray(c[cam][k])), (cam, k)
    assert json.loads(str(npz["in/flags"])) == c["flags"]
    assert set(c["upstream"]) == {k[len("grad_in/"):] for k in npz.files if k.startswith("grad_in/")}
    for k, g in c["upstream"].items():
        assert g.dtype == np.float32 and np.array_equal(npz["grad_in/" + k], g), k


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_drawn_input_meets_the_conditions(name):
    c = cases.case(name)
    assert cases.margin(c, name) >= 1.0
    if name == cases.VARIANT_OF:
        assert cases.epsilons(name) == (0.1, 0.0)
        for share in cases.mask_shares(c, name):
            assert 0.1 <= share <= 0.9, share


def _projections(c):
    t = {k: torch.tensor(c[k].astype(np.float64)) for k in ("in_pos_wc", "out_pos_wc")}
    return ro.depths(t["in_pos_wc"], t["out_pos_wc"], c["camera1"], c["camera2"])


def test_the_cases_reach_what_they_are_there_for():
    for name in cases.NAMES:
        c = cases.case(name)
        assert c["camera1"]["fovy"] != c["camera2"]["fovy"] and c["camera1"]["focal_length"] != c["camera2"]["focal_length"]
    v, g = cases.expected("1x1")
    c = cases.case("1x1")
    assert np.all(v["mask"] == 0) and np.array_equal(v["out"], c["rotated_image"].astype(np.float64))
    assert np.array_equal(v["image1"], c["rgb"].astype(np.float64)) and np.abs(g["rgb"]).max() > 0
    # 12x16: pixels inside the frame that the raised square hides from camera 1, by far more than depth_epsilon
    c = cases.case("12x16")
    c1, _, d, d_out = _projections(c)
    H, W = c["shape"][1:3]
    inside = ~((c1[..., 1] < 0.5) | (c1[..., 0] < 0.5) | (c1[..., 1] >= H - 0.5) | (c1[..., 0] >= W - 0.5))
    assert int((inside & ((d - d_out)[..., 0] > 0.5)).sum()) >= 10
    assert np.all(np.isin(cases.expected("12x16")[0]["mask"], (0.0, 1.0)))
    # 17x9: samples off every edge, points behind both cameras
    c1, c2, _, _ = _projections(cases.case("17x9"))
    for px in (c1, c2):
        u, v, z = px[..., 0] - 0.5, px[..., 1] - 0.5, px[..., 2]
        assert (u < -1).any() and (u > 9).any() and (v < -1).any() and (v > 17).any() and (z < 0).any()
    # cluster_8x8: one sample cell; four texels carry all of grad rgb
    c1, _, _, _ = _projections(cases.case("cluster_8x8"))
    assert len(torch.unique(torch.floor(c1[..., :2] - 0.5).reshape(-1, 2), dim=0)) == 1
    touched = np.abs(cases.expected("cluster_8x8")[1]["rgb"]).sum(-1) > 0
    assert touched.sum() == 4
    assert cases.case("36x48")["shape"][1] * cases.case("36x48")["shape"][2] > 4 * 256       # several workgroups


def test_the_variants_change_what_they_name():
    base, base_g = cases.expected("12x16")
    assert not np.array_equal(cases.expected("12x16", "eps0")[0]["mask"], base["mask"])
    no_rot = cases.expected("12x16", "no_rotated")[0]
    assert np.array_equal(no_rot["out"], no_rot["image1"]) and np.array_equal(no_rot["image1"], base["image1"])
    assert "depth" not in cases.expected("12x16", "no_depth")[0] and "depth" in base
    assert np.all(cases.expected("12x16", "no_depth")[1]["in_pos_wc"] == 0) and np.abs(base_g["in_pos_wc"]).max() > 0
    for k in ro.INPUTS:
        assert set(cases.expected("12x16", "wrt_" + k)[1]) == {k}
    assert all(np.all(g == 0) for g in cases.expected("12x16", "only_mask")[1].values())
    assert np.abs(cases.expected("12x16", "only_depth")[1]["in_pos_wc"]).max() > 0
    assert np.all(cases.expected("12x16", "only_depth")[1]["rgb"] == 0)


def test_a_batch_is_its_views():
    for name in ("12x16", "17x9"):
        c = cases.case(name)
        whole, whole_g = cases.expected(name)
        for b in range(c["shape"][0]):
            one, one_g = cases.gradients(cases.view(c, b))
            for k in whole:
                np.testing.assert_allclose(one[k], whole[k][b:b + 1], rtol=1e-12, atol=1e-14)
            for k in whole_g:
                np.testing.assert_allclose(one_g[k], whole_g[k][b:b + 1], rtol=1e-10, atol=1e-12)
