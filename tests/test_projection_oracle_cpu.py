"""tests/projection_oracle.py against the reference's own projection_renderer_differentiable_fast, recorded in float32
(tests/golden/projection/pr1_*.npz, tools/gen_projection_golden.py): values and input gradients, every element.

Tolerance: the reference runs this function in float32 only, so the fixtures carry its float32 rounding and the
comparison is fp64 restatement against float32 reference.  Measured over all twelve fixtures, max|ref - oracle| /
max|oracle| per array (torch 2.x CPU build, default thread count):
    out 1.44e-6   mask 1.18e-6   image1 1.76e-6   depth 1.74e-6
    grad surfels 4.90e-6   grad rgb 3.28e-6   grad rotated_image 3.43e-7
The bound asserted is 4x the measured value, because float32 summation order changes with the torch build and the
thread count.  It is tight enough to see a wrong constant (checked once by hand): with z_scale 2 -> 2.1 every array
misses its bound by a factor of 700 to 2300, and with sigma taken from W instead of H every array of the 3x5 fixture by
more than 2e4.

Also the kink condition of every seeded case (tests/projection_cases.py), which is what lets the GPU comparison
(tests/test_hip_projection.py) leave no element out."""
import glob
import json
import os

import numpy as np
import pytest

import projection_cases as cases
import projection_oracle as po
from conftest import GOLDEN_DIR

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "projection", "pr1_*.npz")))
MEASURED = {"out": 1.44e-6, "mask": 1.18e-6, "image1": 1.76e-6, "depth": 1.74e-6,
            "grad/surfels": 4.90e-6, "grad/rgb": 3.28e-6, "grad/rotated_image": 3.43e-7}
CAMERA = ("eye", "at", "up", "viewport", "fovy", "focal_length")


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "projection", name + ".npz"), allow_pickle=False)


def _oracle(npz):
    camera = {k: npz["in/camera/" + k] for k in CAMERA}
    inputs = {k: (npz["in/" + k] if "in/" + k in npz.files else None) for k in po.INPUTS}
    upstream = {k[len("grad_in/"):]: npz[k] for k in npz.files if k.startswith("grad_in/")}
    return po.gradients(inputs, camera, upstream, float(npz["in/blur_size"]), **json.loads(str(npz["in/flags"])))


def test_the_fixtures_are_there():
    assert FIXTURES == sorted("pr1_" + cases.tag(n, v) for n, v in cases.ALL)
    for name in FIXTURES:
        npz = _load(name)
        for k in npz.files:
            if k.startswith(("in/surfels", "in/rgb", "in/rotated_image", "grad_in/", "ref/", "grad/")):
                assert npz[k].dtype == np.float32, (name, k)


@pytest.mark.parametrize("name", FIXTURES)
def test_values_and_gradients_match_the_reference(name):
    npz = _load(name)
    values, grads = _oracle(npz)
    assert set(values) == {k[len("ref/"):] for k in npz.files if k.startswith("ref/")}
    for k, got in list(values.items()) + [("grad/" + k, g) for k, g in grads.items()]:
        want = npz[k if k.startswith("grad/") else "ref/" + k].astype(np.float64)
        assert np.all(np.isfinite(want)) and np.abs(want).max() > 0, (name, k)
        err = np.abs(got - want).max() / np.abs(got).max()
        print(f"{name} {k}: max|ref - oracle| / max|oracle| = {err:.3g}")
        assert err <= 4 * MEASURED[k], (name, k, err)


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_a_fixture_holds_the_inputs_of_its_seeded_case(name, variant):
    npz, c = _load("pr1_" + cases.tag(name, variant)), cases.case(name, variant)
    for k in po.INPUTS:
        assert (c[k] is None) == ("in/" + k not in npz.files)
        if c[k] is not None:
            assert c[k].dtype == np.float32 and np.array_equal(npz["in/" + k], c[k]), k      # as the GPU sees them
    for k in CAMERA:
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert json.loads(str(npz["in/flags"])) == c["flags"] and float(npz["in/blur_size"]) == c["blur_size"]
    for k, g in c["upstream"].items():
        assert g.dtype == np.float32 and np.array_equal(npz["grad_in/" + k], g), k


@pytest.mark.parametrize("name", cases.NAMES)
def test_no_drawn_input_sits_on_a_kink(name):
    assert cases.margin(cases.case(name), name) >= 1.0


def test_the_cases_reach_what_they_are_there_for():
    half = {n: po.blur_kernel(cases.case(n)["blur_size"], cases.case(n)["shape"][1])[0] for n in cases.NAMES}
    assert half == {"2x2": 3, "3x5": 1, "12x16": 3, "17x9": 3, "cluster_8x8": 2, "36x48": 2}
    assert po.blur_kernel(cases.case("3x5")["blur_size"], 5)[0] != half["3x5"]         # sigma from W would differ
    mask = cases.expected("12x16")[0]["mask"]
    assert (mask > 1).any() and (mask < 1).any()                                       # both branches of the merge
    mask = cases.expected("cluster_8x8")[0]["mask"]
    assert (mask == 0).any() and (mask > 0).any()
    import torch
    c = cases.case("cluster_8x8")
    px = po.pixel_coordinates(torch.tensor(c["surfels"].astype(np.float64)), c["camera"])
    assert len(torch.unique(torch.floor(px[..., :2] - 0.5).reshape(-1, 2), dim=0)) == 1            # one cell
    c = cases.case("17x9")
    px = po.pixel_coordinates(torch.tensor(c["surfels"].astype(np.float64)), c["camera"])
    u, v, z = px[..., 0] - 0.5, px[..., 1] - 0.5, px[..., 2]
    assert (u < -1).any() and (u > 9).any() and (v < -1).any() and (v > 17).any() and (z < 0).any()


def test_a_batch_is_its_views():
    c = cases.case("17x9")
    whole, whole_g = cases.expected("17x9")
    for b in range(3):
        cam = dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in ("eye", "at", "up")})
        one, one_g = po.gradients({k: (c[k][b:b + 1] if c[k] is not None else None) for k in po.INPUTS}, cam,
                                  {k: g[b:b + 1] for k, g in c["upstream"].items()}, c["blur_size"], **c["flags"])
        for k in whole:
            np.testing.assert_allclose(one[k], whole[k][b:b + 1], rtol=1e-12, atol=1e-14)
        for k in whole_g:
            np.testing.assert_allclose(one_g[k], whole_g[k][b:b + 1], rtol=1e-10, atol=1e-12)
