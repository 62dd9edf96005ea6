"""tests/dense_projection_oracle.py against the reference's own projection_renderer_differentiable, recorded in float64
(tests/golden/dense_projection/dp1_*.npz, tools/gen_dense_projection_golden.py: the unedited function runs in float64
under ref_harness.precision): values and input gradients, every element, without a rotated image -- with one the
reference raises, so that branch is checked against the restatement alone (see tests/dense_projection_oracle.py).

Tolerance: both sides are float64, so what is left is the order of operations.  Measured over all ten fixtures,
max|ref - oracle| / max|oracle| per array (torch 2.x CPU build; the same at 1, 2, 3, 4, 8 and 16 threads):
    out 1.79e-15   mask 0   grad surfels 3.72e-16   grad rgb 9.46e-16
The bound asserted is 4x the measured value, because summation order changes with the torch build.  The mask came out
bit for bit (the restatement forms it by the reference's operations in the reference's order); a measurement of 0 says
"below one unit in the last place", so its entry is 2^-52, the smallest difference float64 resolves at the array's
maximum.  The bound sees a wrong constant: test_a_wrong_constant_trips_the_bound asserts that every array misses it, and
the factors measured (out, mask, grad surfels, grad rgb) are
    sigma from H instead of rgb.shape[-2] (3x5_grid)       2.6e13  1.1e15  3.6e14  1.9e14
    pixel centres without the 1/2 (12x16_grid)             1.9e13  1.8e14  4.1e14  1.2e14
    W instead of W - 1 in the pixel scale (12x16_grid)     1.3e13  1.8e14  3.6e14  7.7e13

Also: the separable form (the kernels') equals the dense form to 1e-12 of each array's maximum, the |Z| margin of every
seeded case (which is what lets the GPU comparison leave no element out), and the fixtures' inputs are the seeded
cases'."""
import glob
import os

import numpy as np
import pytest

import dense_projection_cases as cases
import dense_projection_oracle as do
from conftest import GOLDEN_DIR

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "dense_projection", "dp1_*.npz")))
EPS = 2.0 ** -52
MEASURED = {"out": 1.79e-15, "mask": EPS, "grad/surfels": 3.72e-16, "grad/rgb": 9.46e-16}
CAMERA = ("eye", "at", "up", "viewport", "fovy", "focal_length")


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "dense_projection", name + ".npz"), allow_pickle=False)


def _oracle(npz, wrong=()):
    camera = {k: npz["in/camera/" + k] for k in CAMERA}
    inputs = {k: (npz["in/" + k] if "in/" + k in npz.files else None) for k in do.INPUTS}
    upstream = {k[len("grad_in/"):]: npz[k] for k in npz.files if k.startswith("grad_in/")}
    return do.gradients(inputs, camera, upstream, float(npz["in/blur_size"]), wrong=wrong)


def _errors(npz, wrong=()):
    """{array: max|ref - oracle| / max|oracle|} of one fixture"""
    values, grads = _oracle(npz, wrong)
    assert set(values) == {k[len("ref/"):] for k in npz.files if k.startswith("ref/")}
    errs = {}
    for k, got in list(values.items()) + [("grad/" + k, g) for k, g in grads.items()]:
        want = npz[k if k.startswith("grad/") else "ref/" + k].astype(np.float64)
        assert got.shape == want.shape and np.all(np.isfinite(want)) and np.abs(want).max() > 0, k
        errs[k] = np.abs(got - want).max() / np.abs(got).max()
    return errs


def test_the_fixtures_are_there():
    assert FIXTURES == sorted("dp1_" + cases.tag(f, layout) for f, layout in cases.RECORDED)
    for name in FIXTURES:
        npz = _load(name)
        assert str(npz["in/precision"]) == "float64" and "in/rotated_image" not in npz.files
        for k in npz.files:
            if k.startswith(("in/surfels", "in/rgb", "grad_in/")):
                assert npz[k].dtype == np.float32, (name, k)
            if k.startswith(("ref/", "grad/")):
                assert npz[k].dtype == np.float64, (name, k)


@pytest.mark.parametrize("name", FIXTURES)
def test_values_and_gradients_match_the_reference(name):
    for k, err in _errors(_load(name)).items():
        print(f"{name} {k}: max|ref - oracle| / max|oracle| = {err:.3g}")
        assert err <= 4 * MEASURED[k], (name, k, err)


@pytest.mark.parametrize("wrong,name", [("sigma_from_height", "dp1_3x5_grid"), ("no_half_pixel", "dp1_12x16_grid"),
                                        ("scale_by_width", "dp1_12x16_grid")])
def test_a_wrong_constant_trips_the_bound(wrong, name):
    factors = {k: err / (4 * MEASURED[k]) for k, err in _errors(_load(name), wrong=(wrong,)).items()}
    print(f"{wrong} on {name}: misses the bound by {', '.join(f'{k} {v:.3g}x' for k, v in factors.items())}")
    assert min(factors.values()) > 1, factors


@pytest.mark.parametrize("frame,layout", cases.RECORDED)
def test_a_fixture_holds_the_inputs_of_its_seeded_case(frame, layout):
    npz, c = _load("dp1_" + cases.tag(frame, layout)), cases.case(frame, layout)
    for k in ("surfels", "rgb"):
        assert c[k].dtype == np.float32 and np.array_equal(npz["in/" + k], c[k]), k           # as the GPU sees them
    for k in CAMERA:
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert float(npz["in/blur_size"]) == c["blur_size"]
    for k, g in c["upstream"].items():
        assert g.dtype == np.float32 and np.array_equal(npz["grad_in/" + k], g), k


@pytest.mark.parametrize("frame", cases.FRAMES)
def test_no_drawn_surfel_is_near_the_kink(frame):
    c = cases.case(frame)
    assert do.z_margin(c["surfels"], c["camera"]) >= cases.Z_MARGIN


@pytest.mark.parametrize("frame,layout,rotated", cases.ALL)
def test_the_separable_form_is_the_dense_form(frame, layout, rotated):
    c = cases.case(frame, layout, rotated)
    want, want_g = cases.expected(frame, layout, rotated)
    got, got_g = do.gradients(cases.inputs(c), c["camera"], c["upstream"], c["blur_size"], fn=do.project_separable)
    for k, w in list(want.items()) + [("grad " + k, g) for k, g in want_g.items()]:
        g = got_g[k[5:]] if k.startswith("grad ") else got[k]
        assert np.abs(w).max() > 0 and np.abs(g - w).max() <= 1e-12 * np.abs(w).max(), (k, np.abs(g - w).max() / np.abs(w).max())


def test_the_cases_reach_what_they_are_there_for():
    import torch
    for frame in cases.FRAMES:
        s = cases.sigma(cases.case(frame, "grid"))
        assert 0.6 - 1e-6 <= s <= 1.5 + 1e-6, (frame, s)
        H = cases.case(frame)["shape"][1]
        assert cases.sigma(cases.case(frame, "flat")) == pytest.approx(s * H)            # the quirk: N instead of W
    c = cases.case("3x5")
    assert do.sigma_of((3, 0), c["blur_size"]) != cases.sigma(c)                        # sigma from H would differ
    c = cases.case("17x9")
    px = do.pixel_coordinates(torch.tensor(c["surfels"].astype(np.float64)), c["camera"])
    u, v, z = px[..., 0] - 0.5, px[..., 1] - 0.5, px[..., 2]
    s = cases.sigma(c)
    assert (u < -2 * s).any() and (u > 8 + 2 * s).any() and (v < -2 * s).any() and (v > 16 + 2 * s).any()
    assert all((z[b] < 0).sum() == 4 for b in range(3))                                 # behind the camera, and counted
    mask = cases.expected("36x48")[0]["mask"]
    assert mask.max() > 1.5                                                             # not normalised
    # the flat layout of the same image is another function: sigma is H times as wide
    assert not np.allclose(cases.expected("12x16", "flat")[0]["mask"].reshape(-1), cases.expected("12x16")[0]["mask"].reshape(-1))


def test_a_batch_is_its_views():
    c = cases.case("17x9", "grid", True)
    whole, whole_g = cases.expected("17x9", "grid", True)
    for b in range(3):
        cam = dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in ("eye", "at", "up")})
        one, one_g = do.gradients({k: c[k][b:b + 1] for k in do.INPUTS}, cam,
                                  {k: g[b:b + 1] for k, g in c["upstream"].items()}, c["blur_size"])
        for k in whole:
            np.testing.assert_allclose(one[k], whole[k][b:b + 1], rtol=1e-12, atol=1e-14)
        for k in whole_g:
            np.testing.assert_allclose(one_g[k], whole_g[k][b:b + 1], rtol=1e-10, atol=1e-12)
