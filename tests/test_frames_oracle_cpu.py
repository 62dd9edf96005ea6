"""tests/frames_oracle.py against the reference's own frame transforms and point projection, recorded in float64 and
in float32 (tests/golden/frames/fr1_*.npz, tools/gen_frames_golden.py):

    restatement against ref64      values and every gradient, the camera's included, to 1e-12 of each array's largest
                                   magnitude: the same function in the same precision
    restatement against ref32      the array-scale tolerance (projection_checks.RTOL / ATOL_SCALE): the condition that the
                                   seeded cases are well-posed for the reference's own float32 arithmetic.  It is NOT what
                                   the kernels are held to: they meet one float32 rounding per entry (tests/entry_checks.py),
                                   which this float32 record breaks on 45 % of its entries
                                   (tests/test_entry_checks_cpu.py)
    px_idx                         equal to both runs on EVERY surfel: the seeded surfels keep 1e-3 px from every rounding
                                   boundary (frames_cases), which this also shows to hold for the committed inputs
Also that a fixture holds its seeded case's inputs, that the unbatched functions give the batched ones' values, that a
batch equals its views in the restatement, and the size cap of the fixtures."""
import glob
import os

import numpy as np
import pytest
import torch

import frames_cases as cases
import frames_oracle as fo
from conftest import GOLDEN_DIR
from projection_checks import ATOL_SCALE, RTOL

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "frames", "fr1_*.npz")))
TRANSFORMS = [(n, d) for n in cases.GOLDEN_TRANSFORM for d in cases.DIRECTIONS]
VIEW_KEYS = ("eye", "at", "up")


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "frames", name + ".npz"), allow_pickle=False)


def _camera(npz):
    return {k[len("in/camera/"):]: npz[k] for k in npz.files if k.startswith("in/camera/")}


def _close64(got, want, tag):
    assert got.shape == want.shape and want.dtype == np.float64 and np.all(np.isfinite(want)), tag
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / (scale if scale > 0 else 1.0)
    print(f"{tag}: max|ref64 - restatement| / max|ref64| = {err:.3g}")
    assert err <= 1e-12, (tag, err)


def _close32(ref32, want, tag):
    assert ref32.dtype == np.float32 and ref32.shape == want.shape, tag
    np.testing.assert_allclose(ref32.astype(np.float64), want, rtol=RTOL, atol=ATOL_SCALE * max(np.abs(want).max(), 1.0),
                               err_msg=tag)


def test_the_fixtures_are_there_and_small():
    assert FIXTURES == sorted([f"fr1_{n}_{d}" for n, d in TRANSFORMS] + ["fr1_" + n for n in cases.GOLDEN_PROJECT])
    cap = max(os.path.getsize(p) for sub in ("surfels", "hard_projection")
              for p in glob.glob(os.path.join(GOLDEN_DIR, sub, "*.npz")))
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "frames", name + ".npz")) <= cap, name


@pytest.mark.parametrize("name,direction", TRANSFORMS)
def test_a_transform_fixture_matches_the_restatement(name, direction):
    npz, c = _load(f"fr1_{name}_{direction}"), cases.transform_case(name)
    for k in ("pos", "normal"):
        assert (c[k] is None) == ("in/" + k not in npz.files)
        if c[k] is not None:
            assert npz["in/" + k].dtype == np.float32 and np.array_equal(npz["in/" + k], c[k])
            assert np.array_equal(npz["grad_in/" + k], c["upstream"][k])
    camera = _camera(npz)
    assert set(camera) == set(VIEW_KEYS) and all(np.array_equal(camera[k], c["camera"][k]) for k in VIEW_KEYS)
    values, grads, cam_grads = fo.transform_gradients(direction, {k: c[k] for k in ("pos", "normal")}, camera,
                                                      {k: npz["grad_in/" + k] for k in c["upstream"]})
    assert set(values) == set(c["upstream"])
    for k, v in values.items():
        tag = f"{name} {direction} {k}"
        _close64(v, npz["ref64/" + k], tag)
        _close64(grads[k], npz["ref64/grad/" + k], tag + " grad")
        _close32(npz["ref32/" + k], v, tag + " ref32")
        if "ref64/one/" + k in npz.files:             # the unbatched function on the one view
            _close64(v[0], npz["ref64/one/" + k], tag + " unbatched")
            _close32(npz["ref32/one/" + k], v[0], tag + " unbatched ref32")
    assert ("ref64/one/" + next(iter(values)) in npz.files) == (camera["eye"].shape[0] == 1)
    if "pos" in values:
        w = c["pos"][..., 3] if c["pos"].shape[-1] == 4 else np.ones(c["pos"].shape[:2])
        assert values["pos"].shape[-1] == 4 and np.array_equal(values["pos"][..., 3], w)
    if "normal" in grads and c["normal"].shape[-1] == 4:
        assert np.all(grads["normal"][..., 3] == 0)
    for k in VIEW_KEYS:
        _close64(cam_grads[k], npz["ref64/grad/camera/" + k], f"{name} {direction} camera {k}")
        if cam_grads[k].shape[-1] == 4:
            assert np.all(cam_grads[k][..., 3] == 0)


@pytest.mark.parametrize("name", cases.GOLDEN_PROJECT)
def test_a_projection_fixture_matches_the_restatement(name):
    npz, c = _load("fr1_" + name), cases.project_case(name)
    assert npz["in/surfels"].dtype == np.float32 and np.array_equal(npz["in/surfels"], c["surfels"])
    camera = _camera(npz)
    assert set(camera) == set(c["camera"])
    assert all(np.array_equal(camera[k], np.asarray(c["camera"][k])) for k in camera)
    W, H = c["frame"]
    for coords, out in ((False, "plane"), (True, "px_coord")):
        assert np.array_equal(npz["grad_in/" + out], c["upstream"][out])
        values, grads, cam_grads = fo.project_gradients(coords, c["surfels"], camera, {out: npz["grad_in/" + out]})
        tag = f"{name} {out}"
        _close64(values[out], npz["ref64/" + out], tag)
        _close32(npz["ref32/" + out], values[out], tag + " ref32")
        _close64(grads["surfels"], npz[f"ref64/grad_{out}/surfels"], tag + " grad surfels")
        for k in VIEW_KEYS:
            _close64(cam_grads[k], npz[f"ref64/grad_{out}/camera/{k}"], f"{tag} camera {k}")
        if coords:
            idx = values["px_idx"]
            assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() <= W * H
            # no surfel is excluded: the float64 run, the float32 run and the restatement name the same pixel
            assert np.array_equal(idx, npz["ref64/px_idx"]) and np.array_equal(idx, npz["ref32/px_idx"])
            if idx.size >= 16:
                assert (idx == W * H).any() and (idx < W * H).any()
    assert cases.boundary_distance(c["surfels"], c["camera"]).min() >= cases.MARGIN


@pytest.mark.parametrize("name", cases.PROJECT)
def test_every_seeded_surfel_keeps_its_margin_and_every_side_is_missed(name):
    c = cases.project_case(name)
    W, H = c["frame"]
    assert cases.boundary_distance(c["surfels"], c["camera"]).min() >= cases.MARGIN
    _, px = fo.project_image_coordinates(torch.as_tensor(c["surfels"].astype(np.float64)), c["camera"])
    x, y, depth = (px[..., k].numpy() for k in range(3))
    if x.size >= 16:
        for side in (x < 0, x > W, y < 0, y > H, depth < 0):
            assert side.any()


def test_a_batch_equals_its_views_in_the_restatement():
    c = cases.transform_case("t153_b3")
    whole = fo.transform_gradients("to_world", cases.transform_inputs(c), c["camera"], c["upstream"])
    for b in range(3):
        one = fo.transform_gradients("to_world", {k: c[k][b:b + 1] for k in ("pos", "normal")},
                                     {k: v[b:b + 1] for k, v in c["camera"].items()},
                                     {k: u[b:b + 1] for k, u in c["upstream"].items()})
        for x, y in zip(whole, one):
            for k in y:
                np.testing.assert_allclose(x[k][b:b + 1], y[k], rtol=1e-13, atol=1e-13)
