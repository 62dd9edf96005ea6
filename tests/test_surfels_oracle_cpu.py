"""tests/surfels_oracle.py against the reference's own depth lift, recorded in float64 and in float32 (tests/golden/
surfels/sf1_*.npz, tools/gen_surfels_golden.py): positions and the gradient to depth, every element.

    restatement, grid="torch", against ref64     1e-9 of each array's largest magnitude: the same function in the same
                                                 precision on the same float32 grid, so only the order of fp64 sums differs
    restatement grid="numpy" against grid="torch"   the pixel grids differ by at most surfels_oracle.GRID_BOUND = 4 * 2^-24
                                                 of the half extent, and the positions by what that moves them
    ref32 against ref64                          the array-scale tolerance (projection_checks.RTOL / ATOL_SCALE): the seeded
                                                 cases are well-posed for the reference's own float32 arithmetic.  The
                                                 kernels are held to one float32 rounding per entry (tests/entry_checks.py),
                                                 which this float32 record does not meet (tests/test_entry_checks_cpu.py)
Also the conditions on every seeded case, and that a batch equals its views in the restatement."""
import glob
import os

import numpy as np
import pytest

import surfels_cases as cases
import surfels_oracle as so
from conftest import GOLDEN_DIR
from projection_checks import ATOL_SCALE, RTOL

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "surfels", "sf1_*.npz")))
CAMERA = ("eye", "at", "up", "viewport", "fovy", "focal_length")


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "surfels", name + ".npz"), allow_pickle=False)


def _camera(npz):
    return {k: npz["in/camera/" + k] for k in CAMERA}


def test_the_fixtures_are_there():
    assert FIXTURES == sorted("sf1_" + cases.tag(n, v) for n, v in cases.ALL)
    for name in FIXTURES:
        npz = _load(name)
        assert npz["in/depth"].dtype == np.float32 and npz["grad_in/pos"].dtype == np.float32
        for k in ("pos", "grad/depth"):
            assert npz["ref64/" + k].dtype == np.float64 and npz["ref32/" + k].dtype == np.float32, (name, k)


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_a_fixture_holds_the_inputs_of_its_seeded_case(name, variant):
    npz, c = _load("sf1_" + cases.tag(name, variant)), cases.case(name, variant)
    assert c["depth"].dtype == np.float32 and np.array_equal(npz["in/depth"], c["depth"])
    assert npz["in/depth"].shape == c["depth"].shape and str(npz["in/frame"]) == c["frame"]
    for k in CAMERA:
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert np.array_equal(npz["grad_in/pos"], c["upstream"]["pos"])


@pytest.mark.parametrize("name", FIXTURES)
def test_the_restatement_on_the_torch_grid_matches_the_float64_reference(name):
    npz = _load(name)
    values, grads = so.gradients({"depth": npz["in/depth"]}, _camera(npz), {"pos": npz["grad_in/pos"]},
                                 str(npz["in/frame"]), grid="torch")
    for k, got in (("pos", values["pos"]), ("grad/depth", grads["depth"])):
        want = npz["ref64/" + k]
        assert want.shape == got.shape and np.all(np.isfinite(want)), (name, k)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name} {k}: max|ref64 - restatement| / max|ref64| = {err:.3g}")
        assert err <= 1e-9, (name, k, err)
    dead = npz["in/depth"].reshape(want.shape) <= 0
    assert dead.any() or dead.size == 1
    assert np.all(grads["depth"][dead] == 0) and np.all(npz["ref64/grad/depth"][dead] == 0)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_float32_reference_meets_the_stated_tolerance(name):
    npz = _load(name)
    for k in ("pos", "grad/depth"):
        got, want = npz["ref32/" + k].astype(np.float64), npz["ref64/" + k]
        scale = max(np.abs(want).max(), 1.0) if k == "pos" else np.abs(want).max()
        share = (np.abs(got - want) / (ATOL_SCALE * scale + RTOL * np.abs(want))).max()
        print(f"{name} {k}: the reference's float32 error is {share:.3g} of the tolerance")
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL_SCALE * scale, err_msg=f"{name} {k}")


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_the_two_grids_differ_by_no_more_than_the_bound(name, variant):
    c = cases.case(name, variant)
    half = so.frame_extent(c["camera"])
    for axis, (a, b) in enumerate(zip(so.pixel_grid(c["camera"], "numpy"), so.pixel_grid(c["camera"], "torch"))):
        assert a.shape == b.shape == (c["shape"][2 - axis],)
        assert np.array_equal(a, a.astype(np.float32)) and np.array_equal(b, b.astype(np.float32))
        print(f"{cases.tag(name, variant)} axis {axis}: {np.abs(a - b).max() / half[axis] * 2 ** 24:.3g} x 2^-24")
        assert np.abs(a - b).max() <= so.GRID_BOUND * half[axis]
    # and the positions by what the grid moves them: |d| / f times the bound per camera-space component, which the
    # rotation into the world frame spreads over at most sqrt(2) of it
    f = c["camera"]["focal_length"]
    reach = np.abs(c["depth"]).max() / f * so.GRID_BOUND * max(half) * np.sqrt(2.0)
    (v_np, g_np), (v_t, g_t) = cases.expected(name, variant, "numpy"), cases.expected(name, variant, "torch")
    assert np.abs(v_np["pos"] - v_t["pos"]).max() <= reach
    assert np.abs(g_np["depth"] - g_t["depth"]).max() <= reach / np.abs(c["depth"]).max() * np.sqrt(3.0)


def test_a_single_sample_is_the_start_point():
    for name, axis in (("1x1", 0), ("1x1", 1), ("1x4", 1), ("4x1", 0)):
        c = cases.case(name)
        half = so.frame_extent(c["camera"])
        for grid in ("numpy", "torch"):
            got = so.pixel_grid(c["camera"], grid)[axis]
            assert got.shape == (1,) and got[0] == np.float32((-1.0, 1.0)[axis] * half[axis]), (name, axis, grid)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_drawn_input_meets_the_conditions(name):
    c = cases.case(name)
    B, H, W = c["shape"]
    d = c["depth"].reshape(B, H * W)
    assert np.all(np.abs(d[d != 0]) >= 1e-3)
    if H * W > 1:
        for b in range(B):
            assert (d[b] <= 0).sum() * 8 >= H * W and (d[b] == 0).any() and (d[b] < 0).any()
        v, g = cases.expected(name)
        eye = np.asarray(c["camera"]["eye"], dtype=np.float64)[:, None, :3]
        assert np.array_equal(v["pos"][d <= 0], np.broadcast_to(eye, v["pos"].shape)[d <= 0])    # the point is the eye
        assert np.all(g["depth"].reshape(B, H * W)[d <= 0] == 0) and np.all(g["depth"].reshape(B, H * W)[d > 0] != 0)
    assert cases.case("36x48")["shape"][1] * cases.case("36x48")["shape"][2] > 4 * 256           # several workgroups


def test_the_three_depth_shapes_are_all_used_and_the_camera_variant_is_the_camera_frame():
    assert {cases.case(n)["depth"].ndim for n in cases.NAMES} == {2, 3, 4}
    c = cases.case("12x16", "camera")
    v, _ = cases.expected("12x16", "camera")
    np.testing.assert_array_equal(v["pos"][..., 2], -np.maximum(c["depth"].reshape(2, -1).astype(np.float64), 0.0))
    R, eye = so.camera_to_world(c["camera"])
    world = v["pos"] @ R.numpy().transpose(0, 2, 1) + eye.numpy()[:, None]
    np.testing.assert_allclose(world, cases.expected("12x16")[0]["pos"], rtol=0, atol=1e-14)


def test_a_batch_is_its_views():
    for name in ("12x16", "17x9"):
        c = cases.case(name)
        whole, whole_g = cases.expected(name)
        for b in range(c["shape"][0]):
            camera = dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in ("eye", "at", "up")})
            one, one_g = so.gradients({"depth": c["depth"][b:b + 1]}, camera, {"pos": c["upstream"]["pos"][b:b + 1]})
            np.testing.assert_allclose(one["pos"], whole["pos"][b:b + 1], rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(one_g["depth"], whole_g["depth"][b:b + 1], rtol=1e-10, atol=1e-12)
