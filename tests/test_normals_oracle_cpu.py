"""tests/normals_oracle.py against the reference's own plane fit, recorded in float64 and in float32 (tests/golden/
normals/nm1_*.npz, tools/gen_normals_golden.py): normals and the gradient to pos, every element.

    restatement against ref64          1e-9 of each array's largest magnitude: the same function in the same precision,
                                       so only the order of fp64 sums differs
    ref32 against ref64                the array-scale tolerance (projection_checks.RTOL / ATOL_SCALE): the condition that
                                       the seeded cases are well-posed for the reference's own float32 arithmetic.  The
                                       kernels are held to one float32 rounding per entry (tests/entry_checks.py), which
                                       this float32 record does not meet (tests/test_entry_checks_cpu.py)
    restatement against splat_oracle.plane_fit_normals   1e-12: that one is pinned to the reference through p1_estimated_*
Also the conditions on every seeded case, and that a batch equals its views in the restatement."""
import glob
import os

import numpy as np
import pytest
import torch

import normals_cases as cases
import normals_oracle as no
import splat_oracle
from conftest import GOLDEN_DIR
from projection_checks import ATOL_SCALE, RTOL

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "normals", "nm1_*.npz")))
CAMERA = ("eye", "at", "up", "viewport", "fovy", "focal_length")
LARGEST_SIBLING = max(os.path.getsize(p) for d, pre in (("surfels", "sf1_"), ("hard_projection", "hp1_"))
                      for p in glob.glob(os.path.join(GOLDEN_DIR, d, pre + "*.npz")))


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "normals", name + ".npz"), allow_pickle=False)


def _camera(npz):
    return {k: npz["in/camera/" + k] for k in CAMERA}


def test_the_fixtures_are_there():
    assert FIXTURES == sorted("nm1_" + cases.tag(n, v) for n, v in cases.ALL)
    for name in FIXTURES:
        npz = _load(name)
        assert npz["in/pos"].dtype == np.float32 and npz["grad_in/normal"].dtype == np.float32
        for k in ("normal", "grad/pos"):
            assert npz["ref64/" + k].dtype == np.float64 and npz["ref32/" + k].dtype == np.float32, (name, k)
            assert npz["ref64/" + k].shape == npz["ref32/" + k].shape == npz["in/pos"].shape, (name, k)
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "normals", name + ".npz")) <= LARGEST_SIBLING, name


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_a_fixture_holds_the_inputs_of_its_seeded_case(name, variant):
    npz, c = _load("nm1_" + cases.tag(name, variant)), cases.case(name, variant)
    assert c["pos"].dtype == np.float32 and np.array_equal(npz["in/pos"], c["pos"])
    assert npz["in/pos"].shape == c["pos"].shape and str(npz["in/frame"]) == c["frame"]
    for k in CAMERA:
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert np.array_equal(npz["grad_in/normal"], c["upstream"]["normal"])


@pytest.mark.parametrize("name", FIXTURES)
def test_the_restatement_matches_the_float64_reference(name):
    npz = _load(name)
    values, grads = no.gradients({"pos": npz["in/pos"]}, _camera(npz), {"normal": npz["grad_in/normal"]},
                                 str(npz["in/frame"]))
    for k, got in (("normal", values["normal"]), ("grad/pos", grads["pos"])):
        want = npz["ref64/" + k]
        assert want.shape == got.shape and np.all(np.isfinite(want)), (name, k)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name} {k}: max|ref64 - restatement| / max|ref64| = {err:.3g}")
        assert err <= 1e-9, (name, k, err)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_float32_reference_meets_the_stated_tolerance(name):
    npz = _load(name)
    for k in ("normal", "grad/pos"):
        got, want = npz["ref32/" + k].astype(np.float64), npz["ref64/" + k]
        scale = max(np.abs(want).max(), 1.0) if k == "normal" else np.abs(want).max()
        share = (np.abs(got - want) / (ATOL_SCALE * scale + RTOL * np.abs(want))).max()
        print(f"{name} {k}: the reference's float32 error is {share:.3g} of the tolerance")
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL_SCALE * scale, err_msg=f"{name} {k}")


def test_the_unbatched_reference_function_equals_the_batched_one_bit_for_bit_in_float64():
    npz = _load("nm1_" + cases.UNBATCHED)
    for k in ("normal", "grad/pos"):
        assert np.array_equal(npz["ref64/unbatched/" + k], npz["ref64/" + k]), k
        assert npz["ref32/unbatched/" + k].dtype == np.float32
        np.testing.assert_allclose(npz["ref32/unbatched/" + k].astype(np.float64), npz["ref64/" + k], rtol=RTOL,
                                   atol=ATOL_SCALE * max(np.abs(npz["ref64/" + k]).max(), 1.0), err_msg=k)
    assert [n for n in FIXTURES if "ref64/unbatched/normal" in _load(n).files] == ["nm1_" + cases.UNBATCHED]


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_restatement_equals_the_splat_oracles_plane_fit(name):
    c = cases.case(name)
    pos = torch.tensor(c["pos"].astype(np.float64))
    got = no.plane_fit(pos)
    for b in range(c["shape"][0]):
        want = splat_oracle.plane_fit_normals(pos[b])
        np.testing.assert_allclose(got[b].numpy(), want.numpy(), rtol=0, atol=1e-12, err_msg=f"{name} view {b}")


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_drawn_input_meets_the_conditions(name):
    c = cases.case(name)
    B, H, W = c["shape"]
    assert c["pos"].shape == (B, H, W, 3) and H >= 2 and W >= 2
    depth = -c["pos"][..., 2].astype(np.float64)
    assert np.all(np.abs(depth - 3.0) <= 0.5 + cases.NOISE + 1e-6)            # 3 + smooth (at most 0.5) + noise
    v, g = cases.expected(name)
    assert np.all(v["normal"][..., 2] > 0) if c["frame"] == "camera" else True
    np.testing.assert_allclose(np.linalg.norm(v["normal"], axis=-1), 1.0, rtol=0, atol=1e-9)
    up = c["upstream"]["normal"]
    assert np.array_equal(up * 64, np.round(up * 64)) and np.abs(up).max() <= 1.0
    if name in cases.UNSEEN_ROWS:
        r0, r1 = cases.UNSEEN_ROWS[name]
        assert np.all(up[:, r0:r1] == 0) and np.all(g["pos"][:, r0 + 1:r1 - 1] == 0)
        assert np.all(np.abs(g["pos"][:, r0 - 1]).max(-1) > 0) and np.all(np.abs(g["pos"][:, r1]).max(-1) > 0)
    else:
        assert np.all(np.abs(g["pos"]).max(-1) > 0)
    assert cases.case("36x48")["shape"][1] * cases.case("36x48")["shape"][2] > 4 * 256          # several workgroups
    assert cases.case("36x48")["shape"][1] * cases.case("36x48")["shape"][2] % 256               # the last one ragged


def test_the_flat_variant_is_the_same_points_and_the_world_case_is_the_rotated_camera_frame():
    c, f = cases.case("12x16"), cases.case("12x16", "flat")
    assert f["pos"].shape == (2, 12 * 16, 3) and np.array_equal(f["pos"].reshape(c["pos"].shape), c["pos"])
    (v, g), (vf, gf) = cases.expected("12x16"), cases.expected("12x16", "flat")
    assert np.array_equal(v["normal"].reshape(vf["normal"].shape), vf["normal"])
    assert np.array_equal(g["pos"].reshape(gf["pos"].shape), gf["pos"])
    w = cases.case("17x9")
    assert w["frame"] == "world"
    cam, _ = no.gradients({"pos": w["pos"]}, None, w["upstream"], "camera")
    R = no.rotation(w["camera"], 3).numpy()
    np.testing.assert_allclose(np.einsum("brc,bhwc->bhwr", R, cam["normal"]), cases.expected("17x9")[0]["normal"],
                               rtol=0, atol=1e-14)
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), (3, 3, 3)), rtol=0, atol=1e-9)


def test_a_batch_is_its_views():
    for name in ("12x16", "17x9"):
        c = cases.case(name)
        whole, whole_g = cases.expected(name)
        for b in range(c["shape"][0]):
            camera = dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in ("eye", "at", "up")})
            one, one_g = no.gradients({"pos": c["pos"][b:b + 1]}, camera, {"normal": c["upstream"]["normal"][b:b + 1]},
                                      c["frame"])
            np.testing.assert_allclose(one["normal"], whole["normal"][b:b + 1], rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(one_g["pos"], whole_g["pos"][b:b + 1], rtol=1e-10, atol=1e-12)
