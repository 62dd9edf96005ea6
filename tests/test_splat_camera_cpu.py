"""camera_grad of the two splat renderers, without a GPU: the fp64 restatement with camera leaves
(tests/splat_camera_oracle.py) against the reference's float64 record (tests/golden/splat_camera/sc1_*.npz), the
fixtures' own promises, and the host-side validation of the keyword, which runs before anything reaches the GPU."""
import glob
import os

import numpy as np
import pytest
import torch

import splat_camera_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splat_camera")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "sc1_*.npz")))
WANTED = {"ar_2x2", "ar_3x5", "ar_3x5_lw", "ar_12x16_s2", "ar_17x9_b3_quartic", "ar_36x48", "ndc_1x1", "ndc_2x2",
          "ndc_3x5_ds_quartic", "ndc_3x5_l1", "ndc_17x9_b3", "ndc_36x48"}


def test_the_fixtures_are_the_issue_s_cases_and_small():
    assert set(CASES) == WANTED
    top = max(os.path.getsize(p) for p in glob.glob(os.path.join(os.path.dirname(GOLDEN), "*.npz")))
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"sc1_{name}.npz")) < top, name


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_float64_record(name):
    kind, scene, kw, g_image, grads, meta = oracle.load(os.path.join(GOLDEN, f"sc1_{name}.npz"))
    got = oracle.batch_gradients(kind, scene, g_image, **kw)
    for k in oracle.CAMERA_LEAVES:
        want = grads["64"][k]
        assert got[k].shape == want.shape, k
        big = np.abs(want).max()
        assert big > 0, k                                                    # the reference's gradient is real
        assert np.abs(got[k] - want).max() <= 1e-9 * big, (name, k, np.abs(got[k] - want).max() / big)
        assert np.all(got[k][..., 3:] == 0) and np.all(want[..., 3:] == 0)   # the reference slices [:3]
        # the float32 record is within a quarter of the tolerance the GPU tests give it
        assert np.abs(grads["32"][k] - want).max() <= 0.25 * 3e-3 * max(big, 1e-6), k


def test_a_light_with_w_other_than_one_is_among_the_cases():
    for name in ("ar_3x5_lw", "ndc_3x5_l1"):
        _, scene, *_ = oracle.load(os.path.join(GOLDEN, f"sc1_{name}.npz"))
        w = np.asarray(scene["lights"]["pos"])[..., 3]
        assert np.any(w != 1.0), name
    _, scene, *_ = oracle.load(os.path.join(GOLDEN, "sc1_ar_3x5_lw.npz"))
    assert set(np.asarray(scene["lights"]["pos"])[:, 3]) == {0.5, 0.0}


def _scene(kind, leaf=None, dtype=torch.float32):
    _, scene, kw, *_ = oracle.load(os.path.join(GOLDEN, "sc1_ar_3x5.npz" if kind == "along_ray" else "sc1_ndc_2x2.npz"))
    scene = dict(scene, camera=dict(scene["camera"]))
    if leaf:
        scene["camera"][leaf] = torch.tensor(np.asarray(scene["camera"][leaf]), dtype=dtype, requires_grad=True)
    return scene


def _entry(kind, batched=False):
    import surf_renderer_amd as S
    return {("along_ray", False): S.render_splats_along_ray, ("along_ray", True): S.render_splats_along_ray_batch,
            ("ndc", False): S.render_splats_NDC, ("ndc", True): S.render_splats_NDC_batch}[kind, batched]


def _batch(scene):
    disk = scene["objects"]["disk"]
    return dict(scene, objects={"disk": dict(disk, pos=np.asarray(disk["pos"])[None])})


@pytest.mark.parametrize("kind", ["along_ray", "ndc"])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("value", [1, 0, None, "yes", 1.0, np.bool_(True)])
def test_camera_grad_must_be_a_bool(kind, batched, value):
    scene = _scene(kind)
    with pytest.raises(ValueError, match="camera_grad"):
        _entry(kind, batched)(_batch(scene) if batched else scene, camera_grad=value)


@pytest.mark.parametrize("kind,key", [("along_ray", "fovy"), ("along_ray", "focal_length"), ("along_ray", "viewport"),
                                      ("along_ray", "far"), ("ndc", "fovy"), ("ndc", "near"), ("ndc", "far"),
                                      ("ndc", "viewport")])
def test_only_eye_at_and_up_may_require_grad(kind, key):
    scene = _scene(kind)
    scene["camera"][key] = torch.tensor(np.asarray(scene["camera"][key], dtype=np.float64), requires_grad=True)
    for flag in (True, False):
        with pytest.raises(ValueError, match=f"camera\\['{key}'\\] requires grad"):
            _entry(kind)(scene, camera_grad=flag)


@pytest.mark.parametrize("kind", ["along_ray", "ndc"])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("leaf", ["eye", "at", "up"])
def test_a_leaf_without_the_keyword_is_still_refused(kind, batched, leaf):
    scene = _scene(kind, leaf)
    scene = _batch(scene) if batched else scene
    for kw in ({}, {"camera_grad": False}):
        with pytest.raises(ValueError, match=f"camera\\['{leaf}'\\] requires grad"):
            _entry(kind, batched)(scene, **kw)


@pytest.mark.parametrize("kind", ["along_ray", "ndc"])
def test_with_the_keyword_the_leaf_passes_validation(kind):
    """Past the camera checks the call stops only for want of a GPU."""
    if torch.cuda.is_available():
        assert "image" in _entry(kind)(_scene(kind, "eye"), camera_grad=True)
    else:
        with pytest.raises(RuntimeError, match="needs a GPU"):
            _entry(kind)(_scene(kind, "eye"), camera_grad=True)


def test_camera_matrices_are_the_reference_s_lookat_attached_to_the_leaves():
    from surf_renderer_amd._camera import view_matrices
    from surf_renderer_amd.splats import camera_matrices
    cam = {"eye": torch.tensor([[0.5, 1.0, 6.0, 1.0], [0.75, 0.5, 6.125, 1.0]], requires_grad=True),
           "at": torch.tensor([0.125, -0.25, 0.0, 1.0], dtype=torch.float64, requires_grad=True),
           "up": np.array([0.25, 1.0, 0.375, 0.0], np.float32)}
    M = camera_matrices(cam, 2, "cpu")
    assert M.shape == (2, 3, 4) and M.dtype == torch.float64 and M.requires_grad
    want = view_matrices(cam["eye"].detach().double()[:, :3], cam["at"].detach()[None, :3].expand(2, 3),
                         torch.from_numpy(cam["up"].astype(np.float64))[None, :3].expand(2, 3))
    assert torch.equal(M.detach(), want)
    M.sum().backward()
    assert cam["eye"].grad.shape == (2, 4) and cam["eye"].grad.dtype == torch.float32
    assert torch.all(cam["eye"].grad[:, 3] == 0) and torch.any(cam["eye"].grad[:, :3] != 0)
    assert cam["at"].grad.shape == (4,) and cam["at"].grad.dtype == torch.float64 and cam["at"].grad[3] == 0
    assert camera_matrices({k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in cam.items()}, 2, "cpu") is None
