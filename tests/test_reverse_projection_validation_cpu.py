"""projection_reverse_renderer refuses what the kernels cannot index -- ValueError on the host, before the library is
loaded and before anything reaches the GPU (so these run without one)."""
import numpy as np
import pytest
import torch

from surf_renderer_amd import _lib, projection_reverse_renderer as project


@pytest.fixture(autouse=True)
def _no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def _camera(B, H, W, fovy, focal, hom=False):
    cam = {"eye": torch.tensor([[0.0, 0.5, 4.0]] * B), "at": torch.zeros(B, 3), "up": torch.tensor([[0.0, 1.0, 0.0]] * B),
           "viewport": [0, 0, W, H], "fovy": fovy, "focal_length": focal}
    if hom:
        cam["eye"] = torch.cat((cam["eye"], torch.ones(B, 1)), -1)
        cam["at"] = torch.cat((cam["at"], torch.ones(B, 1)), -1)
        cam["up"] = torch.cat((cam["up"], torch.zeros(B, 1)), -1)
    return cam


def _args(B=2, H=4, W=5, D=3, hom=False):
    g = torch.Generator().manual_seed(0)
    return {"rgb": torch.rand(B, H, W, D, generator=g), "in_pos_wc": torch.rand(B, H * W, 3, generator=g),
            "out_pos_wc": torch.rand(B, H * W, 3, generator=g), "camera1": _camera(B, H, W, 0.7, 0.5, hom),
            "camera2": _camera(B, H, W, 0.9, 0.8, hom)}


def _refused(match, **change):
    a = _args()
    a.update(change)
    with pytest.raises(ValueError, match=match):
        project(**a)


@pytest.mark.parametrize("shape", [(2, 20, 3), (4, 5, 3), (2, 4, 5), (2, 1, 4, 5, 3)])
def test_rgb_that_is_not_a_batch_of_images(shape):
    _refused("rgb", rgb=torch.zeros(shape))


@pytest.mark.parametrize("D", [0, 5, 8])
def test_a_channel_count_outside_one_to_four(D):
    _refused("channels", rgb=torch.zeros(2, 4, 5, D))


@pytest.mark.parametrize("key", ["in_pos_wc", "out_pos_wc"])
@pytest.mark.parametrize("shape", [(2, 20), (2, 20, 4), (20, 3), (2, 4, 5, 3), (2, 19, 3), (1, 20, 3)])
def test_positions_of_another_shape(key, shape):
    _refused(key, **{key: torch.zeros(shape)})


@pytest.mark.parametrize("shape", [(2, 20, 3), (2, 4, 5, 2), (1, 4, 5, 3), (2, 5, 4, 3)])
def test_a_rotated_image_unlike_rgb(shape):
    _refused("rotated_image", rotated_image=torch.zeros(shape))


@pytest.mark.parametrize("cam", ["camera1", "camera2"])
@pytest.mark.parametrize("viewport", [[0, 0, 4, 5], [0, 0, 5, 5], [0, 0, 6, 4], [0, 0, 0, 4], [3, 0, 2, 4], [0, 0, 5]])
def test_a_viewport_that_is_not_the_frame_of_rgb(cam, viewport):
    a = _args()
    _refused(cam + r".*viewport", **{cam: dict(a[cam], viewport=viewport)})


@pytest.mark.parametrize("cam", ["camera1", "camera2"])
@pytest.mark.parametrize("key", ["eye", "at", "up", "viewport", "fovy", "focal_length"])
def test_a_missing_camera_entry(cam, key):
    a = _args()
    c = dict(a[cam])
    del c[key]
    _refused(cam + r".*" + key, **{cam: c})


@pytest.mark.parametrize("cam", ["camera1", "camera2"])
@pytest.mark.parametrize("key", ["eye", "at", "up"])
@pytest.mark.parametrize("shape", [(3,), (2, 2), (2, 5), (1, 3), (2, 1, 3)])
def test_camera_vectors_of_another_shape(cam, key, shape):
    a = _args()
    _refused(cam + r".*" + key, **{cam: dict(a[cam], **{key: torch.ones(shape)})})


@pytest.mark.parametrize("cam", ["camera1", "camera2"])
def test_the_w_conventions_of_the_reference(cam):
    a = _args(hom=True)
    for key, w in (("up", 1.0), ("eye", 0.0), ("at", 0.0)):
        v = a[cam][key].clone()
        v[1, 3] = w
        a2 = dict(a, **{cam: dict(a[cam], **{key: v})})
        with pytest.raises(ValueError, match=f"{cam}.*{key}.*w"):
            project(**a2)


@pytest.mark.parametrize("cam", ["camera1", "camera2"])
def test_a_degenerate_camera(cam):
    a = _args()
    _refused(cam + ".*eye.*at", **{cam: dict(a[cam], at=a[cam]["eye"].clone())})
    _refused(cam + ".*up", **{cam: dict(a[cam], up=torch.zeros(2, 3))})
    _refused(cam + ".*up", **{cam: dict(a[cam], up=a[cam]["eye"] - a[cam]["at"])})
    _refused(cam + ".*eye", **{cam: dict(a[cam], eye=torch.full((2, 3), float("nan")))})


@pytest.mark.parametrize("cam", ["camera1", "camera2"])
@pytest.mark.parametrize("key,value", [("fovy", 0.0), ("fovy", 3.2), ("fovy", float("nan")), ("focal_length", 0.0),
                                       ("focal_length", -1.0), ("focal_length", float("inf"))])
def test_projection_scalars_out_of_range(cam, key, value):
    a = _args()
    _refused(cam + r".*" + key, **{cam: dict(a[cam], **{key: value})})


@pytest.mark.parametrize("cam", ["camera1", "camera2"])
@pytest.mark.parametrize("key", ["eye", "at", "up"])
def test_a_camera_that_requires_grad(cam, key):
    a = _args()
    _refused(cam + ".*requires grad", **{cam: dict(a[cam], **{key: a[cam][key].clone().requires_grad_(True)})})


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_a_depth_epsilon_that_is_not_finite(value):
    _refused("depth_epsilon", depth_epsilon=value)


@pytest.mark.parametrize("value", [-0.1, 1.0, 1.5, float("nan")])
def test_a_mask_dropout_outside_zero_to_one(value):
    _refused("mask_dropout", mask_dropout=value)


@pytest.mark.parametrize("key", ["rgb", "in_pos_wc", "out_pos_wc", "rotated_image"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.bool])
def test_a_non_float_input(key, dtype):
    a = _args()
    a["rotated_image"] = a["rgb"].clone()
    a[key] = a[key].to(dtype)
    with pytest.raises(ValueError, match="floating"):
        project(**a)
    a[key] = np.zeros(tuple(a[key].shape), dtype=np.int64)
    with pytest.raises(ValueError, match="floating"):
        project(**a)


def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for hom in (False, True):
        for dtype in (torch.float32, torch.float64, torch.float16):
            a = _args(hom=hom)
            with pytest.raises(RuntimeError, match="GPU"):
                project(a["rgb"].to(dtype), a["in_pos_wc"].to(dtype), a["out_pos_wc"], a["camera1"], a["camera2"],
                        rotated_image=a["rgb"], compute_new_depth=True, depth_epsilon=0.0, mask_dropout=0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        project(**_args(B=1, H=1, W=1, D=1))
