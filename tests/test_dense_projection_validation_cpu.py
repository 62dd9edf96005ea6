"""projection_renderer_differentiable refuses what the kernels cannot index -- ValueError on the host, before the
library is loaded and before anything reaches the GPU (so these run without one)."""
import numpy as np
import pytest
import torch

from surf_renderer_amd import _lib, projection_renderer_differentiable as project


@pytest.fixture(autouse=True)
def _no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def _args(B=2, H=4, W=5, D=3, hom=False):
    g = torch.Generator().manual_seed(0)
    cam = {"eye": torch.tensor([[0.0, 0.5, 4.0]] * B), "at": torch.zeros(B, 3), "up": torch.tensor([[0.0, 1.0, 0.0]] * B),
           "viewport": [0, 0, W, H], "fovy": 0.7, "focal_length": 0.5}
    if hom:
        cam["eye"] = torch.cat((cam["eye"], torch.ones(B, 1)), -1)
        cam["at"] = torch.cat((cam["at"], torch.ones(B, 1)), -1)
        cam["up"] = torch.cat((cam["up"], torch.zeros(B, 1)), -1)
    return {"surfels": torch.rand(B, H * W, 3, generator=g), "rgb": torch.rand(B, H, W, D, generator=g), "camera": cam}


def _refused(match, **change):
    a = _args()
    a.update(change)
    with pytest.raises(ValueError, match=match):
        project(**a)


@pytest.mark.parametrize("shape", [(2, 20), (2, 20, 4), (20, 3), (2, 4, 5, 3)])
def test_surfels_of_another_shape(shape):
    _refused("surfels", surfels=torch.zeros(shape))


@pytest.mark.parametrize("n", [19, 21, 25])
def test_a_surfel_count_that_is_not_the_frame(n):
    _refused("W x H", surfels=torch.zeros(2, n, 3))


@pytest.mark.parametrize("shape", [(2, 20), (3, 20, 3), (2, 5, 4, 3), (2, 21, 3), (20, 3), (2, 4, 5)])
def test_rgb_of_another_shape(shape):
    _refused("rgb", rgb=torch.zeros(shape))


@pytest.mark.parametrize("D", [0, 5, 8])
def test_a_channel_count_outside_one_to_four(D):
    _refused("channels", rgb=torch.zeros(2, 20, D))


@pytest.mark.parametrize("shape", [(2, 20, 3), (2, 4, 5, 2), (1, 4, 5, 3)])
def test_a_rotated_image_unlike_rgb(shape):
    _refused("rotated_image", rotated_image=torch.zeros(shape))


def test_an_empty_batch():
    a = _args()
    a["camera"] = dict(a["camera"], eye=torch.zeros(0, 3), at=torch.zeros(0, 3), up=torch.zeros(0, 3))
    with pytest.raises(ValueError, match="empty"):
        project(torch.zeros(0, 20, 3), torch.zeros(0, 20, 3), a["camera"])


@pytest.mark.parametrize("viewport", [[0, 0, 0, 4], [0, 0, 5, 0], [3, 0, 2, 4], [0, 0, 5]])
def test_an_empty_or_malformed_viewport(viewport):
    a = _args()
    _refused("viewport", camera=dict(a["camera"], viewport=viewport))


@pytest.mark.parametrize("blur_size", [0.0, -0.15, float("nan"), float("inf")])
def test_a_blur_size_that_is_not_positive_and_finite(blur_size):
    _refused("blur_size", blur_size=blur_size)


def test_any_positive_blur_size_passes_the_checks(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for blur_size in (1e-6, 0.15, 1e6):              # sigma has no upper limit here: there is no tap table to fill
        with pytest.raises(RuntimeError, match="GPU"):
            project(**_args(), blur_size=blur_size)


@pytest.mark.parametrize("key", ["eye", "at", "up", "viewport", "fovy", "focal_length"])
def test_a_missing_camera_entry(key):
    a = _args()
    cam = dict(a["camera"])
    del cam[key]
    _refused(key, camera=cam)


@pytest.mark.parametrize("key", ["eye", "at", "up"])
@pytest.mark.parametrize("shape", [(3,), (2, 2), (2, 5), (1, 3), (2, 1, 3)])
def test_camera_vectors_of_another_shape(key, shape):
    a = _args()
    _refused(key, camera=dict(a["camera"], **{key: torch.ones(shape)}))


def test_the_w_conventions_of_the_reference():
    a = _args(hom=True)
    for key, w in (("up", 1.0), ("eye", 0.0), ("at", 0.0)):
        v = a["camera"][key].clone()
        v[1, 3] = w
        _refused(f"{key}.*w", camera=dict(a["camera"], **{key: v}))


def test_a_degenerate_camera():
    a = _args()
    _refused("eye.*at", camera=dict(a["camera"], at=a["camera"]["eye"].clone()))
    _refused("up", camera=dict(a["camera"], up=torch.zeros(2, 3)))
    _refused("up", camera=dict(a["camera"], up=a["camera"]["eye"] - a["camera"]["at"]))
    _refused("eye", camera=dict(a["camera"], eye=torch.full((2, 3), float("nan"))))


@pytest.mark.parametrize("key,value", [("fovy", 0.0), ("fovy", 3.2), ("fovy", float("nan")), ("focal_length", 0.0),
                                       ("focal_length", -1.0), ("focal_length", float("inf"))])
def test_projection_scalars_out_of_range(key, value):
    a = _args()
    _refused(key, camera=dict(a["camera"], **{key: value}))


@pytest.mark.parametrize("key", ["eye", "at", "up"])
def test_a_camera_that_requires_grad(key):
    a = _args()
    _refused("requires grad", camera=dict(a["camera"], **{key: a["camera"][key].clone().requires_grad_(True)}))


@pytest.mark.parametrize("key", ["surfels", "rgb", "rotated_image"])
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
                project(a["surfels"].to(dtype), a["rgb"].to(dtype).reshape(2, 20, 3), a["camera"],
                        rotated_image=a["rgb"].reshape(2, 20, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        project(**_args(B=1, H=1, W=1, D=1))
