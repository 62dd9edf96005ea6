"""projection_renderer refuses what the kernels cannot index -- ValueError on the host, before the library is loaded and
before anything reaches the GPU (so these run without one).  The camera checks it shares with the other re-projection
layers are those of tests/projection_validation.py; the layer has no rotated image and no blur, so its own follow."""
import numpy as np
import pytest
import torch

from projection_validation import camera, camera_tests, refused
from projection_validation import cam, no_library  # noqa: F401  (fixtures)
from surf_renderer_amd import projection_renderer as project


def _args(B=2, H=4, W=5, D=3, hom=False):
    g = torch.Generator().manual_seed(0)
    return {"surfels": torch.rand(B, H * W, 3, generator=g), "rgb": torch.rand(B, H, W, D, generator=g),
            "camera": camera(B, H, W, hom=hom)}


globals().update(camera_tests(project, _args))


@pytest.mark.parametrize("shape", [(2, 20), (2, 20, 4), (20, 3), (2, 4, 5, 3)])
def test_surfels_of_another_shape(shape):
    refused(project, _args, "surfels", surfels=torch.zeros(shape))


@pytest.mark.parametrize("n", [19, 21, 25])
def test_a_surfel_count_that_is_not_the_frame(n):
    refused(project, _args, "W x H", surfels=torch.zeros(2, n, 3))


@pytest.mark.parametrize("shape", [(2, 20), (3, 20, 3), (2, 5, 4, 3), (2, 21, 3), (20, 3), (2, 4, 5)])
def test_rgb_of_another_shape(shape):
    refused(project, _args, "rgb", rgb=torch.zeros(shape))


@pytest.mark.parametrize("D", [0, 5, 8])
def test_a_channel_count_outside_one_to_four(D):
    refused(project, _args, "channels", rgb=torch.zeros(2, 20, D))


def test_an_empty_batch():
    c = dict(_args()["camera"], eye=torch.zeros(0, 3), at=torch.zeros(0, 3), up=torch.zeros(0, 3))
    with pytest.raises(ValueError, match="empty"):
        project(torch.zeros(0, 20, 3), torch.zeros(0, 20, 3), c)


@pytest.mark.parametrize("viewport", [[0, 0, 0, 4], [0, 0, 5, 0], [3, 0, 2, 4], [0, 0, 5]])
def test_an_empty_or_malformed_viewport(viewport):
    refused(project, _args, "viewport", camera=dict(_args()["camera"], viewport=viewport))


@pytest.mark.parametrize("key", ["surfels", "rgb"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.bool])
def test_a_non_float_input(key, dtype):
    a = _args()
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
                project(a["surfels"].to(dtype), a["rgb"].to(dtype).reshape(2, 20, 3), a["camera"])
    with pytest.raises(RuntimeError, match="GPU"):
        project(**_args(B=1, H=1, W=1, D=1))
