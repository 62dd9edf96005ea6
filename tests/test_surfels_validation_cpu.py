"""depth_to_surfels refuses what the kernels cannot index -- ValueError on the host, before the library is loaded and
before anything reaches the GPU (so these run without one).  The camera checks it shares with the re-projection layers
are those of tests/projection_validation.py; its own follow."""
import numpy as np
import pytest
import torch

from projection_validation import camera, camera_tests, refused
from projection_validation import cam, no_library  # noqa: F401  (fixtures)
from surf_renderer_amd import depth_to_surfels as lift


def _args(B=2, H=4, W=5, D=None, hom=False):
    g = torch.Generator().manual_seed(0)
    return {"depth": torch.rand(B, H, W, generator=g) + 1.0, "camera": camera(B, H, W, hom=hom)}


globals().update(camera_tests(lift, _args))


@pytest.mark.parametrize("shape", [(20,), (2, 19), (2, 21), (2, 5, 4), (2, 4, 5, 2), (2, 4, 5, 1, 1), (2, 20, 1), ()])
def test_a_depth_that_is_not_one_value_per_pixel(shape):
    refused(lift, _args, "depth", depth=torch.ones(shape))


def test_an_empty_batch():
    c = dict(_args()["camera"], eye=torch.zeros(0, 3), at=torch.zeros(0, 3), up=torch.zeros(0, 3))
    with pytest.raises(ValueError, match="depth"):
        lift(torch.zeros(0, 20), c)


@pytest.mark.parametrize("viewport", [[0, 0, 0, 4], [0, 0, 5, 0], [3, 0, 2, 4], [0, 0, 5]])
def test_an_empty_or_malformed_viewport(viewport):
    refused(lift, _args, "viewport", camera=dict(_args()["camera"], viewport=viewport))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.bool])
def test_a_non_float_depth(dtype):
    a = _args()
    with pytest.raises(ValueError, match="floating"):
        lift(a["depth"].to(dtype), a["camera"])
    with pytest.raises(ValueError, match="floating"):
        lift(np.ones((2, 20), dtype=np.int64), a["camera"])
    with pytest.raises(ValueError, match="missing"):
        lift(None, a["camera"])


@pytest.mark.parametrize("frame", ["World", "ndc", "", None, 1])
def test_a_frame_that_is_neither_world_nor_camera(frame):
    refused(lift, _args, "frame", frame=frame)


def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for hom in (False, True):
        for frame in ("world", "camera"):
            for dtype in (torch.float32, torch.float64, torch.float16):
                a = _args(hom=hom)
                for depth in (a["depth"], a["depth"].reshape(2, 20), a["depth"][..., None]):
                    with pytest.raises(RuntimeError, match="GPU"):
                        lift(depth.to(dtype), a["camera"], frame=frame)
    with pytest.raises(RuntimeError, match="GPU"):
        lift(**_args(B=1, H=1, W=1))
