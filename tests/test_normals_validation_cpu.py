"""The plane-fit layer refuses what the kernels cannot index -- ValueError on the host, naming the argument, before the
library is loaded and before anything reaches the GPU (so these run without one)."""
import numpy as np
import pytest
import torch

from projection_validation import camera
from projection_validation import no_library  # noqa: F401  (autouse fixture)
from surf_renderer_amd import (estimate_surface_normals, estimate_surface_normals_plane_fit,
                               estimate_surface_normals_plane_fit_batched as fit)


def _pos(*shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(0))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.bool])
def test_a_non_float_pos(dtype):
    with pytest.raises(ValueError, match="pos.*floating"):
        fit(_pos(2, 4, 5, 3).to(dtype))
    with pytest.raises(ValueError, match="pos.*floating"):
        fit(np.ones((2, 4, 5, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="pos.*floating"):
        estimate_surface_normals_plane_fit(_pos(4, 5, 3).to(dtype))
    with pytest.raises(ValueError, match="pos.*missing"):
        fit(None)


@pytest.mark.parametrize("shape", [(20,), (4, 5), (2, 4, 5, 2), (2, 4, 5, 4), (2, 4, 5, 3, 1), (1, 2, 4, 5, 3), (0, 4, 5, 3)])
def test_a_pos_of_another_rank_or_last_dimension(shape):
    with pytest.raises(ValueError, match="pos"):
        fit(torch.zeros(shape))


@pytest.mark.parametrize("shape", [(2, 1, 5, 3), (2, 5, 1, 3), (1, 1, 1, 3)])
def test_a_side_below_two(shape):
    with pytest.raises(ValueError, match="pos.*H >= 2"):
        fit(torch.zeros(shape))
    with pytest.raises(ValueError, match="pos.*H >= 2"):
        estimate_surface_normals_plane_fit(torch.zeros(shape[1:]))


def test_flat_points_need_a_camera_and_one_point_per_pixel():
    with pytest.raises(ValueError, match="camera.*viewport"):
        fit(_pos(2, 20, 3))
    cam = camera(2, 4, 5)
    for n in (19, 21, 25):
        with pytest.raises(ValueError, match="pos.*W x H"):
            fit(_pos(2, n, 3), cam)
    with pytest.raises(ValueError, match="camera.*viewport.*missing"):
        fit(_pos(2, 20, 3), {k: v for k, v in cam.items() if k != "viewport"})
    for viewport in ([0, 0, 0, 4], [0, 0, 5, 0], [0, 0, 5]):
        with pytest.raises(ValueError, match="viewport"):
            fit(_pos(2, 20, 3), dict(cam, viewport=viewport))
    with pytest.raises(ValueError, match="pos.*H >= 2"):
        fit(_pos(2, 5, 3), dict(cam, viewport=[0, 0, 5, 1]))


@pytest.mark.parametrize("frame", ["World", "ndc", "", None, 1])
def test_a_frame_that_is_neither_camera_nor_world(frame):
    with pytest.raises(ValueError, match="frame"):
        fit(_pos(2, 4, 5, 3), camera(2, 4, 5), frame=frame)


def test_the_world_frame_needs_a_camera_with_eye_at_and_up():
    with pytest.raises(ValueError, match="frame = 'world' needs a camera"):
        fit(_pos(2, 4, 5, 3), frame="world")
    cam = camera(2, 4, 5)
    for k in ("eye", "at", "up"):
        with pytest.raises(ValueError, match="camera.*" + k + ".*missing"):
            fit(_pos(2, 4, 5, 3), {q: v for q, v in cam.items() if q != k}, frame="world")
        with pytest.raises(ValueError, match="camera.*" + k):
            fit(_pos(2, 4, 5, 3), dict(cam, **{k: torch.ones(3, 3)}), frame="world")          # three views for two
        with pytest.raises(ValueError, match="camera.*" + k):
            fit(_pos(2, 4, 5, 3), dict(cam, **{k: torch.ones(2)}), frame="world")
    with pytest.raises(ValueError, match="eye.*at"):
        fit(_pos(2, 4, 5, 3), dict(cam, at=cam["eye"].clone()), frame="world")
    with pytest.raises(ValueError, match="up"):
        fit(_pos(2, 4, 5, 3), dict(cam, up=torch.zeros(2, 3)), frame="world")


@pytest.mark.parametrize("key", ["eye", "at", "up"])
@pytest.mark.parametrize("frame", ["camera", "world"])
def test_a_camera_that_requires_grad(key, frame):
    cam = camera(2, 4, 5)
    cam[key] = cam[key].clone().requires_grad_(True)
    for pos in (_pos(2, 4, 5, 3), _pos(2, 20, 3)):
        with pytest.raises(ValueError, match="camera.*" + key + ".*requires grad"):
            fit(pos, cam, frame=frame)


def test_the_unbatched_entry_point_takes_a_grid_and_the_dispatcher_only_the_plane_fit():
    for shape in [(20, 3), (2, 4, 5, 3), (4, 5, 2), (3,)]:
        with pytest.raises(ValueError, match="pos.*H, W, 3"):
            estimate_surface_normals_plane_fit(torch.zeros(shape))
    for method in ("avg_normal", "quadric", "Plane", None):
        with pytest.raises(ValueError, match=repr(method)):
            estimate_surface_normals(_pos(4, 5, 3), method=method)


def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cam = camera(2, 4, 5)
    shared = dict(cam, eye=cam["eye"][0], at=cam["at"][0], up=cam["up"][0])
    hom = camera(2, 4, 5, hom=True)
    for dtype in (torch.float32, torch.float64, torch.float16):
        for call in (lambda p: fit(p), lambda p: fit(p, cam), lambda p: fit(p, cam, frame="world"),
                     lambda p: fit(p, shared, frame="world"), lambda p: fit(p, hom, frame="world"),
                     lambda p: fit(p.reshape(2, 20, 3), cam), lambda p: fit(p.reshape(2, 20, 3), cam, "world"),
                     lambda p: estimate_surface_normals_plane_fit(p[0]), lambda p: estimate_surface_normals(p[0], 3),
                     lambda p: estimate_surface_normals_plane_fit(p[0].numpy().astype(np.float64), kernel_size=5)):
            with pytest.raises(RuntimeError, match="GPU"):
                call(_pos(2, 4, 5, 3).to(dtype))
