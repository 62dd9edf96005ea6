"""projection_reverse_renderer refuses what the kernels cannot index -- ValueError on the host, before the library is
loaded and before anything reaches the GPU (so these run without one).  The checks it shares with the other
re-projection layers are those of tests/projection_validation.py, the camera's run against both of its cameras; its own
follow."""
import pytest
import torch

from projection_validation import camera, camera_tests, image_tests, refused
from projection_validation import no_library  # noqa: F401  (fixtures)
from surf_renderer_amd import projection_reverse_renderer as project

CAMERAS = ["camera1", "camera2"]


def _args(B=2, H=4, W=5, D=3, hom=False):
    g = torch.Generator().manual_seed(0)
    return {"rgb": torch.rand(B, H, W, D, generator=g), "in_pos_wc": torch.rand(B, H * W, 3, generator=g),
            "out_pos_wc": torch.rand(B, H * W, 3, generator=g), "camera1": camera(B, H, W, 0.7, 0.5, hom),
            "camera2": camera(B, H, W, 0.9, 0.8, hom)}


globals().update(image_tests(project, _args, ["rgb", "in_pos_wc", "out_pos_wc", "rotated_image"], lambda D: (2, 4, 5, D),
                             [(2, 20, 3), (2, 4, 5, 2), (1, 4, 5, 3), (2, 5, 4, 3)]))
globals().update(camera_tests(project, _args, CAMERAS))


@pytest.mark.parametrize("shape", [(2, 20, 3), (4, 5, 3), (2, 4, 5), (2, 1, 4, 5, 3)])
def test_rgb_that_is_not_a_batch_of_images(shape):
    refused(project, _args, "rgb", rgb=torch.zeros(shape))


@pytest.mark.parametrize("key", ["in_pos_wc", "out_pos_wc"])
@pytest.mark.parametrize("shape", [(2, 20), (2, 20, 4), (20, 3), (2, 4, 5, 3), (2, 19, 3), (1, 20, 3)])
def test_positions_of_another_shape(key, shape):
    refused(project, _args, key, **{key: torch.zeros(shape)})


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("viewport", [[0, 0, 4, 5], [0, 0, 5, 5], [0, 0, 6, 4], [0, 0, 0, 4], [3, 0, 2, 4], [0, 0, 5]])
def test_a_viewport_that_is_not_the_frame_of_rgb(cam, viewport):
    refused(project, _args, cam + r".*viewport", **{cam: dict(_args()[cam], viewport=viewport)})


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_a_depth_epsilon_that_is_not_finite(value):
    refused(project, _args, "depth_epsilon", depth_epsilon=value)


@pytest.mark.parametrize("value", [-0.1, 1.0, 1.5, float("nan")])
def test_a_mask_dropout_outside_zero_to_one(value):
    refused(project, _args, "mask_dropout", mask_dropout=value)


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
