"""projection_renderer_differentiable_fast refuses what the kernels cannot index -- ValueError on the host, before the
library is loaded and before anything reaches the GPU (so these run without one).  The checks it shares with the other
re-projection layers are those of tests/projection_validation.py; its own follow."""
import pytest
import torch

from projection_validation import camera, camera_tests, image_tests, refused, surfel_tests
from projection_validation import cam, no_library  # noqa: F401  (fixtures)
from surf_renderer_amd import projection_renderer_differentiable_fast as project


def _args(B=2, H=4, W=5, D=3, hom=False):
    g = torch.Generator().manual_seed(0)
    return {"surfels": torch.rand(B, H * W, 3, generator=g), "rgb": torch.rand(B, H, W, D, generator=g),
            "camera": camera(B, H, W, hom=hom)}


globals().update(surfel_tests(project, _args))
globals().update(image_tests(project, _args, ["surfels", "rgb", "rotated_image"], lambda D: (2, 20, D),
                             [(2, 20, 3), (2, 4, 5, 2), (1, 4, 5, 3)]))
globals().update(camera_tests(project, _args))


def test_a_blur_wider_than_the_kernels_hold(monkeypatch):
    refused(project, _args, "half-width", blur_size=32.6)           # floor(3 * 32.6 * 4 / 6) = 65
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):                  # 64 passes the check
        project(**_args(), blur_size=32.4)
