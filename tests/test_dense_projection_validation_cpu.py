"""projection_renderer_differentiable refuses what the kernels cannot index -- ValueError on the host, before the
library is loaded and before anything reaches the GPU (so these run without one).  The checks it shares with the other
re-projection layers are those of tests/projection_validation.py; its own follow."""
import pytest
import torch

from projection_validation import camera, camera_tests, image_tests, surfel_tests
from projection_validation import cam, no_library  # noqa: F401  (fixtures)
from surf_renderer_amd import projection_renderer_differentiable as project


def _args(B=2, H=4, W=5, D=3, hom=False):
    g = torch.Generator().manual_seed(0)
    return {"surfels": torch.rand(B, H * W, 3, generator=g), "rgb": torch.rand(B, H, W, D, generator=g),
            "camera": camera(B, H, W, hom=hom)}


globals().update(surfel_tests(project, _args))
globals().update(image_tests(project, _args, ["surfels", "rgb", "rotated_image"], lambda D: (2, 20, D),
                             [(2, 20, 3), (2, 4, 5, 2), (1, 4, 5, 3)]))
globals().update(camera_tests(project, _args))


def test_any_positive_blur_size_passes_the_checks(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for blur_size in (1e-6, 0.15, 1e6):              # sigma has no upper limit here: there is no tap table to fill
        with pytest.raises(RuntimeError, match="GPU"):
            project(**_args(), blur_size=blur_size)
