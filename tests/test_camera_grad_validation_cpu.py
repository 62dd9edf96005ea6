"""camera_grad of depth_to_surfels, projection_renderer_differentiable_fast and projection_reverse_renderer on the host:
ValueError before the library is loaded and before anything reaches the GPU, so these run without one.

  - camera_grad=True keeps every camera check of tests/projection_validation.py (run here with camera leaves that
    require grad), except the one it exists to lift;
  - camera_grad must be a bool;
  - the default still refuses a camera that requires grad -- the layers' own test modules assert that through
    projection_validation.test_a_camera_that_requires_grad, and it is asserted again here with the message's new hint;
  - fovy, focal_length and the viewport get no gradient anywhere, so they are refused under either value;
  - a valid call gets as far as asking for the GPU."""
import functools

import pytest
import torch

from projection_validation import camera, camera_tests
from projection_validation import cam, no_library  # noqa: F401  (fixtures)
from surf_renderer_amd import (depth_to_surfels, projection_renderer_differentiable, projection_renderer_differentiable_fast,
                               projection_reverse_renderer)

KEYS = ("eye", "at", "up")


def _leaves(c):
    return dict(c, **{k: c[k].clone().requires_grad_(True) for k in KEYS})


def _lift_args(B=2, H=4, W=5, D=None, hom=False, grad=True):
    g = torch.Generator().manual_seed(0)
    c = camera(B, H, W, hom=hom)
    return {"depth": torch.rand(B, H, W, generator=g) + 1.0, "camera": _leaves(c) if grad else c}


def _project_args(B=2, H=4, W=5, D=3, hom=False, grad=True):
    g = torch.Generator().manual_seed(0)
    c = camera(B, H, W, hom=hom)
    return {"surfels": torch.rand(B, H * W, 3, generator=g), "rgb": torch.rand(B, H, W, D, generator=g),
            "camera": _leaves(c) if grad else c}


def _reverse_args(B=2, H=4, W=5, D=3, hom=False, grad=True):
    g = torch.Generator().manual_seed(0)
    c1, c2 = camera(B, H, W, 0.7, 0.5, hom), camera(B, H, W, 0.9, 0.8, hom)
    return {"rgb": torch.rand(B, H, W, D, generator=g), "in_pos_wc": torch.rand(B, H * W, 3, generator=g),
            "out_pos_wc": torch.rand(B, H * W, 3, generator=g), "camera1": _leaves(c1) if grad else c1,
            "camera2": _leaves(c2) if grad else c2}


LAYERS = {"lift": (depth_to_surfels, _lift_args, None),
          "projection": (projection_renderer_differentiable_fast, _project_args, None),
          "reverse": (projection_reverse_renderer, _reverse_args, ["camera1", "camera2"])}

# every camera check, with camera_grad=True and camera leaves; the replaced entries of a check are plain tensors beside
# leaves, as a caller who optimises only some of them has it
for _layer, (_fn, _args, _cams) in LAYERS.items():
    _tests = camera_tests(functools.partial(_fn, camera_grad=True), _args, _cams)
    del _tests["test_a_camera_that_requires_grad"]
    globals().update({f"test_{_layer}_with_camera_grad_{name[5:]}": t for name, t in _tests.items()})


def _cameras(layer):
    return LAYERS[layer][2] or ["camera"]


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("value", [1, 0, None, "yes", 1.0, torch.tensor(True)])
def test_camera_grad_that_is_not_a_bool(layer, value):
    fn, args, _ = LAYERS[layer]
    for grad in (False, True):
        with pytest.raises(ValueError, match="camera_grad"):
            fn(**args(grad=grad), camera_grad=value)


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("key", KEYS)
def test_the_default_still_refuses_a_camera_that_requires_grad(layer, key):
    fn, args, _ = LAYERS[layer]
    for label in _cameras(layer):
        for kw in ({}, {"camera_grad": False}):
            a = args(grad=False)
            a[label] = dict(a[label], **{key: a[label][key].clone().requires_grad_(True)})
            with pytest.raises(ValueError, match=label + r".*requires grad.*camera_grad=True"):
                fn(**a, **kw)


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("key", ["fovy", "focal_length", "viewport"])
def test_what_is_not_eye_at_or_up_is_refused_under_either_value(layer, key):
    fn, args, _ = LAYERS[layer]
    for label in _cameras(layer):
        for camera_grad in (False, True):
            a = args(grad=camera_grad)
            a[label] = dict(a[label], **{key: torch.tensor(a[label][key], dtype=torch.float64, requires_grad=True)})
            with pytest.raises(ValueError, match=label + r".*" + key + r".*requires grad"):
                fn(**a, camera_grad=camera_grad)


def test_the_layers_without_the_keyword_keep_refusing():
    a = _project_args(grad=True)
    with pytest.raises(ValueError, match="requires grad"):
        projection_renderer_differentiable(**a)
    with pytest.raises(TypeError):
        projection_renderer_differentiable(**a, camera_grad=True)


@pytest.mark.parametrize("layer", list(LAYERS))
def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(layer, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fn, args, _ = LAYERS[layer]
    for hom in (False, True):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(**args(hom=hom), camera_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):                   # the keyword without a leaf is the detached call
        fn(**args(grad=False), camera_grad=True)
