"""camera_grad of projection_renderer_differentiable_camera and estimate_surface_normals_plane_fit_batched on the host:
ValueError before the library is loaded and before anything reaches the GPU, so these run without one.

  - camera_grad=True keeps every camera check of tests/projection_validation.py for the dense layer (run here with
    camera leaves that require grad), except the one it exists to lift;
  - camera_grad must be a bool;
  - the default still refuses a camera that requires grad, and the message offers camera_grad=True;
  - fovy, focal_length and the viewport get no gradient anywhere, so they are refused under either value;
  - frame='camera' of the normals accepts camera leaves under camera_grad=True (it does not read them);
  - the function under the reference's name keeps the reference's signature: no keyword, the camera is data;
  - a valid call gets as far as asking for the GPU."""
import functools

import pytest
import torch

from projection_validation import camera, camera_tests
from projection_validation import cam, no_library  # noqa: F401  (fixtures)
from surf_renderer_amd import (estimate_surface_normals_plane_fit_batched, projection_renderer_differentiable,
                               projection_renderer_differentiable_camera)

KEYS = ("eye", "at", "up")


def _leaves(c):
    return dict(c, **{k: c[k].clone().requires_grad_(True) for k in KEYS})


def _dense_args(B=2, H=4, W=5, D=3, hom=False, grad=True):
    g = torch.Generator().manual_seed(0)
    c = camera(B, H, W, hom=hom)
    return {"surfels": torch.rand(B, H * W, 3, generator=g), "rgb": torch.rand(B, H, W, D, generator=g),
            "camera": _leaves(c) if grad else c}


def _normals_args(B=2, H=4, W=5, D=None, hom=False, grad=True, frame="world", flat=False):
    g = torch.Generator().manual_seed(0)
    c = camera(B, H, W, hom=hom)
    pos = torch.rand(B, H, W, 3, generator=g)
    return {"pos": pos.reshape(B, H * W, 3) if flat else pos, "camera": _leaves(c) if grad else c, "frame": frame}


LAYERS = {"dense": (projection_renderer_differentiable_camera, _dense_args),
          "normals": (estimate_surface_normals_plane_fit_batched, _normals_args)}

# every camera check of the re-projection layers, with camera_grad=True and camera leaves
_tests = camera_tests(functools.partial(projection_renderer_differentiable_camera, camera_grad=True), _dense_args)
del _tests["test_a_camera_that_requires_grad"]
globals().update({f"test_dense_with_camera_grad_{name[5:]}": t for name, t in _tests.items()})


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("value", [1, 0, None, "yes", 1.0, torch.tensor(True)])
def test_camera_grad_that_is_not_a_bool(layer, value):
    fn, args = LAYERS[layer]
    for grad in (False, True):
        with pytest.raises(ValueError, match="camera_grad"):
            fn(**args(grad=grad), camera_grad=value)


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("key", KEYS)
def test_the_default_still_refuses_a_camera_that_requires_grad(layer, key):
    fn, args = LAYERS[layer]
    for kw in ({}, {"camera_grad": False}):
        a = args(grad=False)
        a["camera"] = dict(a["camera"], **{key: a["camera"][key].clone().requires_grad_(True)})
        with pytest.raises(ValueError, match=r"camera.*requires grad.*camera_grad=True"):
            fn(**a, **kw)


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("key", ["fovy", "focal_length", "viewport"])
def test_what_is_not_eye_at_or_up_is_refused_under_either_value(layer, key):
    fn, args = LAYERS[layer]
    for camera_grad in (False, True):
        a = args(grad=camera_grad)
        a["camera"] = dict(a["camera"], **{key: torch.tensor(a["camera"][key], dtype=torch.float64, requires_grad=True)})
        with pytest.raises(ValueError, match=r"camera.*" + key + r".*requires grad"):
            fn(**a, camera_grad=camera_grad)


def test_the_normals_keep_their_camera_checks_under_camera_grad():
    a = _normals_args()
    for key, value, match in (("eye", a["camera"]["at"], "eye"), ("up", torch.zeros(2, 3, requires_grad=True), "up"),
                              ("at", torch.zeros(3, 3), "at")):
        with pytest.raises(ValueError, match=match):
            estimate_surface_normals_plane_fit_batched(a["pos"], dict(a["camera"], **{key: value}), "world",
                                                       camera_grad=True)
    with pytest.raises(ValueError, match="needs a camera"):
        estimate_surface_normals_plane_fit_batched(a["pos"], None, "world", camera_grad=True)


@pytest.mark.parametrize("layer", list(LAYERS))
def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(layer, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fn, args = LAYERS[layer]
    for hom in (False, True):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(**args(hom=hom), camera_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):                   # the keyword without a leaf is the detached call
        fn(**args(grad=False), camera_grad=True)


@pytest.mark.parametrize("flat", [False, True])
def test_the_camera_frame_of_the_normals_accepts_camera_leaves(flat, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        estimate_surface_normals_plane_fit_batched(**_normals_args(frame="camera", flat=flat), camera_grad=True)
    shared = _normals_args()
    shared["camera"] = dict(shared["camera"], **{k: shared["camera"][k][0].detach().clone().requires_grad_(True)
                                                 for k in KEYS})
    with pytest.raises(RuntimeError, match="GPU"):                   # shared [3] leaves in the world frame
        estimate_surface_normals_plane_fit_batched(**shared, camera_grad=True)


def test_the_reference_named_dense_call_keeps_its_signature_and_names_itself():
    a = _dense_args(grad=True)
    with pytest.raises(ValueError, match=r"^projection_renderer_differentiable: camera.*requires grad"):
        projection_renderer_differentiable(**a)
    with pytest.raises(TypeError):
        projection_renderer_differentiable(**a, camera_grad=True)
    with pytest.raises(ValueError, match=r"^projection_renderer_differentiable_camera: camera.*camera_grad=True"):
        projection_renderer_differentiable_camera(**a)
