"""render_splats_NDC(_batch) checks every shape and range the HIP kernels rely on, on the host, before the library is
loaded or anything reaches the GPU: a wrong input is a ValueError naming the key, never a read past the end of a device
buffer.  Runs without a GPU."""
import copy
import os

import numpy as np
import pytest
import torch

import splats_ndc_oracle as oracle
from conftest import GOLDEN_DIR


def _scene(name="3x5"):
    npz = np.load(os.path.join(GOLDEN_DIR, "splats_ndc", f"sn1_{name}.npz"), allow_pickle=False)
    return oracle.unpack(npz)                              # 3 x 5 grid, N = 15, 2 lights, 2 materials, [N, 3] pos


def test_the_public_names_exist_and_valid_scenes_pass():
    import surf_renderer_amd
    from surf_renderer_amd.splats_ndc import _validate
    assert callable(surf_renderer_amd.render_splats_NDC) and callable(surf_renderer_amd.render_splats_NDC_batch)
    assert _validate(_scene(), batched=False) == (3, 5)
    assert _validate(_scene("3x5_w4"), batched=False) == (3, 5)
    assert _validate(_scene("17x9_b3"), batched=True) == (17, 9)
    assert _validate(_scene("17x9_b3_shared"), batched=True) == (17, 9)


def _set(path, value):
    def spoil(sc):
        d = sc
        for p in path[:-1]:
            d = d[p]
        d[path[-1]] = value
    return spoil


DISK, CAM, LIGHTS = ("objects", "disk"), ("camera",), ("lights",)
BAD = [
    ("camera.viewport", _set(CAM + ("viewport",), [0, 0, 3])),
    ("camera.viewport", _set(CAM + ("viewport",), [0, 0, 0, 5])),
    ("objects.disk.pos", _set(DISK + ("pos",), np.zeros((14, 3), np.float32))),
    ("objects.disk.pos", _set(DISK + ("pos",), np.zeros((15, 2), np.float32))),
    ("objects.disk.pos", _set(DISK + ("pos",), np.zeros((15,), np.float32))),
    ("objects.disk.pos", _set(DISK + ("pos",), np.zeros((2, 15, 3), np.float32))),
    ("objects.disk.normal", _set(DISK + ("normal",), np.zeros((14, 3), np.float32))),
    ("objects.disk.normal", _set(DISK + ("normal",), np.zeros((15, 2), np.float32))),
    ("objects.disk.normal", _set(DISK + ("normal",), None)),
    ("objects.disk.material_idx", _set(DISK + ("material_idx",), np.zeros(10, int))),
    ("lights.pos", _set(LIGHTS + ("pos",), np.zeros((2, 3), np.float32))),
    ("lights.pos", _set(LIGHTS + ("pos",), np.zeros((0, 4), np.float32))),
    ("lights.pos", _set(LIGHTS + ("pos",), np.zeros((65, 4), np.float32))),
    ("lights.color_idx", _set(LIGHTS + ("color_idx",), np.array([1]))),
    ("lights.attenuation", _set(LIGHTS + ("attenuation",), np.zeros((1, 3)))),
    ("lights.ambient", _set(LIGHTS + ("ambient",), np.zeros(2))),
    ("colors", _set(("colors",), np.zeros((3, 2)))),
    ("materials.albedo", _set(("materials", "albedo"), np.zeros((2, 4)))),
    ("materials.coeffs", _set(("materials", "coeffs"), np.zeros((1, 3)))),
    ("camera.near", _set(CAM + ("near",), 0.0)),
    ("camera.near", _set(CAM + ("near",), 10.0)),
    ("camera.far", _set(CAM + ("far",), 0.5)),
    ("camera.fovy", _set(CAM + ("fovy",), 0.0)),
    ("camera.fovy", _set(CAM + ("fovy",), 3.5)),
    ("camera.eye", _set(CAM + ("eye",), np.zeros(2))),
    ("camera.eye", _set(CAM + ("eye",), np.zeros((2, 4)))),
    ("camera.eye", _set(CAM + ("eye",), np.array([0.5, 1.0, 6.0, 0.5]))),
    ("camera.up", _set(CAM + ("up",), np.zeros(2))),
]


@pytest.fixture
def no_library(monkeypatch):
    """The refusals come before the library is loaded."""
    from surf_renderer_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the host checks")
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("name,spoil", BAD)
def test_a_wrong_input_is_refused_before_any_launch(name, spoil, no_library):
    from surf_renderer_amd import render_splats_NDC
    sc = _scene()
    spoil(sc)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        render_splats_NDC(sc)


@pytest.mark.parametrize("key", ["pos", "normal", "eye", "lights.pos"])
def test_a_batch_axis_that_disagrees_is_refused(key, no_library):
    from surf_renderer_amd import render_splats_NDC_batch
    sc = _scene("17x9_b3")
    d = sc["objects"]["disk"]
    if key == "eye":
        sc["camera"]["eye"] = sc["camera"]["eye"][:2]
    elif key == "lights.pos":
        sc["lights"]["pos"] = sc["lights"]["pos"][:2]
    elif key == "pos":
        d["pos"] = d["pos"][:, :100]
    else:
        d["normal"] = d["normal"][:2]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        render_splats_NDC_batch(copy.deepcopy(sc))


@pytest.mark.parametrize("key", ["eye", "at", "up"])
def test_a_camera_that_requires_grad_is_refused(key, no_library):
    from surf_renderer_amd import render_splats_NDC
    sc = _scene()
    sc["camera"][key] = torch.tensor(np.asarray(sc["camera"][key]), requires_grad=True)
    with pytest.raises(ValueError, match=f"camera\\['{key}'\\] requires grad"):
        render_splats_NDC(sc)


def test_without_a_gpu_the_call_fails_loudly(monkeypatch, no_library):
    from surf_renderer_amd import render_splats_NDC, render_splats_NDC_batch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        render_splats_NDC(_scene())
    with pytest.raises(RuntimeError, match="GPU"):
        render_splats_NDC_batch(_scene("17x9_b3"))
