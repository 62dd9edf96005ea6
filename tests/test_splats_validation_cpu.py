"""render_splats_along_ray(_batch) checks every shape the HIP kernels index by on the host, before anything reaches the
GPU: a wrong shape is a ValueError, never a read past the end of a device buffer.  Runs without a GPU."""
import copy

import numpy as np
import pytest

import splat_oracle
from conftest import GOLDEN_DIR
from surf_renderer_amd import render_splats_along_ray, render_splats_along_ray_batch
from surf_renderer_amd.splats import _validate


def _scene():
    npz = np.load(f"{GOLDEN_DIR}/p1_given_normals_vis_30x40.npz", allow_pickle=False)
    return splat_oracle.unpack(npz)                     # 40 x 30 grid, N = 1200, 2 lights, 2 materials, [N, 3] pos


def _batch(B=3):
    sc = _scene()
    d = sc["objects"]["disk"]
    d["pos"] = np.stack([d["pos"]] * B)
    d["normal"] = np.stack([d["normal"]] * B)
    sc["camera"]["eye"] = np.stack([sc["camera"]["eye"]] * B)
    sc["lights"]["pos"] = np.stack([sc["lights"]["pos"]] * B)
    return sc


def test_valid_scenes_pass():
    _validate(_scene(), batched=False)
    _validate(_batch(), batched=True)
    sc = _batch()
    sc["objects"]["disk"]["normal"] = sc["objects"]["disk"]["normal"][0]        # shared by every view
    sc["objects"]["disk"]["light_vis"] = sc["objects"]["disk"]["light_vis"][None].repeat(3, 0)
    _validate(sc, batched=True)


BAD = [
    ("objects.disk.pos", lambda sc: sc["objects"]["disk"].__setitem__("pos", np.zeros((1199, 3), np.float32))),
    ("objects.disk.pos", lambda sc: sc["objects"]["disk"].__setitem__("pos", np.zeros((1200, 2), np.float32))),
    ("objects.disk.normal", lambda sc: sc["objects"]["disk"].__setitem__("normal", np.zeros((1000, 3), np.float32))),
    ("objects.disk.normal", lambda sc: sc["objects"]["disk"].__setitem__("normal", np.zeros((1200, 2), np.float32))),
    ("objects.disk.light_vis", lambda sc: sc["objects"]["disk"].__setitem__("light_vis", np.zeros((3, 1200)))),
    ("objects.disk.light_vis", lambda sc: sc["objects"]["disk"].__setitem__("light_vis", np.zeros((2, 1100)))),
    ("objects.disk.material_idx", lambda sc: sc["objects"]["disk"].__setitem__("material_idx", np.zeros(100, int))),
    ("lights.pos", lambda sc: sc["lights"].__setitem__("pos", np.zeros((2, 3), np.float32))),
    ("lights.color_idx", lambda sc: sc["lights"].__setitem__("color_idx", np.array([1]))),
    ("lights.attenuation", lambda sc: sc["lights"].__setitem__("attenuation", np.zeros((1, 3)))),
    ("lights.ambient", lambda sc: sc["lights"].__setitem__("ambient", np.zeros(2))),
    ("colors", lambda sc: sc.__setitem__("colors", np.zeros((3, 2)))),
    ("materials.coeffs", lambda sc: sc["materials"].__setitem__("coeffs", np.zeros((1, 3)))),
    ("camera.eye", lambda sc: sc["camera"].__setitem__("eye", np.zeros((2, 4)))),
    ("camera.eye", lambda sc: sc["camera"].__setitem__("eye", np.zeros(2))),
    ("lights.pos", lambda sc: sc["lights"].__setitem__("pos", np.zeros((65, 4)))),
]


@pytest.mark.parametrize("name,spoil", BAD)
def test_a_wrong_shape_is_refused_before_any_launch(name, spoil):
    sc = _scene()
    spoil(sc)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        render_splats_along_ray(sc)


@pytest.mark.parametrize("key", ["pos", "normal", "eye", "lights.pos", "light_vis"])
def test_a_batch_dimension_that_disagrees_is_refused(key):
    sc = _batch(3)
    d = sc["objects"]["disk"]
    if key == "eye":
        sc["camera"]["eye"] = sc["camera"]["eye"][:2]
    elif key == "lights.pos":
        sc["lights"]["pos"] = sc["lights"]["pos"][:2]
    elif key == "light_vis":
        d["light_vis"] = np.stack([d["light_vis"]] * 4)
    elif key == "pos":
        d["pos"] = d["pos"][:, :1000]
    else:
        d["normal"] = d["normal"][:2]
    with pytest.raises(ValueError):
        render_splats_along_ray_batch(copy.deepcopy(sc))
