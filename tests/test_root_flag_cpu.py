"""The host's decision about a camera's primary rays (srh.hip: camera_to_frame, read through srh_camera_ray_flags).
Bit 0: the three divisions by |D| may share one reciprocal.  Bit 1, only with bit 0: |D|^2 is bounded over the frame
(1e-100 <= |D| <= 1e100 with a lower bound within 1e6 of the upper one), so the binned finish rounds take its square root
without range guards (srh_device.h: sqrt_bounded).  No GPU: the entry point returns before any HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, golden_cases
from oracle.golden_io import load_case
from surf_renderer_amd import _lib, build, renderer, synthetic

SHARED, BOUNDED = 1, 2


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def flags(lib, camera, shading="numpy"):
    cam = renderer.camera_struct(camera, shading)
    out = C.c_int32(-1)
    _lib.check(lib.srh_camera_ray_flags(C.byref(cam), 1 if shading == "torch" else 0, C.byref(out)))
    return out.value


def scaled(camera, focal=None, fovy=None, **vectors):
    cam = dict(camera)
    if focal is not None:
        cam["focal_length"] = focal
    if fovy is not None:
        cam["fovy"] = fovy
    for k, v in vectors.items():
        cam[k] = np.asarray(v, dtype=np.float64)
    return cam


@pytest.mark.parametrize("shading", ["numpy", "torch"])
def test_the_benchmarks_camera_is_bounded(lib, shading):
    assert flags(lib, synthetic.disk_cloud_scene(4)["camera"], shading) == SHARED | BOUNDED
    assert flags(lib, synthetic.demo_scene(96, 64, with_planes=True)["camera"], shading) == SHARED | BOUNDED


@pytest.mark.parametrize("case", golden_cases())
def test_golden_cameras_are_bounded(lib, case):
    scene, _, _ = load_case(os.path.join(GOLDEN_DIR, case + ".npz"))
    assert flags(lib, scene["camera"]) == SHARED | BOUNDED


def test_cameras_out_of_the_admitted_range_are_not(lib):
    base = synthetic.disk_cloud_scene(4, 64, 48)["camera"]
    assert flags(lib, base) == SHARED | BOUNDED
    # |D| >= focal = 1e-120 is all the host can say: below 1e-100.  The shared division goes with it (1e-15 .. 1e15).
    assert flags(lib, scaled(base, focal=1e-120)) == 0
    assert flags(lib, scaled(base, focal=1e120)) == 0
    # magnitudes the shared division admits, but a lower bound more than 1e6 below the upper one: fovy so close to pi
    # that the image plane is 1e7 focal lengths wide
    wide = flags(lib, scaled(base, fovy=float(np.pi - 2e-7)))
    assert wide & BOUNDED == 0 and wide == SHARED
    # up nearly parallel to the view direction: x = up x z is tiny, the basis leaves the shared division's range
    assert flags(lib, scaled(base, up=[0.0, 1e-17, 1.0, 0.0])) & BOUNDED == 0


def test_the_bounded_bit_is_never_set_alone(lib):
    base = synthetic.disk_cloud_scene(4, 64, 48)["camera"]
    rng = np.random.RandomState(3)
    seen = set()
    for _ in range(200):
        cam = scaled(base, focal=float(10.0 ** rng.uniform(-130, 130)), fovy=float(rng.uniform(0.01, np.pi - 1e-8)),
                     eye=np.append(rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3), 1.0), up=np.append(rng.normal(size=3), 0.0))
        f = flags(lib, cam)
        seen.add(f)
        assert f in (0, SHARED, SHARED | BOUNDED)
    assert {0, SHARED | BOUNDED} <= seen


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_cameras_are_not(lib, bad):
    base = synthetic.disk_cloud_scene(4, 64, 48)["camera"]
    cam = renderer.camera_struct(scaled(base, focal=bad))
    out = C.c_int32(-1)
    rc = lib.srh_camera_ray_flags(C.byref(cam), 0, C.byref(out))
    assert rc != 0 or out.value & BOUNDED == 0
    cam = renderer.camera_struct(scaled(base, eye=[bad, 0.0, 4.0, 1.0]))
    rc = lib.srh_camera_ray_flags(C.byref(cam), 0, C.byref(out))
    assert rc != 0 or out.value == 0


def test_the_environment_switch_clears_only_the_bounded_bit(lib):
    base = synthetic.disk_cloud_scene(4, 64, 48)["camera"]
    os.environ["SRH_ROOT_GUARDS"] = "1"
    try:
        assert flags(lib, base) == SHARED
    finally:
        del os.environ["SRH_ROOT_GUARDS"]
    assert flags(lib, base) == SHARED | BOUNDED


def test_null_output_is_refused(lib):
    cam = renderer.camera_struct(synthetic.disk_cloud_scene(4, 64, 48)["camera"])
    assert lib.srh_camera_ray_flags(C.byref(cam), 0, None) == -1 and b"flags" in lib.srh_last_error()
