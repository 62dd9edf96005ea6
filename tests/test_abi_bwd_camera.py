"""srh_render_bwd_camera and srh_camera_grad_scratch_bytes (ABI 11, added without a version change): exported, bound, and
their argument checks -- which return before any HIP call, so they run without a GPU."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _call(lib, shading="torch", grad_image=None, grad_depth=None, scratch=None, scratch_bytes=0, want=("eye", "at", "up"),
          viewport=(0, 0, 48, 36), rows=(0, 36)):
    cam, ob, li, mat = _lib.SrhCamera(), _lib.SrhObjects(), _lib.SrhLights(), _lib.SrhMaterials()
    cam.viewport[:] = list(viewport)
    params = _lib.SrhParams(row0=rows[0], row1=rows[1], shading=_lib.SHADING[shading])
    grads, cg = _lib.SrhGrads(), _lib.SrhCameraGrads()
    out = (C.c_float * 12)()
    for i, k in enumerate(("eye", "at", "up")):
        if k in want:
            setattr(cg, k, C.addressof(out) + 16 * i)
    return lib.srh_render_bwd_camera(C.byref(cam), C.byref(ob), C.byref(li), C.byref(mat), C.byref(params), None, 0,
                                     grad_image, grad_depth, None, None, None, None, C.byref(grads), C.byref(cg),
                                     scratch, scratch_bytes, None)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12
    assert "srh_render_bwd_camera" in _lib.EXPORTS and "srh_camera_grad_scratch_bytes" in _lib.EXPORTS
    assert len(lib.srh_render_bwd_camera.argtypes) == 18
    assert C.sizeof(_lib.SrhCameraGrads) == 24
    assert [f[0] for f in _lib.SrhCameraGrads._fields_] == ["eye", "at", "up"]


def test_all_upstream_gradients_null_is_refused(lib):
    assert _call(lib) == -1                                       # SRH_E_NULL
    assert b"all NULL" in lib.srh_last_error()


def test_numpy_shading_is_refused(lib):
    buf = (C.c_float * 12)()
    scratch = (C.c_double * 4096)()
    assert _call(lib, "numpy", grad_image=C.addressof(buf), scratch=C.addressof(scratch),
                 scratch_bytes=C.sizeof(scratch)) == -3           # SRH_E_TYPE
    assert b"SRH_SHADING_TORCH" in lib.srh_last_error()


def test_scratch_null_or_too_small_is_refused(lib):
    buf = (C.c_float * 12)()
    need = lib.srh_camera_grad_scratch_bytes(48, 36)
    assert need == 1 * 9 * 12 * 8                                 # one 64 x 4-pixel workgroup per slot of 12 doubles
    assert _call(lib, grad_depth=C.addressof(buf)) == -4          # SRH_E_WORKSPACE
    assert b"camera scratch" in lib.srh_last_error()
    scratch = (C.c_double * (need // 8))()
    assert _call(lib, grad_depth=C.addressof(buf), scratch=C.addressof(scratch), scratch_bytes=need - 8) == -4
    assert b"camera scratch" in lib.srh_last_error()
    # a large enough scratch passes this check: the call goes on to the frame's own validation (an all-zero camera)
    assert _call(lib, grad_depth=C.addressof(buf), scratch=C.addressof(scratch), scratch_bytes=need) == -5
    # with no camera gradient wanted the scratch is not looked at (the call is srh_render_bwd_aux)
    assert _call(lib, grad_depth=C.addressof(buf), want=()) == -5


def test_scratch_bytes_are_positive_and_monotone(lib):
    f = lib.srh_camera_grad_scratch_bytes
    assert f(1, 1) > 0
    for w in (1, 63, 64, 65, 640, 2048):
        for h in (1, 4, 5, 480, 2048):
            assert f(w, h) > 0
            assert f(w + 1, h) >= f(w, h) and f(w, h + 1) >= f(w, h) and f(w + 64, h + 4) > f(w, h)
    assert f(2048, 2048) == 32 * 512 * 96
    assert f(0, 4) == 0 and f(4, 0) == 0
    assert lib.srh_last_error()
