"""srh_render_bwd_aux (ABI 11): exported, bound, and its argument checks -- which return before any HIP call, so they run
without a GPU."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _call(lib, shading, grad_image=None, grad_depth=None, grad_normal=None, grad_pos=None):
    cam, ob, li, mat = _lib.SrhCamera(), _lib.SrhObjects(), _lib.SrhLights(), _lib.SrhMaterials()
    params = _lib.SrhParams(row0=0, row1=1, shading=_lib.SHADING[shading])
    grads = _lib.SrhGrads()
    return lib.srh_render_bwd_aux(C.byref(cam), C.byref(ob), C.byref(li), C.byref(mat), C.byref(params), None, 0,
                                  grad_image, grad_depth, grad_normal, grad_pos, None, None, C.byref(grads), None)


def test_entry_point_is_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12
    assert "srh_render_bwd_aux" in _lib.EXPORTS
    assert len(lib.srh_render_bwd_aux.argtypes) == 15


def test_all_upstream_gradients_null_is_refused(lib):
    assert _call(lib, "torch") == -1                              # SRH_E_NULL
    assert b"all NULL" in lib.srh_last_error()


def test_numpy_shading_has_no_normal_or_pos_gradients(lib):
    buf = (C.c_float * 12)()
    assert _call(lib, "numpy", grad_image=C.addressof(buf), grad_normal=C.addressof(buf)) == -3     # SRH_E_TYPE
    assert b"SRH_SHADING_TORCH" in lib.srh_last_error()
    assert _call(lib, "numpy", grad_image=C.addressof(buf), grad_pos=C.addressof(buf)) == -3
    assert _call(lib, "numpy", grad_depth=C.addressof(buf)) == -1                                    # needs grad_image
