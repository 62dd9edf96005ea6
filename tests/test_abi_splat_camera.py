"""srh_splat_bwd_view / srh_splat_ndc_bwd_view: exported, bound, declared, and their argument checks -- which return
before any HIP call, so they run without a GPU.  Host buffers stand in for device pointers: no call here reaches a
launch."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build
from test_abi import declared_prototypes

NULL, RANGE, TYPE, WORKSPACE = -1, -2, -3, -4
BIG = 1 << 30


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _scene(ndc):
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    if ndc:
        p = _lib.SrhSplatNdcParams(n_views=2, width=20, height=30, pos_cols=3, shade=1, fovy=0.8, near_clip=1.0,
                                   far_clip=10.0)
        inp = _lib.SrhSplatNdcInputs(pos=a, pos_view_stride=1800, normal=a, eye=a)
    else:
        p = _lib.SrhSplatParams(n_views=2, width=20, height=30, samples=2, pos_cols=1, shade=1, fovy=0.8,
                                focal_length=1.0)
        inp = _lib.SrhSplatInputs(pos=a, pos_view_stride=600, normal=a, eye=a)
    p.up[:] = [0.0, 1.0, 0.0]
    idx = (C.c_int32 * 4)()
    li = _lib.SrhLights(n_lights=1, n_colors=1, pos=a, color_idx=C.addressof(idx), colors=a)
    ma = _lib.SrhMaterials(n_materials=1, albedo=a)
    return p, inp, li, ma, a, (buf, idx)


def _call(lib, ndc, p, inp, li, ma, grads, g_image, g_depth, grad_view, vws, vws_bytes):
    head = (C.byref(p), C.byref(inp), C.byref(li), C.byref(ma))
    tail = (C.byref(grads) if grads is not None else None, grad_view, vws, vws_bytes, None)
    if ndc:
        return lib.srh_splat_ndc_bwd_view(*head, g_image, g_depth, None, *tail)
    return lib.srh_splat_bwd_view(*head, None, 0, g_image, g_depth, None, None, *tail)


def _grads(ndc, **kw):
    return (_lib.SrhSplatNdcGrads if ndc else _lib.SrhSplatGrads)(**kw)


def test_entry_points_are_exported_bound_and_declared(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    protos = declared_prototypes()
    for name, n in (("srh_splat_bwd_view", 15), ("srh_splat_ndc_bwd_view", 12)):
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name) and name in protos
        assert len(getattr(lib, name).argtypes) == n == len(protos[name][1])
    assert len(lib.srh_splat_bwd_view.argtypes) == len(lib.srh_splat_bwd.argtypes) + 3
    assert len(lib.srh_splat_ndc_bwd_view.argtypes) == len(lib.srh_splat_ndc_bwd.argtypes) + 3


@pytest.mark.parametrize("ndc", [False, True])
def test_grad_view_and_its_workspace_are_checked_by_name(lib, ndc):
    p, inp, li, ma, a, keep = _scene(ndc)
    g = _grads(ndc)                                                          # every other gradient output NULL
    assert _call(lib, ndc, p, inp, li, ma, g, a, None, None, a, BIG) == NULL
    assert b"grad_view" in lib.srh_last_error()
    assert _call(lib, ndc, p, inp, li, ma, g, a, None, a + 4, a, BIG) == WORKSPACE
    assert b"grad_view" in lib.srh_last_error() and b"aligned" in lib.srh_last_error()
    assert _call(lib, ndc, p, inp, li, ma, g, a, None, a, None, BIG) != 0
    assert b"view_workspace" in lib.srh_last_error()
    # the BASE grid decides the workgroups: 20 x 30 = 600 splats = 3 workgroups per view, whatever `samples`
    need = lib.srh_view_grad_workspace_bytes(2, 20, 30)
    assert need == 2 * 3 * 12 * 8
    assert _call(lib, ndc, p, inp, li, ma, g, a, None, a, a, need - 1) == WORKSPACE
    assert b"view_workspace" in lib.srh_last_error()
    assert _call(lib, ndc, p, inp, li, ma, None, a, None, a, a, BIG) == NULL
    assert b"grads" in lib.srh_last_error()
    assert _call(lib, ndc, p, inp, li, ma, g, None, None, a, a, BIG) == NULL
    assert b"all NULL" in lib.srh_last_error()


@pytest.mark.parametrize("ndc", [False, True])
def test_a_geometry_only_frame_has_no_camera_gradient(lib, ndc):
    p, inp, li, ma, a, keep = _scene(ndc)
    p.shade = 0
    assert _call(lib, ndc, p, inp, li, ma, _grads(ndc, pos=a), None, a, a, a, BIG) == TYPE
    assert b"grad_view" in lib.srh_last_error()


@pytest.mark.parametrize("ndc", [False, True])
def test_the_layer_s_own_checks_come_first(lib, ndc):
    p, inp, li, ma, a, keep = _scene(ndc)
    p.n_views = 0
    assert _call(lib, ndc, p, inp, li, ma, _grads(ndc), a, None, a, a, BIG) == RANGE
    p, inp, li, ma, a, keep = _scene(ndc)
    inp.eye = None
    assert _call(lib, ndc, p, inp, li, ma, _grads(ndc), a, None, a, a, BIG) == NULL


def test_the_plain_ndc_entry_point_still_refuses_no_gradient_buffers(lib):
    p, inp, li, ma, a, keep = _scene(True)
    g = _grads(True)
    assert lib.srh_splat_ndc_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), a, None, None, C.byref(g),
                                 None) == NULL
    assert b"all NULL" in lib.srh_last_error()
