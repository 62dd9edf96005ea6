"""srh_splat_workspace_bytes / srh_splat_fwd / srh_splat_bwd: exported, bound, and their argument checks -- which return
before any HIP call, so they run without a GPU.  Host buffers stand in for device pointers: no call here reaches a
launch."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid():
    buf = (C.c_float * 64)()
    p = _lib.SrhSplatParams(n_views=2, width=4, height=3, samples=1, pos_cols=1, shade=1, fovy=0.8, focal_length=1.0)
    p.up[:] = [0.0, 1.0, 0.0]
    inp = _lib.SrhSplatInputs(pos=C.addressof(buf), pos_view_stride=12, eye=C.addressof(buf))
    idx = (C.c_int32 * 4)()
    li = _lib.SrhLights(n_lights=1, n_colors=1, pos=C.addressof(buf), color_idx=C.addressof(idx), colors=C.addressof(buf))
    ma = _lib.SrhMaterials(n_materials=1, albedo=C.addressof(buf))
    return p, inp, li, ma, buf


def _fwd(lib, p, inp, li, ma, buf, image=True):
    a = C.addressof(buf)
    return lib.srh_splat_fwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), a if image else None, a, a, a, None)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name in ("srh_splat_workspace_bytes", "srh_splat_fwd", "srh_splat_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.srh_splat_fwd.argtypes) == 9
    assert len(lib.srh_splat_bwd.argtypes) == 12


def test_workspace_holds_nine_doubles_per_splat_and_view(lib):
    p, inp, *_ = _valid()
    assert lib.srh_splat_workspace_bytes(C.byref(p), C.byref(inp)) == 2 * 12 * 9 * 8
    inp.normal = inp.pos                                                    # given normals: no stencil, no workspace
    assert lib.srh_splat_workspace_bytes(C.byref(p), C.byref(inp)) == 0
    assert lib.srh_splat_workspace_bytes(None, C.byref(inp)) == 0 and b"NULL" in lib.srh_last_error()


def test_null_arguments_are_refused(lib):
    p, inp, li, ma, buf = _valid()
    a = C.addressof(buf)
    assert lib.srh_splat_fwd(None, C.byref(inp), C.byref(li), C.byref(ma), a, a, a, a, None) == -1     # SRH_E_NULL
    assert _fwd(lib, p, inp, li, ma, buf, image=False) == -1                # shading needs an image buffer
    inp.eye = None
    assert _fwd(lib, p, inp, li, ma, buf) == -1
    p, inp, li, ma, buf = _valid()
    li.colors = None
    assert _fwd(lib, p, inp, li, ma, buf) == -1
    p, inp, li, ma, buf = _valid()
    grads = _lib.SrhSplatGrads(pos=a)
    assert lib.srh_splat_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), None, 0, None, None, None, None,
                             C.byref(grads), None) == -1
    assert b"all NULL" in lib.srh_last_error()
    grads = _lib.SrhSplatGrads(light_vis=a)                                 # no light_vis input to differentiate
    assert lib.srh_splat_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), None, 0, a, None, None, None,
                             C.byref(grads), None) == -1
    grads = _lib.SrhSplatGrads(pos=a)                                       # estimated normals: the stencil workspace
    assert lib.srh_splat_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), None, 0, a, None, None, None,
                             C.byref(grads), None) == -4                    # SRH_E_WORKSPACE


def test_a_geometry_only_frame_refuses_shading_gradients(lib):
    p, inp, li, ma, buf = _valid()
    a = C.addressof(buf)
    p.shade = 0
    inp.normal = a
    inp.light_vis = a
    for field in ("light_vis", "lights_pos", "colors", "attenuation", "ambient", "albedo", "coeffs"):
        grads = _lib.SrhSplatGrads(**{field: a})
        assert lib.srh_splat_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), None, 0, None, a, None, None,
                                 C.byref(grads), None) == -3, field                # SRH_E_TYPE
    grads = _lib.SrhSplatGrads(pos=a)
    assert lib.srh_splat_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), None, 0, a, None, None, None,
                             C.byref(grads), None) == -3                            # grad_image without an image


@pytest.mark.parametrize("field,value", [("n_views", 0), ("width", 0), ("samples", 0), ("samples", 9),
                                         ("pos_cols", 2), ("focal_length", 0.0), ("fovy", 3.5)])
def test_out_of_range_parameters_are_refused(lib, field, value):
    p, inp, li, ma, buf = _valid()
    setattr(p, field, value)
    assert _fwd(lib, p, inp, li, ma, buf) == -2                             # SRH_E_RANGE


def test_small_grids_and_light_counts(lib):
    p, inp, li, ma, buf = _valid()
    p.width = 1                                                              # the plane fit needs 2 x 2
    assert _fwd(lib, p, inp, li, ma, buf) == -2
    assert b"2 x 2" in lib.srh_last_error()
    p, inp, li, ma, buf = _valid()
    li.n_lights = 65
    assert _fwd(lib, p, inp, li, ma, buf) == -2
    p, inp, li, ma, buf = _valid()
    p.up[:] = [0.0, 0.0, 0.0]
    assert _fwd(lib, p, inp, li, ma, buf) == -5                             # SRH_E_CAMERA
