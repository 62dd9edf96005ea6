"""srh_splat_ndc_fwd / srh_splat_ndc_bwd: exported, bound, and their argument checks -- which return before any HIP call,
so they run without a GPU.  Host buffers stand in for device pointers: no call here reaches a launch."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid():
    buf = (C.c_float * 64)()
    p = _lib.SrhSplatNdcParams(n_views=2, width=4, height=3, pos_cols=3, shade=1, fovy=0.8, near_clip=1.0, far_clip=10.0)
    p.up[:] = [0.0, 1.0, 0.0]
    a = C.addressof(buf)
    inp = _lib.SrhSplatNdcInputs(pos=a, pos_view_stride=36, normal=a, normal_view_stride=36, eye=a)
    idx = (C.c_int32 * 4)()
    li = _lib.SrhLights(n_lights=1, n_colors=1, pos=a, color_idx=C.addressof(idx), colors=a)
    ma = _lib.SrhMaterials(n_materials=1, albedo=a)
    return p, inp, li, ma, buf, idx


def _fwd(lib, p, inp, li, ma, buf, image=True):
    a = C.addressof(buf)
    return lib.srh_splat_ndc_fwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), a if image else None, a, a, None)


def _bwd(lib, p, inp, li, ma, ups, grads):
    return lib.srh_splat_ndc_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), *ups, C.byref(grads), None)


def test_entry_points_are_exported_and_bound(lib):
    assert hasattr(lib, "srh_splat_ndc_fwd") and hasattr(lib, "srh_splat_ndc_bwd")
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name in ("srh_splat_ndc_fwd", "srh_splat_ndc_bwd"):
        assert name in _lib.EXPORTS
    assert len(lib.srh_splat_ndc_fwd.argtypes) == 8
    assert len(lib.srh_splat_ndc_bwd.argtypes) == 9
    assert C.sizeof(_lib.SrhSplatNdcParams) == 8 * 4 + 3 * 8 + 6 * 8
    assert C.sizeof(_lib.SrhSplatNdcInputs) == 8 * 8
    assert C.sizeof(_lib.SrhSplatNdcGrads) == 8 * 8


def test_the_public_names_are_exported():
    import surf_renderer_amd
    assert "render_splats_NDC" in surf_renderer_amd.__all__
    assert "render_splats_NDC_batch" in surf_renderer_amd.__all__


def test_null_arguments_are_refused(lib):
    p, inp, li, ma, buf, _ = _valid()
    a = C.addressof(buf)
    assert lib.srh_splat_ndc_fwd(None, C.byref(inp), C.byref(li), C.byref(ma), a, a, a, None) == -1    # SRH_E_NULL
    assert lib.srh_splat_ndc_fwd(C.byref(p), None, C.byref(li), C.byref(ma), a, a, a, None) == -1
    assert lib.srh_splat_ndc_fwd(C.byref(p), C.byref(inp), None, C.byref(ma), a, a, a, None) == -1
    assert lib.srh_splat_ndc_fwd(C.byref(p), C.byref(inp), C.byref(li), None, a, a, a, None) == -1
    assert _fwd(lib, p, inp, li, ma, buf, image=False) == -1                # shading needs an image buffer
    assert lib.srh_splat_ndc_fwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), a, None, a, None) == -1
    assert lib.srh_splat_ndc_fwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), a, a, None, None) == -1
    for field in ("pos", "eye", "normal"):
        p, inp, li, ma, buf, _ = _valid()
        setattr(inp, field, None)
        assert _fwd(lib, p, inp, li, ma, buf) == -1, field
        assert field.encode() in lib.srh_last_error()
    for field in ("pos", "color_idx", "colors"):
        p, inp, li, ma, buf, _ = _valid()
        setattr(li, field, None)
        assert _fwd(lib, p, inp, li, ma, buf) == -1, field
    p, inp, li, ma, buf, _ = _valid()
    ma.albedo = None
    assert _fwd(lib, p, inp, li, ma, buf) == -1
    assert b"albedo" in lib.srh_last_error()


def test_a_backward_without_gradients_is_refused(lib):
    p, inp, li, ma, buf, _ = _valid()
    a = C.addressof(buf)
    assert lib.srh_splat_ndc_bwd(C.byref(p), C.byref(inp), C.byref(li), C.byref(ma), a, None, None, None, None) == -1
    assert _bwd(lib, p, inp, li, ma, (None, None, None), _lib.SrhSplatNdcGrads(pos=a)) == -1
    assert b"all NULL" in lib.srh_last_error()
    assert _bwd(lib, p, inp, li, ma, (a, None, None), _lib.SrhSplatNdcGrads()) == -1
    assert b"all NULL" in lib.srh_last_error()


def test_a_geometry_only_frame_refuses_shading_gradients(lib):
    p, inp, li, ma, buf, _ = _valid()
    a = C.addressof(buf)
    p.shade = 0
    for field in ("lights_pos", "colors", "attenuation", "ambient", "albedo", "coeffs"):
        grads = _lib.SrhSplatNdcGrads(**{field: a})
        assert _bwd(lib, p, inp, li, ma, (None, a, None), grads) == -3, field          # SRH_E_TYPE
    assert _bwd(lib, p, inp, li, ma, (a, None, None), _lib.SrhSplatNdcGrads(pos=a)) == -3   # grad_image without an image
    assert b"geometry-only" in lib.srh_last_error()


@pytest.mark.parametrize("field,value", [("n_views", 0), ("width", 0), ("height", 0), ("pos_cols", 2), ("pos_cols", 5),
                                         ("fovy", 0.0), ("fovy", 3.5), ("near_clip", 0.0), ("near_clip", 10.0),
                                         ("far_clip", 0.5)])
def test_out_of_range_parameters_are_refused(lib, field, value):
    p, inp, li, ma, buf, _ = _valid()
    setattr(p, field, value)
    assert _fwd(lib, p, inp, li, ma, buf) == -2                             # SRH_E_RANGE
    name = {"n_views": b"n_views", "width": b"grid", "height": b"grid"}.get(field, field.split("_")[0].encode())
    assert name in lib.srh_last_error()


@pytest.mark.parametrize("n_lights", [0, 65])
def test_the_light_count_is_held_to_its_range(lib, n_lights):
    p, inp, li, ma, buf, _ = _valid()
    li.n_lights = n_lights
    assert _fwd(lib, p, inp, li, ma, buf) == -2
    assert b"n_lights" in lib.srh_last_error()


def test_a_degenerate_camera_is_refused(lib):
    p, inp, li, ma, buf, _ = _valid()
    p.up[:] = [0.0, 0.0, 0.0]
    assert _fwd(lib, p, inp, li, ma, buf) == -5                             # SRH_E_CAMERA
    assert b"degenerate" in lib.srh_last_error()
