"""srh_depth_to_surfels_fwd / _bwd: exported, bound, and their argument checks -- which return before any HIP call, so
they run without a GPU.  Host buffers stand in for device pointers: no call here reaches a launch."""
import ctypes as C

import pytest

from projection_abi import CAMERA, NULL, PINHOLE_ROWS, RANGE, TYPE, call, pointers, valid_params
from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid(**fields):
    return valid_params(_lib.SrhSurfelsParams, **dict(dict(n_views=2, width=16, height=12, frame=1, fovy=0.7,
                                                           focal_length=0.5), **fields))


FWD = ("view", "depth", "out")
BWD = ("view", "depth", "g_out", "grad_depth")


def _fwd(lib, p, a, **given):
    return call(lib.srh_depth_to_surfels_fwd, FWD, p, a, **given)


def _bwd(lib, p, a, **given):
    return call(lib.srh_depth_to_surfels_bwd, BWD, p, a, **given)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name in ("srh_depth_to_surfels_fwd", "srh_depth_to_surfels_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.srh_depth_to_surfels_fwd.argtypes) == 5
    assert len(lib.srh_depth_to_surfels_bwd.argtypes) == 6
    assert C.sizeof(_lib.SrhSurfelsParams) == 4 * 4 + 2 * 8
    assert _lib.SURFELS_FRAME == {"camera": 0, "world": 1}
    import surf_renderer_amd
    assert "depth_to_surfels" in surf_renderer_amd.__all__
    assert callable(surf_renderer_amd.depth_to_surfels)


def test_null_arguments_are_refused_by_name(lib):
    p, a, _ = _valid()
    assert lib.srh_depth_to_surfels_fwd(None, a, a, a, None) == NULL and b"params" in lib.srh_last_error()
    assert lib.srh_depth_to_surfels_bwd(None, a, a, a, a, None) == NULL and b"params" in lib.srh_last_error()
    for fn, spec in ((_fwd, FWD), (_bwd, BWD)):
        for k in pointers(spec):
            assert fn(lib, p, a, **{k: None}) == NULL, k
            assert k.encode() in lib.srh_last_error(), k


def test_the_camera_frame_does_without_a_view_but_not_without_the_rest(lib):
    p, a, _ = _valid(frame=0)
    for fn, spec in ((_fwd, FWD), (_bwd, BWD)):
        for k in pointers(spec):
            if k != "view":
                assert fn(lib, p, a, view=None, **{k: None}) == NULL and k.encode() in lib.srh_last_error(), k


@pytest.mark.parametrize("field,value,code", [
    ("n_views", 0, RANGE), ("n_views", 65536, RANGE), ("width", 0, RANGE), ("height", 0, RANGE), ("width", 1 << 22, RANGE),
    ("frame", 2, TYPE), ("frame", -1, TYPE)] + PINHOLE_ROWS + [("focal_length", -1.0, CAMERA)])
def test_out_of_range_parameters_are_refused_by_name(lib, field, value, code):
    p, a, _ = _valid(**{field: value})
    name = {"width": b"width x height", "height": b"width x height"}.get(field, field.encode())
    for fn in (_fwd, _bwd):
        assert fn(lib, p, a) == code, fn.__name__
        assert name in lib.srh_last_error(), (fn.__name__, lib.srh_last_error())
