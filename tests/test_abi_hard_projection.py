"""srh_hard_projection_keys / _fwd / _bwd: exported, bound, and their argument checks -- which return before any HIP
call, so they run without a GPU.  Host buffers stand in for device pointers: no call here reaches a launch."""
import ctypes as C

import pytest

from projection_abi import CAMERA, FRAME_ROWS, NULL, PINHOLE_ROWS, call, pointers, valid_params
from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid(**fields):
    return valid_params(_lib.SrhHardProjectionParams, **dict(dict(n_views=2, width=16, height=12, channels=3, fovy=0.7,
                                                                  focal_length=0.5), **fields))


KEYS = ("view", "surfels", "keys")
FWD = ("rgb", "keys", "order", "out", "mask", "count")
BWD = ("keys", "count", "g_out", "grad_rgb")
CALLS = (("srh_hard_projection_keys", KEYS), ("srh_hard_projection_fwd", FWD), ("srh_hard_projection_bwd", BWD))


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name, spec in CALLS:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(spec) + 2
    assert C.sizeof(_lib.SrhHardProjectionParams) == 4 * 4 + 2 * 8
    import surf_renderer_amd
    assert "projection_renderer" in surf_renderer_amd.__all__
    assert callable(surf_renderer_amd.projection_renderer)


def test_null_arguments_are_refused_by_name(lib):
    p, a, _ = _valid()
    for name, spec in CALLS:
        fn = getattr(lib, name)
        assert fn(None, *[a] * len(spec), None) == NULL and b"params" in lib.srh_last_error(), name
        for k in pointers(spec):
            assert call(fn, spec, p, a, **{k: None}) == NULL, (name, k)
            assert k.encode() in lib.srh_last_error(), (name, k)


@pytest.mark.parametrize("field,value,code", FRAME_ROWS + PINHOLE_ROWS + [("focal_length", -1.0, CAMERA)])
def test_out_of_range_parameters_are_refused_by_name(lib, field, value, code):
    p, a, _ = _valid(**{field: value})
    name = {"width": b"width x height", "height": b"width x height"}.get(field, field.encode())
    for fn, spec in CALLS:
        assert call(getattr(lib, fn), spec, p, a) == code, fn
        assert name in lib.srh_last_error(), (fn, lib.srh_last_error())
