"""srh_reverse_projection_workspace_bytes / _fwd / _keys / _bwd: exported, bound, and their argument checks -- which
return before any HIP call, so they run without a GPU.  Host buffers stand in for device pointers: no call here reaches
a launch."""
import ctypes as C

import pytest

from projection_abi import (BIG, CAMERA, FRAME_ROWS, NULL, RANGE, WORKSPACE, assert_refused_by_name, call,
                            pointers, valid_params)
from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid(**fields):
    return valid_params(_lib.SrhReverseProjectionParams, **dict(dict(n_views=2, width=16, height=12, channels=3, fovy1=0.7,
                                                                     focal_length1=0.5, fovy2=0.9, focal_length2=0.8,
                                                                     depth_epsilon=0.1), **fields))


FWD = ("view1", "view2", "rgb", "in_pos", "out_pos", "rotated", "keep", "workspace", "ws_bytes", "out", "mask", "image1",
       "depth")
KEYS = ("view1", "out_pos", "workspace", "ws_bytes", "keys")
BWD = ("view1", "view2", "rgb", "in_pos", "out_pos", "mask", "keys", "order", "workspace", "ws_bytes", "g_out", "g_image1",
       "g_depth", "grad_rgb", "grad_in_pos", "grad_out_pos", "grad_rotated")


def _fwd(lib, p, a, **given):
    return call(lib.srh_reverse_projection_fwd, FWD, p, a, **given)


def _keys(lib, p, a, **given):
    return call(lib.srh_reverse_projection_keys, KEYS, p, a, **given)


def _bwd(lib, p, a, **given):
    return call(lib.srh_reverse_projection_bwd, BWD, p, a, **given)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name in ("srh_reverse_projection_workspace_bytes", "srh_reverse_projection_fwd", "srh_reverse_projection_keys",
                 "srh_reverse_projection_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.srh_reverse_projection_fwd.argtypes) == 15
    assert len(lib.srh_reverse_projection_keys.argtypes) == 7
    assert len(lib.srh_reverse_projection_bwd.argtypes) == 19
    assert C.sizeof(_lib.SrhReverseProjectionParams) == 4 * 4 + 5 * 8
    import surf_renderer_amd
    assert "projection_reverse_renderer" in surf_renderer_amd.__all__
    assert callable(surf_renderer_amd.projection_reverse_renderer)


def test_workspace_sizes_follow_the_documented_layouts(lib):
    p, _, _ = _valid()
    px, D = 2 * 16 * 12, 3
    size = lambda which: lib.srh_reverse_projection_workspace_bytes(C.byref(p), which)      # noqa: E731
    assert size(_lib.RPROJ_WS_FWD) == px * 8
    assert size(_lib.RPROJ_WS_BWD) == px * (4 + D + 1) * 8 + 2 * 17 * 13 * 2 * 4
    assert size(2) == 0 and b"which" in lib.srh_last_error()
    assert size(-1) == 0 and b"which" in lib.srh_last_error()
    assert lib.srh_reverse_projection_workspace_bytes(None, 0) == 0 and b"params" in lib.srh_last_error()


def test_null_arguments_are_refused_by_name(lib):
    p, a, _ = _valid()
    assert lib.srh_reverse_projection_keys(None, a, a, a, BIG, a, None) == NULL and b"params" in lib.srh_last_error()
    optional = {"rotated", "keep", "depth"}
    for k in pointers(FWD):
        if k in optional:
            continue
        assert _fwd(lib, p, a, **{k: None}) == (WORKSPACE if k == "workspace" else NULL), k
        assert k.encode() in lib.srh_last_error(), k
    for k in pointers(KEYS):
        assert _keys(lib, p, a, **{k: None}) == (WORKSPACE if k == "workspace" else NULL), k
        assert k.encode() in lib.srh_last_error(), k
    for k in ("view1", "view2", "rgb", "in_pos", "out_pos", "mask", "keys", "order"):
        assert _bwd(lib, p, a, **{k: None}) == NULL and k.encode() in lib.srh_last_error(), k
    assert _bwd(lib, p, a, workspace=None) == WORKSPACE and b"workspace" in lib.srh_last_error()


def test_all_null_gradients_are_refused(lib):
    p, a, _ = _valid()
    assert _bwd(lib, p, a, g_out=None, g_image1=None, g_depth=None) == NULL
    assert b"g_out" in lib.srh_last_error() and b"all NULL" in lib.srh_last_error()
    assert _bwd(lib, p, a, grad_rgb=None, grad_in_pos=None, grad_out_pos=None, grad_rotated=None) == NULL
    assert b"grad_rgb" in lib.srh_last_error() and b"all NULL" in lib.srh_last_error()


@pytest.mark.parametrize("field,value,code", FRAME_ROWS + [
    ("fovy1", 0.0, CAMERA), ("fovy2", 3.2, CAMERA), ("fovy1", float("nan"), CAMERA), ("focal_length1", 0.0, CAMERA),
    ("focal_length2", float("inf"), CAMERA), ("focal_length2", -1.0, CAMERA), ("depth_epsilon", float("nan"), RANGE),
    ("depth_epsilon", float("inf"), RANGE)])
def test_out_of_range_parameters_are_refused_by_name(lib, field, value, code):
    p, a, _ = _valid(**{field: value})
    assert_refused_by_name(lib, (_fwd, _keys, _bwd), lib.srh_reverse_projection_workspace_bytes, p, a, field, code)


def test_short_or_misaligned_buffers_are_refused(lib):
    p, a, _ = _valid()
    need = [lib.srh_reverse_projection_workspace_bytes(C.byref(p), w) for w in range(2)]
    assert _fwd(lib, p, a, ws_bytes=need[0] - 1) == WORKSPACE and str(need[0]).encode() in lib.srh_last_error()
    assert _keys(lib, p, a, ws_bytes=need[1] - 1) == WORKSPACE and str(need[1]).encode() in lib.srh_last_error()
    assert _bwd(lib, p, a, ws_bytes=need[1] - 1) == WORKSPACE and str(need[1]).encode() in lib.srh_last_error()
    assert _fwd(lib, p, a, workspace=a + 4) == WORKSPACE
    assert _keys(lib, p, a, workspace=a + 4) == WORKSPACE
    assert _bwd(lib, p, a, workspace=a + 4) == WORKSPACE
