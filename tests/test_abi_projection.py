"""srh_projection_workspace_bytes / srh_projection_keys / srh_projection_fwd / srh_projection_bwd: exported, bound, and
their argument checks -- which return before any HIP call, so they run without a GPU.  Host buffers stand in for device
pointers: no call here reaches a launch."""
import ctypes as C

import pytest

from projection_abi import (BIG, FRAME_ROWS, NULL, PINHOLE_ROWS, RANGE, TYPE, WORKSPACE, assert_refused_by_name, call, pointers,
                            valid_params)
from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid(**fields):
    p, a, buf = valid_params(_lib.SrhProjectionParams, **dict(dict(n_views=2, width=16, height=12, channels=3, flags=3,
                                                                   blur_half=3, fovy=0.7, focal_length=0.5), **fields))
    p.taps[:4] = [0.4, 0.2, 0.08, 0.02]
    return p, a, buf


KEYS = ("view", "surfels", "workspace", "ws_bytes", "keys")
FWD = ("rgb", "rotated", "keys", "order", "workspace", "ws_bytes", "saved", "saved_bytes", "out", "mask", "image1", "depth")
BWD = ("view", "surfels", "rgb", "rotated", "saved", "saved_bytes", "workspace", "ws_bytes", "g_out", "g_mask", "g_image1",
       "g_depth", "grad_surfels", "grad_rgb", "grad_rotated")


def _keys(lib, p, a, **given):
    return call(lib.srh_projection_keys, KEYS, p, a, **given)


def _fwd(lib, p, a, **given):
    return call(lib.srh_projection_fwd, FWD, p, a, **given)


def _bwd(lib, p, a, **given):
    return call(lib.srh_projection_bwd, BWD, p, a, **given)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name in ("srh_projection_workspace_bytes", "srh_projection_keys", "srh_projection_fwd", "srh_projection_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.srh_projection_keys.argtypes) == 7
    assert len(lib.srh_projection_fwd.argtypes) == 14
    assert len(lib.srh_projection_bwd.argtypes) == 17
    assert C.sizeof(_lib.SrhProjectionParams) == 6 * 4 + 2 * 8 + 65 * 8
    import surf_renderer_amd
    assert "projection_renderer_differentiable_fast" in surf_renderer_amd.__all__
    assert callable(surf_renderer_amd.projection_renderer_differentiable_fast)


def test_workspace_sizes_follow_the_documented_layouts(lib):
    p, _, _ = _valid()
    px, D = 2 * 16 * 12, 3
    plane, corner = 2 * D + 2, 4 * (D + 3)
    size = lambda which: lib.srh_projection_workspace_bytes(C.byref(p), which)      # noqa: E731
    assert size(_lib.PROJ_WS_FWD) == px * (4 + 2 * plane) * 8 + 2 * 17 * 13 * 2 * 4
    assert size(_lib.PROJ_WS_SAVED) == px * (plane + corner) * 8
    assert size(_lib.PROJ_WS_BWD) == px * (2 * plane + corner) * 8
    assert size(3) == 0 and b"which" in lib.srh_last_error()
    assert lib.srh_projection_workspace_bytes(None, 0) == 0 and b"params" in lib.srh_last_error()


def test_null_arguments_are_refused_by_name(lib):
    p, a, _ = _valid()
    assert lib.srh_projection_keys(None, a, a, a, BIG, a, None) == NULL and b"params" in lib.srh_last_error()
    for k in pointers(KEYS):
        assert _keys(lib, p, a, **{k: None}) == (WORKSPACE if k == "workspace" else NULL), k
        assert k.encode() in lib.srh_last_error(), k
    for k in pointers(FWD):
        want = {"workspace": WORKSPACE, "rotated": None, "saved": None, "depth": None}.get(k, NULL)
        if want is not None:                          # rotated, saved and depth are optional
            assert _fwd(lib, p, a, **{k: None}) == want, k
            assert k.encode() in lib.srh_last_error(), k
    for k in ("view", "surfels", "rgb"):
        assert _bwd(lib, p, a, **{k: None}) == NULL and k.encode() in lib.srh_last_error(), k
    for k in ("saved", "workspace"):
        assert _bwd(lib, p, a, **{k: None}) == WORKSPACE and k.encode() in lib.srh_last_error(), k


def test_all_null_gradients_are_refused(lib):
    p, a, _ = _valid()
    assert _bwd(lib, p, a, g_out=None, g_mask=None, g_image1=None, g_depth=None) == NULL
    assert b"g_out" in lib.srh_last_error() and b"all NULL" in lib.srh_last_error()
    assert _bwd(lib, p, a, grad_surfels=None, grad_rgb=None, grad_rotated=None) == NULL
    assert b"grad_surfels" in lib.srh_last_error() and b"all NULL" in lib.srh_last_error()
    assert _bwd(lib, p, a, rotated=None) == NULL and b"grad_rotated without rotated" in lib.srh_last_error()


@pytest.mark.parametrize("field,value,code", FRAME_ROWS + [
    ("blur_half", -1, RANGE), ("blur_half", 65, RANGE), ("flags", 64, TYPE), ("flags", -1, TYPE)] + PINHOLE_ROWS)
def test_out_of_range_parameters_are_refused_by_name(lib, field, value, code):
    p, a, _ = _valid(**{field: value})
    assert_refused_by_name(lib, (_keys, _fwd, _bwd), lib.srh_projection_workspace_bytes, p, a, field, code)


def test_a_tap_that_is_not_finite_is_refused(lib):
    p, a, _ = _valid()
    p.taps[2] = float("nan")
    assert _fwd(lib, p, a) == RANGE and b"taps[2]" in lib.srh_last_error()
    p.taps[2], p.taps[4] = 0.08, float("inf")        # past blur_half: not read
    assert lib.srh_projection_workspace_bytes(C.byref(p), 0) > 0


def test_short_or_misaligned_buffers_are_refused(lib):
    p, a, _ = _valid()
    need = [lib.srh_projection_workspace_bytes(C.byref(p), w) for w in range(3)]
    assert _keys(lib, p, a, ws_bytes=need[0] - 1) == WORKSPACE and str(need[0]).encode() in lib.srh_last_error()
    assert _fwd(lib, p, a, ws_bytes=need[0] - 1) == WORKSPACE and b"workspace" in lib.srh_last_error()
    assert _fwd(lib, p, a, saved_bytes=need[1] - 1) == WORKSPACE and b"saved" in lib.srh_last_error()
    assert _bwd(lib, p, a, saved_bytes=need[1] - 1) == WORKSPACE and b"saved" in lib.srh_last_error()
    assert _bwd(lib, p, a, ws_bytes=need[2] - 1) == WORKSPACE and str(need[2]).encode() in lib.srh_last_error()
    assert _keys(lib, p, a, workspace=a + 4) == WORKSPACE
    assert _fwd(lib, p, a, saved=a + 4) == WORKSPACE
    assert _bwd(lib, p, a, workspace=a + 4) == WORKSPACE
