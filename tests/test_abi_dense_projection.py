"""srh_dense_projection_workspace_bytes / srh_dense_projection_fwd / srh_dense_projection_bwd: exported, bound, declared,
and their argument checks -- which return before any HIP call, so they run without a GPU.  Host buffers stand in for
device pointers: no call here reaches a launch."""
import ctypes as C
import re

import pytest

from projection_abi import (BIG, FRAME_ROWS, NULL, PINHOLE_ROWS, RANGE, TYPE, WORKSPACE, assert_refused_by_name, call, pointers,
                            valid_params)
from surf_renderer_amd import _lib, build

NAMES = ("srh_dense_projection_workspace_bytes", "srh_dense_projection_fwd", "srh_dense_projection_bwd")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid(**fields):
    return valid_params(_lib.SrhDenseProjectionParams, **dict(dict(n_views=2, width=16, height=12, channels=3, has_rotated=1,
                                                                   sigma=1.2, fovy=0.7, focal_length=0.5), **fields))


FWD = ("view", "surfels", "rgb", "rotated", "workspace", "ws_bytes", "saved", "saved_bytes", "out", "mask")
BWD = ("view", "surfels", "rgb", "rotated", "saved", "saved_bytes", "workspace", "ws_bytes", "g_out", "g_mask",
       "grad_surfels", "grad_rgb", "grad_rotated")


def _fwd(lib, p, a, **given):
    return call(lib.srh_dense_projection_fwd, FWD, p, a, **given)


def _bwd(lib, p, a, **given):
    return call(lib.srh_dense_projection_bwd, BWD, p, a, **given)


def test_entry_points_are_exported_bound_and_declared(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    header = re.sub(r"/\*.*?\*/", "", open(build.INCLUDE + "/srh.h").read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert "typedef struct SrhDenseProjectionParams" in header
    assert len(lib.srh_dense_projection_fwd.argtypes) == 12
    assert len(lib.srh_dense_projection_bwd.argtypes) == 15
    assert C.sizeof(_lib.SrhDenseProjectionParams) == 6 * 4 + 3 * 8
    import surf_renderer_amd
    assert "projection_renderer_differentiable" in surf_renderer_amd.__all__
    assert callable(surf_renderer_amd.projection_renderer_differentiable)


def test_workspace_sizes_follow_the_documented_layouts(lib):
    p, _, _ = _valid(width=37, height=35)
    B, N, D = 2, 37 * 35, 3
    size = lambda which: lib.srh_dense_projection_workspace_bytes(C.byref(p), which)      # noqa: E731
    assert size(_lib.DPROJ_WS_FWD) == B * N * 2 * 8
    assert size(_lib.DPROJ_WS_SAVED) == B * N * (D + 1) * 8
    assert size(_lib.DPROJ_WS_BWD) == B * 35 * 48 * (D + 1) * 8          # rows padded to whole strips of 16 columns
    assert size(3) == 0 and b"which" in lib.srh_last_error()
    assert size(-1) == 0 and b"which" in lib.srh_last_error()
    assert lib.srh_dense_projection_workspace_bytes(None, 0) == 0 and b"params" in lib.srh_last_error()
    p.has_rotated = 0                                                      # the sizes do not depend on it
    assert size(_lib.DPROJ_WS_SAVED) == B * N * (D + 1) * 8


def test_the_workspaces_grow_linearly_with_the_frame(lib):
    """No buffer of W H x N: doubling W H doubles every size (a quadratic one would quadruple)."""
    for w, h in ((64, 64), (128, 128), (512, 256)):
        one, _, _ = _valid(width=w, height=h)
        two, _, _ = _valid(width=2 * w, height=h)
        for which in range(3):
            a = lib.srh_dense_projection_workspace_bytes(C.byref(one), which)
            b = lib.srh_dense_projection_workspace_bytes(C.byref(two), which)
            assert a > 0 and b == 2 * a, (w, h, which)
    # and all of them together stay within a small multiple of B (N + P)(D + 2) doubles
    p, _, _ = _valid(n_views=64, width=128, height=128)
    total = sum(lib.srh_dense_projection_workspace_bytes(C.byref(p), which) for which in range(3))
    assert total <= 64 * (2 * 128 * 128) * (3 + 2) * 8


def test_null_arguments_are_refused_by_name(lib):
    p, a, _ = _valid()
    assert lib.srh_dense_projection_fwd(None, a, a, a, a, a, BIG, a, BIG, a, a, None) == NULL
    assert b"params" in lib.srh_last_error()
    for k in pointers(FWD):
        want = {"workspace": WORKSPACE, "saved": None}.get(k, NULL)
        if want is not None:                          # saved is optional
            assert _fwd(lib, p, a, **{k: None}) == want, k
            assert k.encode() in lib.srh_last_error(), k
    for k in ("view", "surfels", "rgb", "rotated"):
        assert _bwd(lib, p, a, **{k: None}) == NULL and k.encode() in lib.srh_last_error(), k
    for k in ("saved", "workspace"):
        assert _bwd(lib, p, a, **{k: None}) == WORKSPACE and k.encode() in lib.srh_last_error(), k


def test_the_rotated_image_is_there_exactly_when_the_parameters_say_so(lib):
    p, a, _ = _valid(has_rotated=0)
    assert _fwd(lib, p, a) == TYPE and b"has_rotated = 0" in lib.srh_last_error()
    assert _bwd(lib, p, a) == TYPE and b"has_rotated = 0" in lib.srh_last_error()
    # without one, grad_rotated has no partner
    assert _bwd(lib, p, a, rotated=None) == NULL and b"grad_rotated without rotated" in lib.srh_last_error()
    p, a, _ = _valid(has_rotated=1)
    assert _fwd(lib, p, a, rotated=None) == NULL and b"has_rotated = 1" in lib.srh_last_error()


def test_all_null_gradients_are_refused(lib):
    p, a, _ = _valid()
    assert _bwd(lib, p, a, g_out=None, g_mask=None) == NULL
    assert b"g_out" in lib.srh_last_error() and b"both NULL" in lib.srh_last_error()
    assert _bwd(lib, p, a, grad_surfels=None, grad_rgb=None, grad_rotated=None) == NULL
    assert b"grad_surfels" in lib.srh_last_error() and b"all NULL" in lib.srh_last_error()


@pytest.mark.parametrize("field,value,code", FRAME_ROWS + [
    ("has_rotated", 2, TYPE), ("has_rotated", -1, TYPE), ("sigma", 0.0, RANGE), ("sigma", -1.0, RANGE),
    ("sigma", float("nan"), RANGE), ("sigma", float("inf"), RANGE)] + PINHOLE_ROWS)
def test_out_of_range_parameters_are_refused_by_name(lib, field, value, code):
    p, a, _ = _valid(**{field: value})
    assert_refused_by_name(lib, (_fwd, _bwd), lib.srh_dense_projection_workspace_bytes, p, a, field, code)


def test_short_or_misaligned_buffers_are_refused(lib):
    p, a, _ = _valid()
    need = [lib.srh_dense_projection_workspace_bytes(C.byref(p), w) for w in range(3)]
    assert _fwd(lib, p, a, ws_bytes=need[0] - 1) == WORKSPACE and str(need[0]).encode() in lib.srh_last_error()
    assert _fwd(lib, p, a, saved_bytes=need[1] - 1) == WORKSPACE and b"saved" in lib.srh_last_error()
    assert _bwd(lib, p, a, saved_bytes=need[1] - 1) == WORKSPACE and b"saved" in lib.srh_last_error()
    assert _bwd(lib, p, a, ws_bytes=need[2] - 1) == WORKSPACE and str(need[2]).encode() in lib.srh_last_error()
    assert _fwd(lib, p, a, workspace=a + 4) == WORKSPACE
    assert _fwd(lib, p, a, saved=a + 4) == WORKSPACE
    assert _bwd(lib, p, a, workspace=a + 4) == WORKSPACE
