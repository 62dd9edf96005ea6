"""srh_dense_projection_bwd_view, srh_normals_bwd_view and SRH_DPROJ_WS_VIEW: exported, bound, and their argument checks
-- which return before any HIP call, so they run without a GPU.  Host buffers stand in for device pointers: no call here
reaches a launch (every call is refused by one of the checks it is about)."""
import ctypes as C

import pytest

from projection_abi import BIG, NULL, RANGE, TYPE, WORKSPACE, call, valid_params
from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _dense(**fields):
    return valid_params(_lib.SrhDenseProjectionParams, **dict(dict(n_views=2, width=16, height=12, channels=3,
                                                                   has_rotated=1, sigma=1.2, fovy=0.7, focal_length=0.5),
                                                              **fields))


VIEW = ("view_workspace", "view_workspace_bytes")
DPROJ = ("view", "surfels", "rgb", "rotated", "saved", "saved_bytes", "workspace", "workspace_bytes", "g_out", "g_mask",
         "grad_surfels", "grad_rgb", "grad_rotated", "grad_view") + VIEW
NORM = ("rot", "pos", "g_out", "workspace", "workspace_bytes", "grad_pos", "grad_rot") + VIEW


def _normals(lib, a, n_views=2, width=16, height=12, **given):
    """srh_normals_bwd_view(n_views, width, height, *NORM, stream = NULL) with projection_abi.call's conventions."""
    return lib.srh_normals_bwd_view(n_views, width, height,
                                    *[given.get(k, BIG if k.endswith("_bytes") else a) for k in NORM], None)


def _size(lib, which=_lib.DPROJ_WS_VIEW, **fields):
    return lib.srh_dense_projection_workspace_bytes(C.byref(_dense(**fields)[0]), which)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name, spec, front in (("srh_dense_projection_bwd_view", DPROJ, 1), ("srh_normals_bwd_view", NORM, 3)):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == front + len(spec) + 1    # params or the sizes in front, the stream behind


def test_the_dense_view_workspace_is_one_set_of_sums_per_wave(lib):
    """The surfel kernel's workgroup is one wave of 64: B ceil(N / 64) sets of 12 fp64, not the 256-lane size."""
    assert _size(lib, n_views=1, width=2, height=2) == 96
    assert _size(lib, n_views=3, width=9, height=17) == 3 * 3 * 96           # N = 153
    assert _size(lib, n_views=2, width=16, height=12) == 2 * 3 * 96 != lib.srh_view_grad_workspace_bytes(2, 16, 12)
    assert _size(lib, n_views=1, width=64, height=65) == 65 * 96
    for w, h in ((16, 12), (48, 36), (64, 64)):                               # doubles when W H doubles
        assert _size(lib, width=2 * w, height=h) == 2 * _size(lib, width=w, height=h) > 0
        assert _size(lib, n_views=4, width=w, height=h) == 2 * _size(lib, n_views=2, width=w, height=h)
    assert _size(lib, which=3) == 0 and b"which" in lib.srh_last_error()      # still no buffer of that number
    assert _size(lib, which=5) == 0 and b"which" in lib.srh_last_error()
    assert _size(lib, n_views=0) == 0 and b"n_views" in lib.srh_last_error()


def test_the_dense_entry_point_refuses_by_name(lib):
    p, a, _ = _dense()
    fn = lib.srh_dense_projection_bwd_view
    need = _size(lib)
    assert call(fn, DPROJ, p, a, grad_view=None) == NULL and b"grad_view" in lib.srh_last_error()
    assert call(fn, DPROJ, p, a, grad_view=a + 4) == WORKSPACE
    assert b"grad_view" in lib.srh_last_error() and b"aligned" in lib.srh_last_error()
    for given in ({"view_workspace_bytes": need - 1}, {"view_workspace": None}, {"view_workspace": a + 4}):
        assert call(fn, DPROJ, p, a, **given) == WORKSPACE, given
        assert b"view_workspace" in lib.srh_last_error() and str(need).encode() in lib.srh_last_error()
    # the layer's own checks come first, as in srh_dense_projection_bwd
    for k in ("view", "surfels", "rgb"):
        assert call(fn, DPROJ, p, a, **{k: None}) == NULL and k.encode() in lib.srh_last_error()
    assert call(fn, DPROJ, p, a, g_out=None, g_mask=None) == NULL and b"g_out" in lib.srh_last_error()
    assert call(fn, DPROJ, p, a, saved_bytes=512) == WORKSPACE and b"saved" in lib.srh_last_error()
    assert call(fn, DPROJ, p, a, workspace_bytes=512) == WORKSPACE
    assert b"workspace" in lib.srh_last_error() and b"view_workspace" not in lib.srh_last_error()
    assert call(fn, DPROJ, p, a, rotated=None) == NULL and b"rotated" in lib.srh_last_error()
    assert fn(None, *[a if not k.endswith("_bytes") else BIG for k in DPROJ], None) == NULL
    assert b"params" in lib.srh_last_error()
    q, a2, _ = _dense(n_views=0)
    assert call(fn, DPROJ, q, a2) == RANGE and b"n_views" in lib.srh_last_error()
    q, a2, _ = _dense(has_rotated=0)
    assert call(fn, DPROJ, q, a2, rotated=None) == NULL and b"grad_rotated" in lib.srh_last_error()
    assert call(fn, DPROJ, q, a2) == TYPE and b"rotated" in lib.srh_last_error()


def test_the_dense_entry_point_takes_null_for_every_other_gradient(lib):
    """Camera-only: what srh_dense_projection_bwd refuses as `nothing requested` passes here, up to the first check
    behind it (the 512-byte stand-in for `saved`)."""
    p, a, _ = _dense()
    none = dict(grad_surfels=None, grad_rgb=None, grad_rotated=None)
    assert call(lib.srh_dense_projection_bwd, DPROJ[:-3], p, a, **none) == NULL
    assert b"grad_surfels" in lib.srh_last_error()
    assert call(lib.srh_dense_projection_bwd_view, DPROJ, p, a, saved_bytes=512, **none) == WORKSPACE
    assert b"saved" in lib.srh_last_error()
    assert call(lib.srh_dense_projection_bwd_view, DPROJ, p, a, view_workspace_bytes=8, **none) == WORKSPACE
    assert b"view_workspace" in lib.srh_last_error()


def test_the_normals_entry_point_refuses_by_name(lib):
    _, a, _buf = _dense()
    need = lib.srh_view_grad_workspace_bytes(2, 16, 12)
    assert need == 2 * 12 * 8
    for k in ("rot", "pos", "g_out"):                          # rot: the gradient exists in the world frame only
        assert _normals(lib, a, **{k: None}) == NULL and k.encode() in lib.srh_last_error()
    assert _normals(lib, a, grad_rot=None) == NULL and b"grad_rot" in lib.srh_last_error()
    assert _normals(lib, a, grad_rot=a + 4) == WORKSPACE
    assert b"grad_rot" in lib.srh_last_error() and b"aligned" in lib.srh_last_error()
    for given in ({"view_workspace_bytes": need - 1}, {"view_workspace": None}, {"view_workspace": a + 4}):
        assert _normals(lib, a, **given) == WORKSPACE, given
        assert b"view_workspace" in lib.srh_last_error() and str(need).encode() in lib.srh_last_error()
    assert _normals(lib, a, workspace_bytes=512) == WORKSPACE
    assert b"workspace" in lib.srh_last_error() and b"view_workspace" not in lib.srh_last_error()
    assert _normals(lib, a, n_views=0) == RANGE and b"n_views" in lib.srh_last_error()
    assert _normals(lib, a, width=1) == RANGE and b"stencil" in lib.srh_last_error()


def test_the_normals_entry_point_takes_null_for_grad_pos(lib):
    """Without grad_pos the moments' workspace is not asked for: a NULL workspace of 0 bytes passes, up to the next
    check (here a short view_workspace)."""
    _, a, _buf = _dense()
    assert _normals(lib, a, grad_pos=None, workspace=None, workspace_bytes=0, view_workspace_bytes=8) == WORKSPACE
    assert b"view_workspace" in lib.srh_last_error()
    assert _normals(lib, a, workspace=None, workspace_bytes=0, view_workspace_bytes=8) == WORKSPACE
    assert b"view_workspace" not in lib.srh_last_error()        # with grad_pos the workspace is checked, and first
