"""srh_view_grad_workspace_bytes, srh_depth_to_surfels_bwd_view, srh_projection_bwd_view and
srh_reverse_projection_bwd_view: exported, bound, and their argument checks -- which return before any HIP call, so they
run without a GPU.  Host buffers stand in for device pointers: no call here reaches a launch."""
import ctypes as C

import pytest

from projection_abi import NULL, RANGE, TYPE, WORKSPACE, call, pointers, valid_params
from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _surfels(**fields):
    return valid_params(_lib.SrhSurfelsParams, **dict(dict(n_views=2, width=16, height=12, frame=1, fovy=0.7,
                                                           focal_length=0.5), **fields))


def _projection(**fields):
    return valid_params(_lib.SrhProjectionParams, **dict(dict(n_views=2, width=16, height=12, channels=3, flags=3,
                                                              blur_half=1, fovy=0.7, focal_length=0.5), **fields))


def _reverse(**fields):
    return valid_params(_lib.SrhReverseProjectionParams, **dict(dict(
        n_views=2, width=16, height=12, channels=3, fovy1=0.7, focal_length1=0.5, fovy2=0.9, focal_length2=0.8,
        depth_epsilon=0.1), **fields))


VIEW = ("view_workspace", "view_workspace_bytes")
LIFT = ("view", "depth", "g_out", "grad_depth", "grad_view") + VIEW
PROJ = ("view", "surfels", "rgb", "rotated", "saved", "saved_bytes", "workspace", "workspace_bytes", "g_out", "g_mask",
        "g_image1", "g_depth", "grad_surfels", "grad_rgb", "grad_rotated", "grad_view") + VIEW
RPROJ = ("view1", "view2", "rgb", "in_pos", "out_pos", "mask", "keys", "order", "workspace", "workspace_bytes", "g_out",
         "g_image1", "g_depth", "grad_rgb", "grad_in_pos", "grad_out_pos", "grad_rotated", "grad_view1", "grad_view2") + VIEW
ENTRIES = {"srh_depth_to_surfels_bwd_view": (_surfels, LIFT, ("grad_view",)),
           "srh_projection_bwd_view": (_projection, PROJ, ("grad_view",)),
           "srh_reverse_projection_bwd_view": (_reverse, RPROJ, ("grad_view1", "grad_view2"))}


def _call(lib, name, **given):
    valid, spec, _ = ENTRIES[name]
    p, a, _buf = valid()
    return call(getattr(lib, name), spec, p, a, **given)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name, (_, spec, _) in ENTRIES.items():
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(spec) + 2            # params in front, the stream behind
    assert "srh_view_grad_workspace_bytes" in _lib.EXPORTS and len(lib.srh_view_grad_workspace_bytes.argtypes) == 3


def test_the_workspace_is_one_set_of_sums_per_workgroup(lib):
    size = lib.srh_view_grad_workspace_bytes
    assert size(1, 1, 1) == 12 * 8 and size(3, 9, 17) == 3 * 12 * 8          # N = 153: one workgroup of 256
    assert size(1, 16, 16) == 12 * 8 and size(1, 257, 1) == 2 * 12 * 8
    assert size(1, 48, 36) == 7 * 12 * 8 and size(2, 4096, 4096) == 2 * 65536 * 12 * 8
    for bad, name in (((0, 4, 4), b"n_views"), ((65536, 4, 4), b"n_views"), ((1, 0, 4), b"width x height"),
                      ((1, 4, 0), b"width x height"), ((1, 4097, 4096), b"width x height")):
        assert size(*bad) == 0 and name in lib.srh_last_error(), bad


@pytest.mark.parametrize("name", ["srh_projection_bwd_view", "srh_reverse_projection_bwd_view"])
def test_a_valid_argument_list_passes_every_check_up_to_the_layers_scratch(lib, name):
    """The stand-in buffer is 512 bytes: with every size honest the first thing refused is the layer's own scratch
    buffer, which is too short, by name -- so every check in front of it passed.  (The lift has no scratch of its own:
    its honest call would launch.)"""
    valid, spec, _ = ENTRIES[name]
    assert _call(lib, name, **{k: 512 for k in spec if k.endswith("_bytes")}) == WORKSPACE
    assert b"view_workspace" not in lib.srh_last_error()
    assert b"saved" in lib.srh_last_error() or b"workspace" in lib.srh_last_error()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_nothing_requested_is_refused_by_name(lib, name):
    _, _, views = ENTRIES[name]
    assert _call(lib, name, **{k: None for k in views}) == NULL
    for k in views:
        assert k.encode() in lib.srh_last_error()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_misaligned_grad_view_is_refused_by_name(lib, name):
    valid, spec, views = ENTRIES[name]
    p, a, _buf = valid()
    for k in views:
        assert call(getattr(lib, name), spec, p, a, **{k: a + 4}) == WORKSPACE
        assert k.encode() in lib.srh_last_error() and b"aligned" in lib.srh_last_error()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_short_missing_or_misaligned_view_workspace_is_refused_by_name(lib, name):
    valid, spec, _ = ENTRIES[name]
    p, a, _buf = valid()
    need = lib.srh_view_grad_workspace_bytes(2, 16, 12)
    assert need == 2 * 12 * 8
    for given in ({"view_workspace_bytes": need - 1}, {"view_workspace": None}, {"view_workspace": a + 4}):
        assert call(getattr(lib, name), spec, p, a, **given) == WORKSPACE, given
        assert b"view_workspace" in lib.srh_last_error() and str(need).encode() in lib.srh_last_error()


def test_the_other_gradients_may_all_be_missing(lib):
    """Camera-only: what the plain entry points refuse as `nothing requested` passes here, up to the first check behind
    it (the 512-byte stand-in for `saved` / the launch-free argument checks are all that runs)."""
    p, a, _ = _projection()
    none = dict(grad_surfels=None, grad_rgb=None, grad_rotated=None)
    assert call(lib.srh_projection_bwd, PROJ[:-3], p, a, **none) == NULL
    assert call(lib.srh_projection_bwd_view, PROJ, p, a, saved_bytes=512, **none) == WORKSPACE
    assert b"saved" in lib.srh_last_error()
    p, a, _ = _reverse()
    none = dict(grad_rgb=None, grad_in_pos=None, grad_out_pos=None, grad_rotated=None)
    assert call(lib.srh_reverse_projection_bwd, RPROJ[:-4], p, a, **none) == NULL
    # camera 2 needs the walk: keys, order and the backward workspace, like grad_in_pos
    assert call(lib.srh_reverse_projection_bwd_view, RPROJ, p, a, keys=None, **none) == NULL
    assert b"keys" in lib.srh_last_error()
    assert call(lib.srh_reverse_projection_bwd_view, RPROJ, p, a, workspace_bytes=512, **none) == WORKSPACE
    assert b"workspace" in lib.srh_last_error() and b"view_workspace" not in lib.srh_last_error()


def test_the_lift_has_a_view_gradient_in_the_world_frame_only(lib):
    p, a, _ = _surfels(frame=0)
    assert call(lib.srh_depth_to_surfels_bwd_view, LIFT, p, a) == TYPE and b"frame" in lib.srh_last_error()
    p, a, _ = _surfels()
    for k in ("view", "depth", "g_out"):
        assert call(lib.srh_depth_to_surfels_bwd_view, LIFT, p, a, **{k: None}) == NULL
        assert k.encode() in lib.srh_last_error()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_the_layers_own_checks_come_first(lib, name):
    valid, spec, _ = ENTRIES[name]
    p, a, _buf = valid(n_views=0)
    assert call(getattr(lib, name), spec, p, a) == RANGE and b"n_views" in lib.srh_last_error()
    fn = getattr(lib, name)
    assert fn(None, *[a if not k.endswith("_bytes") else 1 << 40 for k in spec], None) == NULL
    assert b"params" in lib.srh_last_error()
    for k in pointers(spec)[:2]:
        p, a, _buf = valid()
        assert call(fn, spec, p, a, **{k: None}) == NULL and k.encode() in lib.srh_last_error(), k
