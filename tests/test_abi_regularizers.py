"""srh_regularizers_workspace_bytes / srh_regularizers_fwd / srh_regularizers_bwd: exported, bound, and their argument
checks -- which return before any HIP call, so they run without a GPU.  Host buffers stand in for device pointers: no
call here reaches a launch."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _valid():
    buf = (C.c_double * 64)()
    p = _lib.SrhRegularizerParams(n_views=2, width=40, height=30, z_min=2.0, z_max=4.0, z_scale=2.0,
                                  unit_normal_scale=10.0)
    return p, C.addressof(buf), buf


def _fwd(lib, p, a, ws=None, ws_bytes=None, terms=True, stats=True, inputs=(True,) * 4):
    need = lib.srh_regularizers_workspace_bytes(p.n_views, p.width, p.height)
    return lib.srh_regularizers_fwd(C.byref(p), *[a if k else None for k in inputs], a if ws is None else ws,
                                    need if ws_bytes is None else ws_bytes, a if terms else None, a if stats else None,
                                    None)


def _bwd(lib, p, a, grads=(True,) * 4, stats=True, grad_terms=True, inputs=(True,) * 4):
    return lib.srh_regularizers_bwd(C.byref(p), *[a if k else None for k in inputs], a if stats else None,
                                    a if grad_terms else None, *[a if k else None for k in grads], None)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    for name in ("srh_regularizers_workspace_bytes", "srh_regularizers_fwd", "srh_regularizers_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(lib.srh_regularizers_fwd.argtypes) == 10
    assert len(lib.srh_regularizers_bwd.argtypes) == 12
    assert C.sizeof(_lib.SrhRegularizerParams) == 48
    from surf_renderer_amd import REGULARIZER_TERMS
    assert len(REGULARIZER_TERMS) == _lib.REG_TERMS == 7
    assert REGULARIZER_TERMS == ("z", "unit_normal", "normal_consistency", "spatial", "spatial_var",
                                 "image_depth_consistency", "away_from_camera")


def test_workspace_holds_one_row_of_twelve_doubles_per_workgroup_and_view(lib):
    assert lib.srh_regularizers_workspace_bytes(2, 40, 30) == 2 * 5 * 12 * 8        # 1200 pixels: 5 groups of 256
    assert lib.srh_regularizers_workspace_bytes(1, 2, 2) == 12 * 8
    assert lib.srh_regularizers_workspace_bytes(64, 128, 128) == 64 * 64 * 12 * 8
    for bad in ((0, 40, 30), (65536, 40, 30), (1, 1, 30), (1, 40, 1), (1, 8192, 8192)):
        assert lib.srh_regularizers_workspace_bytes(*bad) == 0 and lib.srh_last_error() != b"", bad


def test_null_arguments_are_refused(lib):
    p, a, _ = _valid()
    assert lib.srh_regularizers_fwd(None, a, a, a, a, a, 1 << 20, a, a, None) == -1           # SRH_E_NULL
    for k in range(4):
        assert _fwd(lib, p, a, inputs=tuple(i != k for i in range(4))) == -1
        assert _bwd(lib, p, a, inputs=tuple(i != k for i in range(4))) == -1
    assert _fwd(lib, p, a, terms=False) == -1 and _fwd(lib, p, a, stats=False) == -1
    assert _bwd(lib, p, a, stats=False) == -1 and _bwd(lib, p, a, grad_terms=False) == -1


def test_all_null_gradient_buffers_are_refused(lib):
    p, a, _ = _valid()
    assert _bwd(lib, p, a, grads=(False,) * 4) == -1
    assert b"all NULL" in lib.srh_last_error()


@pytest.mark.parametrize("field,value", [("n_views", 0), ("n_views", 65536), ("width", 1), ("height", 1), ("width", 0),
                                         ("z_min", 4.5), ("z_max", float("nan"))])
def test_out_of_range_parameters_are_refused(lib, field, value):
    p, a, _ = _valid()
    setattr(p, field, value)
    assert lib.srh_regularizers_fwd(C.byref(p), a, a, a, a, a, 1 << 30, a, a, None) == -2     # SRH_E_RANGE
    assert _bwd(lib, p, a) == -2


def test_the_reflected_stencil_needs_two_by_two(lib):
    p, a, _ = _valid()
    p.width = 1
    assert _fwd(lib, p, a, ws_bytes=1 << 20) == -2 and b"2 x 2" in lib.srh_last_error()


def test_a_short_missing_or_misaligned_workspace_is_refused(lib):
    p, a, _ = _valid()
    need = lib.srh_regularizers_workspace_bytes(p.n_views, p.width, p.height)
    assert _fwd(lib, p, a, ws_bytes=need - 1) == -4                                           # SRH_E_WORKSPACE
    assert str(need).encode() in lib.srh_last_error()
    assert lib.srh_regularizers_fwd(C.byref(p), a, a, a, a, None, need, a, a, None) == -4
    assert _fwd(lib, p, a, ws=a + 4) == -4
