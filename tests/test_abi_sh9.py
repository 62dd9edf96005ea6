"""srh_sh9_project_fwd / _bwd, srh_sh9_irradiance_fwd / _bwd and srh_sh9_workspace_bytes through ctypes: exported, bound
and declared under ABI version 12, and every refusal by parameter name (a refusal returns before any HIP call, so host
buffers stand in for device pointers, and no such call is complete enough to reach a launch)."""
import ctypes as C

import pytest

from projection_abi import BIG, NULL, RANGE, WORKSPACE, call, valid_params
from surf_renderer_amd import _lib, build
from test_abi import declared_prototypes

PROJECT_FWD = ("envmap", "workspace", "workspace_bytes", "L")
PROJECT_BWD = ("g_L", "grad_envmap")
IRRADIANCE_FWD = ("M", "normal", "E")
IRRADIANCE_BWD = ("M", "normal", "g_E", "grad_normal", "grad_M", "workspace", "workspace_bytes")
PROBE = (("srh_sh9_project_fwd", PROJECT_FWD), ("srh_sh9_project_bwd", PROJECT_BWD))
NORMALS = (("srh_sh9_irradiance_fwd", IRRADIANCE_FWD), ("srh_sh9_irradiance_bwd", IRRADIANCE_BWD))
ENTRIES = PROBE + NORMALS


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _params(**fields):
    base = dict(n_views=2, height=5, width=7, n_points=300, channels=3, m_per_view=1)
    return valid_params(_lib.SrhSh9Params, **dict(base, **fields))


def _refused(lib, name, spec, p, a, code, shown, **given):
    assert call(getattr(lib, name), spec, p, a, **given) == code, (name, given)
    assert shown.encode() in lib.srh_last_error(), (name, given, lib.srh_last_error())


def test_entry_points_are_exported_bound_and_declared(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    protos = declared_prototypes()
    for name, spec in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name in protos
        assert len(getattr(lib, name).argtypes) == len(spec) + 2 == len(protos[name][1])     # params, ..., stream
    assert "srh_sh9_workspace_bytes" in _lib.EXPORTS and "srh_sh9_workspace_bytes" in protos
    assert C.sizeof(_lib.SrhSh9Params) == 6 * 4
    assert [f for f, _ in _lib.SrhSh9Params._fields_] == ["n_views", "height", "width", "n_points", "channels", "m_per_view"]
    assert _lib.SH9_MAX == _lib.MESH_MAX == 1 << 24 and _lib.SH9_MAX_CHANNELS == 4


def test_the_workspace_sizes(lib):
    p, _, _ = _params()
    size = lib.srh_sh9_workspace_bytes
    assert size(C.byref(p), _lib.SH9_WS_PROJECT) >= 3 * 2 * 1 * 9 * 8         # 35 pixels: one workgroup per view
    assert size(C.byref(p), _lib.SH9_WS_IRRADIANCE_BWD) >= 3 * 2 * 2 * 10 * 8 + 2 * 3 * 10 * 8      # 300 normals: two
    assert size(C.byref(p), 2) == 0 and b"which" in lib.srh_last_error()
    assert size(None, 0) == 0 and b"params" in lib.srh_last_error()
    big, _, _ = _params(n_views=65535, height=4096, width=4096, n_points=1 << 24, channels=4)
    groups = (1 << 24) // 256
    assert size(C.byref(big), _lib.SH9_WS_PROJECT) >= 4 * 65535 * groups * 9 * 8 > 1 << 32           # size_t arithmetic
    assert size(C.byref(big), _lib.SH9_WS_IRRADIANCE_BWD) >= 4 * 65535 * groups * 10 * 8
    # each size reads its own half of the parameters
    probe_only, _, _ = _params(n_points=0)
    assert size(C.byref(probe_only), _lib.SH9_WS_PROJECT) > 0 and size(C.byref(probe_only), _lib.SH9_WS_IRRADIANCE_BWD) == 0
    normals_only, _, _ = _params(height=0, width=0)
    assert size(C.byref(normals_only), _lib.SH9_WS_IRRADIANCE_BWD) > 0 and size(C.byref(normals_only), _lib.SH9_WS_PROJECT) == 0


def test_null_params_and_inputs_are_refused_by_name(lib):
    p, a, _ = _params()
    for name, spec in ENTRIES:
        assert getattr(lib, name)(None, *[BIG if k.endswith("_bytes") else a for k in spec], None) == NULL
        assert b"params" in lib.srh_last_error()
    for name, spec in ENTRIES:
        for k in spec:
            if k.startswith("workspace") or k in ("grad_normal", "grad_M"):
                continue
            _refused(lib, name, spec, p, a, NULL, k, **{k: None})
    _refused(lib, *NORMALS[1], p, a, NULL, "grad_normal and grad_M", grad_normal=None, grad_M=None)
    _refused(lib, *NORMALS[1], p, a, WORKSPACE, "grad_M", grad_M=a + 4)               # fp64: 8-byte aligned


def test_out_of_range_sizes_are_refused_by_name(lib):
    both = [("n_views", 0), ("n_views", 65536), ("channels", 0), ("channels", 5), ("channels", -1)]
    probe = [("height", 0), ("width", 0), ("width", -3), ("height", 4097, "width", 4096)]
    normals = [("n_points", 0), ("n_points", -1), ("n_points", (1 << 24) + 1)]
    for rows, entries, which in ((both, ENTRIES, (0, 1)), (probe, PROBE, (0,)), (normals, NORMALS, (1,))):
        for row in rows:
            p, a, _ = _params(**dict(zip(row[0::2], row[1::2])))
            shown = "width x height" if row[0] in ("height", "width") else row[0]
            for name, spec in entries:
                _refused(lib, name, spec, p, a, RANGE, shown)
            for w in which:
                assert lib.srh_sh9_workspace_bytes(C.byref(p), w) == 0


def test_a_missing_short_or_misaligned_workspace_is_refused(lib):
    p, a, _ = _params()
    for name, spec in (PROBE[0], NORMALS[1]):
        _refused(lib, name, spec, p, a, WORKSPACE, "workspace", workspace=None)
        _refused(lib, name, spec, p, a, WORKSPACE, "workspace", workspace_bytes=8)
        _refused(lib, name, spec, p, a, WORKSPACE, "workspace", workspace=a + 4)
