"""srh_mesh_sample_fwd / _bwd / _workspace_bytes through ctypes: exported, bound and declared under ABI version 12, and
every refusal by parameter name (a refusal returns before any HIP call, so host buffers stand in for device pointers,
and no such call is complete enough to reach a launch)."""
import ctypes as C

import pytest

from projection_abi import BIG, NULL, RANGE, WORKSPACE, call, valid_params
from surf_renderer_amd import _lib, build
from test_abi import declared_prototypes

FWD = ("v", "f", "eye", "uniforms", "workspace", "workspace_bytes", "pos", "normal", "face", "bary")
BWD = ("v", "f", "uniforms", "face", "sample_order", "corner_order", "g_pos", "g_normal", "workspace", "workspace_bytes",
       "grad_v")
ENTRIES = (("srh_mesh_sample_fwd", FWD), ("srh_mesh_sample_bwd", BWD))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _params(**fields):
    base = dict(n_views=2, n_vertices=5, n_faces=4, n_samples=7, faces_per_view=0, eye_per_view=0)
    return valid_params(_lib.SrhMeshSampleParams, **dict(base, **fields))


def _refused(lib, name, spec, p, a, code, shown, **given):
    assert call(getattr(lib, name), spec, p, a, **given) == code, (name, given)
    assert shown.encode() in lib.srh_last_error(), (name, given, lib.srh_last_error())


def test_entry_points_are_exported_bound_and_declared(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    protos = declared_prototypes()
    for name, spec in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name in protos
        assert len(getattr(lib, name).argtypes) == len(spec) + 2 == len(protos[name][1])     # params, ..., stream
    assert "srh_mesh_sample_workspace_bytes" in _lib.EXPORTS and "srh_mesh_sample_workspace_bytes" in protos
    assert C.sizeof(_lib.SrhMeshSampleParams) == 6 * 4
    assert _lib.MESH_MAX == 1 << 24


def test_the_workspace_sizes(lib):
    p, _, _ = _params()
    size = lib.srh_mesh_sample_workspace_bytes
    assert size(C.byref(p), _lib.MESH_WS_FWD) >= (2 * 4 + 2) * 8              # the cdf and the totals
    assert size(C.byref(p), _lib.MESH_WS_BWD) >= 2 * 4 * 9 * 8               # nine fp64 per face
    assert size(C.byref(p), 2) == 0 and b"which" in lib.srh_last_error()
    assert size(None, 0) == 0
    big, _, _ = _params(n_views=65535, n_faces=1 << 24)
    assert size(C.byref(big), _lib.MESH_WS_BWD) >= 65535 * (1 << 24) * 72    # size_t arithmetic


def test_null_params_and_inputs_are_refused_by_name(lib):
    p, a, _ = _params()
    for name, spec in ENTRIES:
        assert getattr(lib, name)(None, *[BIG if k.endswith("_bytes") else a for k in spec], None) == NULL
        assert b"params" in lib.srh_last_error()
    for k in ("v", "f", "uniforms", "pos", "normal", "face", "bary"):
        _refused(lib, *ENTRIES[0], p, a, NULL, k, **{k: None})
    for k in ("v", "f", "uniforms", "face", "sample_order", "corner_order", "grad_v"):
        _refused(lib, *ENTRIES[1], p, a, NULL, k, **{k: None})
    _refused(lib, *ENTRIES[1], p, a, NULL, "g_pos and g_normal", g_pos=None, g_normal=None)


def test_out_of_range_sizes_are_refused_by_name(lib):
    rows = [("n_views", 0), ("n_views", 65536), ("n_vertices", 0), ("n_vertices", (1 << 24) + 1), ("n_faces", 0),
            ("n_faces", -1), ("n_faces", (1 << 24) + 1), ("n_samples", 0), ("n_samples", (1 << 24) + 1)]
    for field, value in rows:
        p, a, _ = _params(**{field: value})
        for name, spec in ENTRIES:
            _refused(lib, name, spec, p, a, RANGE, field)
        assert lib.srh_mesh_sample_workspace_bytes(C.byref(p), 0) == 0


def test_a_missing_short_or_misaligned_workspace_is_refused(lib):
    p, a, _ = _params()
    for name, spec in ENTRIES:
        _refused(lib, name, spec, p, a, WORKSPACE, "workspace", workspace=None)
        _refused(lib, name, spec, p, a, WORKSPACE, "workspace", workspace_bytes=8)
        _refused(lib, name, spec, p, a, WORKSPACE, "workspace", workspace=a + 4)
