"""srh_nearest_points_fwd / _bwd through ctypes: exported, bound and declared under ABI version 12, and every refusal by
parameter name (a refusal returns before any HIP call, so host buffers stand in for device pointers, and no such call
is complete enough to reach a launch)."""
import ctypes as C

import pytest

from projection_abi import NULL, RANGE, call, valid_params
from surf_renderer_amd import _lib, build
from test_abi import declared_prototypes

FWD = ("u", "v", "dist_u", "idx_u", "dist_v", "idx_v")
BWD = ("u", "v", "idx_u", "idx_v", "order_u", "order_v", "g_dist_u", "g_dist_v", "grad_u", "grad_v")
ENTRIES = (("srh_nearest_points_fwd", FWD), ("srh_nearest_points_bwd", BWD))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _params(**fields):
    return valid_params(_lib.SrhPointSetParams, **dict(dict(n_views=2, n_u=7, n_v=9, dims=3, squared=0), **fields))


def _refused(lib, name, spec, p, a, code, shown, **given):
    assert call(getattr(lib, name), spec, p, a, **given) == code, (name, given)
    assert shown.encode() in lib.srh_last_error(), (name, given, lib.srh_last_error())


def test_entry_points_are_exported_bound_and_declared(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    protos = declared_prototypes()
    for name, spec in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name in protos
        assert len(getattr(lib, name).argtypes) == len(spec) + 2 == len(protos[name][1])     # params, ..., stream
    assert C.sizeof(_lib.SrhPointSetParams) == 5 * 4


def test_null_params_and_point_sets_are_refused_by_name(lib):
    p, a, _ = _params()
    for name, spec in ENTRIES:
        assert getattr(lib, name)(None, *[a] * len(spec), None) == NULL
        assert b"params" in lib.srh_last_error()
        for k in ("u", "v"):
            _refused(lib, name, spec, p, a, NULL, k, **{k: None})


def test_out_of_range_sizes_are_refused_by_name(lib):
    rows = [("n_views", 0), ("n_views", 65536), ("n_u", 0), ("n_u", -1), ("n_u", (1 << 24) + 1), ("n_v", 0),
            ("n_v", (1 << 24) + 1), ("dims", 0), ("dims", 5), ("dims", -3)]
    for field, value in rows:
        p, a, _ = _params(**{field: value})
        for name, spec in ENTRIES:
            _refused(lib, name, spec, p, a, RANGE, field)


def test_a_half_null_output_pair_is_refused_and_so_are_no_outputs_at_all(lib):
    p, a, _ = _params()
    name, spec = ENTRIES[0]
    for missing in ("dist_u", "idx_u", "dist_v", "idx_v"):
        _refused(lib, name, spec, p, a, NULL, missing, **{missing: None})
    _refused(lib, name, spec, p, a, NULL, "all NULL", dist_u=None, idx_u=None, dist_v=None, idx_v=None)


def test_a_backward_nobody_wants_or_without_what_it_reads_is_refused(lib):
    p, a, _ = _params()
    name, spec = ENTRIES[1]
    _refused(lib, name, spec, p, a, NULL, "grad_u and grad_v", grad_u=None, grad_v=None)
    _refused(lib, name, spec, p, a, NULL, "idx_u", idx_u=None)
    _refused(lib, name, spec, p, a, NULL, "idx_v", idx_v=None)
    _refused(lib, name, spec, p, a, NULL, "order_u", order_u=None)
    _refused(lib, name, spec, p, a, NULL, "order_v", order_v=None)
