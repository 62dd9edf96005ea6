"""srh_normals_workspace_bytes / _fwd / _bwd: exported, bound, declared, and their argument checks -- which return before
any HIP call, so they run without a GPU.  Host buffers stand in for device pointers: no call here reaches a launch."""
import ctypes as C

import pytest

from projection_abi import BIG, NULL, RANGE, WORKSPACE
from surf_renderer_amd import _lib, build
from test_abi import declared_prototypes

NAMES = ("srh_normals_workspace_bytes", "srh_normals_fwd", "srh_normals_bwd")
FWD = ("rot", "pos", "out")
BWD = ("rot", "pos", "g_out", "workspace", "workspace_bytes", "grad_pos")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


@pytest.fixture(scope="module")
def a():
    buf = (C.c_double * 64)()
    yield C.addressof(buf)
    del buf


def _call(fn, spec, a, size=(2, 16, 12), **given):
    return fn(*size, *[given.get(k, BIG if k.endswith("_bytes") else a) for k in spec], None)


def test_entry_points_are_exported_bound_and_declared(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    protos = declared_prototypes()
    for name in NAMES:
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name) and name in protos
    assert protos["srh_normals_workspace_bytes"][0] == "size_t" and lib.srh_normals_workspace_bytes.restype is C.c_size_t
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [3, 7, 10] == [len(protos[n][1]) for n in NAMES]
    import surf_renderer_amd
    for name in ("estimate_surface_normals_plane_fit_batched", "estimate_surface_normals_plane_fit",
                 "estimate_surface_normals"):
        assert name in surf_renderer_amd.__all__ and callable(getattr(surf_renderer_amd, name))


def test_the_workspace_is_five_doubles_per_point_and_never_zero_for_valid_sizes(lib):
    assert lib.srh_normals_workspace_bytes(2, 16, 12) == 2 * 16 * 12 * 5 * 8
    assert lib.srh_normals_workspace_bytes(1, 2, 2) == 160
    assert lib.srh_normals_workspace_bytes(65535, 4096, 4096) == 65535 * (1 << 24) * 40


def test_null_arguments_are_refused_by_name(lib, a):
    for fn, spec in ((lib.srh_normals_fwd, FWD), (lib.srh_normals_bwd, BWD)):
        for k in spec:
            if k in ("rot", "workspace", "workspace_bytes"):
                continue
            assert _call(fn, spec, a, **{k: None}) == NULL, k
            assert k.encode() in lib.srh_last_error(), k
            assert _call(fn, spec, a, rot=None, **{k: None}) == NULL, k      # the camera frame does without rot only
            assert k.encode() in lib.srh_last_error(), k


@pytest.mark.parametrize("size,what", [((0, 16, 12), b"n_views"), ((-1, 16, 12), b"n_views"), ((65536, 16, 12), b"n_views"),
                                       ((2, 1, 12), b"both sides >= 2"), ((2, 16, 1), b"both sides >= 2"),
                                       ((2, 0, 12), b"width x height"), ((2, 16, -3), b"width x height"),
                                       ((2, 4097, 4096), b"width x height"), ((2, 1 << 22, 8), b"width x height")])
def test_sizes_out_of_range_are_refused_by_name(lib, a, size, what):
    for fn, spec in ((lib.srh_normals_fwd, FWD), (lib.srh_normals_bwd, BWD)):
        assert _call(fn, spec, a, size=size) == RANGE
        assert what in lib.srh_last_error(), lib.srh_last_error()
    assert lib.srh_normals_workspace_bytes(*size) == 0
    assert what in lib.srh_last_error(), lib.srh_last_error()


def test_a_workspace_that_is_missing_small_or_misaligned(lib, a):
    need = lib.srh_normals_workspace_bytes(2, 16, 12)
    for given in ({"workspace": None}, {"workspace_bytes": need - 1}, {"workspace_bytes": 0}, {"workspace": a + 4}):
        assert _call(lib.srh_normals_bwd, BWD, a, **given) == WORKSPACE, given
        assert b"workspace" in lib.srh_last_error() and str(need).encode() in lib.srh_last_error()
    # the order of the checks: sizes, then NULL pointers, then the workspace
    assert _call(lib.srh_normals_bwd, BWD, a, size=(2, 1, 12), pos=None, workspace=None) == RANGE
    assert _call(lib.srh_normals_bwd, BWD, a, pos=None, workspace=None) == NULL
