"""srh_render_views_bwd (ABI 11, added without a version change): exported, bound, and the argument checks that return
before any HIP call -- so they run without a GPU."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build

E_NULL, E_RANGE, E_TYPE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


class _Args:
    """A well-formed call over `n` 72 x 22 views of one plane; the device pointers are fakes (no check dereferences them)."""

    def __init__(self, lib, n=2):
        self.n = n
        self.cams = (_lib.SrhCamera * max(n, 1))()
        for cam in self.cams:
            cam.viewport[:] = [0, 0, 72, 22]
        self.ob, self.li, self.mat = _lib.SrhObjects(), _lib.SrhLights(), _lib.SrhMaterials()
        self.ob.n_segments = 1
        seg = self.ob.seg[0]
        seg.type, seg.count = 1, 1                              # one plane
        seg.pos = seg.normal = seg.material_idx = 0x1000
        self.params = _lib.SrhParams(row0=0, row1=22, shading=_lib.SHADING["torch"])
        self.grads = (_lib.SrhGrads * max(n, 1))()
        self.need = lib.srh_workspace_bytes_views(C.byref(self.ob), 72, 22, min(max(n, 1), 256))
        self.ws, self.ws_bytes = 0x10000, self.need
        self.g_img = self.g_dep = self.near = self.depth = 0x2000

    def call(self, lib, **null):
        def arg(name, val):
            return None if null.get(name) else val
        return lib.srh_render_views_bwd(self.n, arg("cameras", self.cams), C.byref(self.ob), C.byref(self.li),
                                        C.byref(self.mat), arg("params", C.byref(self.params)), arg("workspace", self.ws),
                                        self.ws_bytes, arg("grad_images", self.g_img), self.g_dep,
                                        arg("nearests", self.near), arg("depths", self.depth), arg("grads", self.grads),
                                        None)


def test_entry_point_is_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12
    assert "srh_render_views_bwd" in _lib.EXPORTS
    assert len(lib.srh_render_views_bwd.argtypes) == 14
    assert lib.srh_render_views_bwd.restype is C.c_int


@pytest.mark.parametrize("n", [0, 257])
def test_view_count_out_of_range_is_refused(lib, n):
    assert _Args(lib, n).call(lib) == E_RANGE
    assert b"1..256" in lib.srh_last_error()


@pytest.mark.parametrize("name", ["cameras", "params", "workspace", "grads", "nearests", "depths", "grad_images"])
def test_null_argument_is_refused(lib, name):
    assert _Args(lib).call(lib, **{name: True}) == E_NULL
    assert name.encode() in lib.srh_last_error()


def test_per_frame_outputs_are_refused(lib):
    a = _Args(lib)
    a.params.normal_out = 0x3000
    assert a.call(lib) == E_TYPE
    assert b"srh_render_views_bwd" in lib.srh_last_error()


def test_unknown_per_view_bit_is_refused(lib):
    a = _Args(lib)
    a.params.per_view = 8
    assert a.call(lib) == E_TYPE
    assert b"per_view" in lib.srh_last_error()


def test_small_workspace_is_refused_with_the_size_it_needs(lib):
    a = _Args(lib, 3)
    assert a.need > 0
    a.ws_bytes = a.need - 1
    assert a.call(lib) == E_RANGE
    assert str(a.need).encode() in lib.srh_last_error()


def test_workspace_has_room_for_the_gradient_descriptors(lib):
    """The header in front of the views' slices holds a frame descriptor and an SrhGrads-sized destination table per
    view: the views workspace is at least that much larger than n single-frame workspaces."""
    a = _Args(lib, 1)
    one = lib.srh_workspace_bytes(C.byref(a.ob), 72, 22)
    for n in (1, 2, 3, 64, 256):
        need = lib.srh_workspace_bytes_views(C.byref(a.ob), 72, 22, n)
        assert need >= n * one + n * C.sizeof(_lib.SrhGrads)
        assert (need - n * one) % 256 == 0
