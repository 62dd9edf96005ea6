"""srh_render_views_aux, srh_camera_grad_scratch_bytes_views and srh_render_views_bwd_camera (ABI 11, added without a
version change): exported, bound, and the argument checks that return before any HIP call -- so they run without a GPU."""
import ctypes as C

import pytest

from surf_renderer_amd import _lib, build

E_NULL, E_RANGE, E_TYPE, E_WORKSPACE = -1, -2, -3, -4
W, H = 72, 22
# srh_workspace_bytes_views(one plane, 72, 22, n) of the commit before these entry points: they must not move it
WORKSPACE_BYTES_BEFORE = {1: 9984, 3: 29952, 256: 2539520}


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


class _Args:
    """A well-formed call over `n` 72 x 22 views of one plane; the device pointers are fakes (no check dereferences them)."""

    def __init__(self, lib, n=2, want=True):
        self.n = n
        m = max(n, 1)
        self.cams = (_lib.SrhCamera * m)()
        for cam in self.cams:
            cam.viewport[:] = [0, 0, W, H]
        self.ob, self.li, self.mat = _lib.SrhObjects(), _lib.SrhLights(), _lib.SrhMaterials()
        self.ob.n_segments = 1
        seg = self.ob.seg[0]
        seg.type, seg.count = 1, 1                              # one plane
        seg.pos = seg.normal = seg.material_idx = 0x1000
        self.params = _lib.SrhParams(row0=0, row1=H, shading=_lib.SHADING["torch"])
        self.grads = (_lib.SrhGrads * m)()
        self.cgrads = (_lib.SrhCameraGrads * m)()
        if want:
            self.cgrads[m - 1].at = 0x5000                      # one member of one view: the batch wants camera gradients
        self.need = lib.srh_workspace_bytes_views(C.byref(self.ob), W, H, min(m, 256))
        self.ws, self.ws_bytes = 0x10000, self.need
        self.g_img = self.g_dep = self.g_nrm = self.g_pos = self.near = self.depth = 0x2000
        self.scratch_need = lib.srh_camera_grad_scratch_bytes_views(W, H, min(m, 256))
        self.scratch, self.scratch_bytes = 0x40000, self.scratch_need

    def call(self, lib, **null):
        def arg(name, val):
            return None if null.get(name) else val
        return lib.srh_render_views_bwd_camera(
            self.n, arg("cameras", self.cams), C.byref(self.ob), C.byref(self.li), C.byref(self.mat),
            arg("params", C.byref(self.params)), arg("workspace", self.ws), self.ws_bytes, arg("grad_images", self.g_img),
            arg("grad_depths", self.g_dep), arg("grad_normals", self.g_nrm), arg("grad_poses", self.g_pos),
            arg("nearests", self.near), arg("depths", self.depth), arg("grads", self.grads),
            arg("camera_grads", self.cgrads), arg("camera_scratch", self.scratch), self.scratch_bytes, None)

    def fwd_aux(self, lib, normals=0x6000, poses=None):
        return lib.srh_render_views_aux(self.n, self.cams, C.byref(self.ob), C.byref(self.li), C.byref(self.mat),
                                        C.byref(self.params), self.ws, self.ws_bytes, 0x2000, 0x2000, None, normals,
                                        poses, None)


def test_entry_points_are_exported_and_bound(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12
    for name, nargs, restype in (("srh_render_views_bwd_camera", 19, C.c_int), ("srh_render_views_aux", 14, C.c_int),
                                 ("srh_camera_grad_scratch_bytes_views", 3, C.c_size_t)):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is restype, name


@pytest.mark.parametrize("n", [0, 257])
def test_view_count_out_of_range_is_refused(lib, n):
    assert _Args(lib, n).call(lib) == E_RANGE
    assert b"1..256" in lib.srh_last_error()


@pytest.mark.parametrize("name", ["cameras", "params", "workspace", "grads", "nearests", "depths"])
def test_null_argument_is_refused(lib, name):
    assert _Args(lib).call(lib, **{name: True}) == E_NULL
    assert name.encode() in lib.srh_last_error()


def test_all_four_upstream_gradients_null_is_refused(lib):
    a = _Args(lib)
    assert a.call(lib, grad_images=True, grad_depths=True, grad_normals=True, grad_poses=True) == E_NULL
    assert b"all NULL" in lib.srh_last_error()


def test_numpy_shading_is_refused(lib):
    a = _Args(lib)
    a.params.shading = _lib.SHADING["numpy"]
    assert a.call(lib) == E_TYPE
    assert b"SRH_SHADING_TORCH" in lib.srh_last_error()


def test_per_frame_outputs_are_refused(lib):
    a = _Args(lib)
    a.params.normal_out = 0x3000
    assert a.call(lib) == E_TYPE
    assert b"srh_render_views_bwd_camera" in lib.srh_last_error()


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


def test_camera_scratch_one_byte_short_is_refused_with_the_size_it_needs(lib):
    a = _Args(lib, 3)
    assert a.scratch_need > 0
    a.scratch_bytes = a.scratch_need - 1
    assert a.call(lib) == E_WORKSPACE
    assert str(a.scratch_need).encode() in lib.srh_last_error()


def test_misaligned_camera_scratch_is_refused_with_the_size_it_needs(lib):
    a = _Args(lib, 3)
    a.scratch += 4
    assert a.call(lib) == E_WORKSPACE
    assert str(a.scratch_need).encode() in lib.srh_last_error()
    assert a.call(lib, camera_scratch=True) == E_WORKSPACE    # wanted, and no scratch at all


@pytest.mark.parametrize("how", ["null array", "null members"])
def test_scratch_is_not_looked_at_when_no_camera_gradient_is_wanted(lib, how):
    """A NULL (or short, or misaligned) scratch passes every argument check; the call then fails only where it needs a
    device -- or, with a device present, is refused for its small workspace, the last check before any HIP call."""
    a = _Args(lib, 2, want=False)
    a.scratch_bytes = 0
    a.ws_bytes = a.need - 1                                  # stops the call after all argument checks, device or not
    null = {"camera_scratch": True}
    if how == "null array":
        null["camera_grads"] = True
    assert a.call(lib, **null) == E_RANGE
    assert str(a.need).encode() in lib.srh_last_error()
    a.ws_bytes = a.need
    a.scratch, a.scratch_bytes = 0x40004, 1
    a.params.per_view = 8                                    # a late check of ViewsCall::check: the scratch came earlier
    assert a.call(lib, **{k: v for k, v in null.items() if k != "camera_scratch"}) == E_TYPE
    assert b"per_view" in lib.srh_last_error()


def test_views_aux_refuses_numpy_shading_when_normals_is_set(lib):
    a = _Args(lib)
    a.params.shading = _lib.SHADING["numpy"]
    assert a.fwd_aux(lib) == E_TYPE
    assert b"SRH_SHADING_TORCH" in lib.srh_last_error()
    assert a.fwd_aux(lib, normals=None, poses=0x6000) == E_TYPE
    # ... and params.normal_out stays a per-frame feature
    a.params.shading = _lib.SHADING["torch"]
    a.params.normal_out = 0x3000
    assert a.fwd_aux(lib) == E_TYPE
    assert b"srh_render_views_aux" in lib.srh_last_error()


def test_batch_scratch_holds_a_slice_per_view(lib):
    one = lib.srh_camera_grad_scratch_bytes(W, H)
    assert one == 2 * 6 * 12 * 8                             # 2 x 6 workgroups, twelve fp64 sums each
    for n in (1, 2, 64, 256):
        need = lib.srh_camera_grad_scratch_bytes_views(W, H, n)
        assert need >= n * one and need % 8 == 0
    for args in ((W, H, 0), (W, H, 257), (0, H, 2), (W, 0, 2)):
        assert lib.srh_camera_grad_scratch_bytes_views(*args) == 0
        assert lib.srh_last_error()


def test_views_workspace_size_did_not_move(lib):
    a = _Args(lib)
    for n, want in WORKSPACE_BYTES_BEFORE.items():
        assert lib.srh_workspace_bytes_views(C.byref(a.ob), W, H, n) == want
