"""srh_frame_transform_fwd / _bwd / _bwd_view and srh_project_coordinates_fwd / _bwd / _bwd_view through ctypes: exported,
bound and declared; every refusal by parameter name (a refusal returns before any HIP call, so host buffers stand in for
device pointers there, and no such call is complete enough to reach a launch); and on the GPU the kernels under hand-made
tables, where the expected bits can be written down -- the identity, a pure translation, Z == 0, coordinates exactly on
a rounding tie, NaN and 1e30 -- with guard words behind every output and workspace buffer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from projection_abi import CAMERA, NULL, PINHOLE_ROWS, RANGE, WORKSPACE, call, valid_params
from surf_renderer_amd import _lib, build
from test_abi import declared_prototypes

DEV = "cuda:0"
gpu = pytest.mark.gpu
GUARD, SENTINEL = 64, -777

T_FWD = ("view_pos", "view_normal", "pos", "normal", "out_pos", "out_normal")
T_BWD = ("view_pos", "view_normal", "g_pos", "g_normal", "grad_pos", "grad_normal")
T_VIEW = ("view_pos", "view_normal", "pos", "normal", "g_pos", "g_normal", "grad_pos", "grad_normal", "grad_view_pos",
          "grad_view_normal", "view_workspace", "view_workspace_bytes")
P_FWD = ("view", "surfels", "plane", "px_coord", "px_idx")
P_BWD = ("view", "surfels", "g_plane", "g_coord", "grad_surfels")
P_VIEW = P_BWD + ("grad_view", "view_workspace", "view_workspace_bytes")
TRANSFORM = (("srh_frame_transform_fwd", T_FWD), ("srh_frame_transform_bwd", T_BWD),
             ("srh_frame_transform_bwd_view", T_VIEW))
PROJECT = (("srh_project_coordinates_fwd", P_FWD), ("srh_project_coordinates_bwd", P_BWD),
           ("srh_project_coordinates_bwd_view", P_VIEW))
# the pointers each entry point cannot do without, and the sets of which not all may be NULL
REQUIRED = {
    "srh_frame_transform_fwd": T_FWD,
    "srh_frame_transform_bwd": ("view_pos", "view_normal", "g_pos", "g_normal"),
    "srh_frame_transform_bwd_view": ("view_pos", "view_normal", "pos", "normal", "g_pos", "g_normal"),
    "srh_project_coordinates_fwd": ("view", "surfels"),
    "srh_project_coordinates_bwd": ("view", "surfels", "grad_surfels"),
    "srh_project_coordinates_bwd_view": ("view", "surfels", "grad_view"),
}
NOT_ALL_NULL = {
    "srh_frame_transform_bwd": [("grad_pos", "grad_normal")],
    "srh_frame_transform_bwd_view": [("grad_view_pos", "grad_view_normal")],
    "srh_project_coordinates_fwd": [("plane", "px_coord", "px_idx")],
    "srh_project_coordinates_bwd": [("g_plane", "g_coord")],
    "srh_project_coordinates_bwd_view": [("g_plane", "g_coord")],
}


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _frame(**fields):
    return valid_params(_lib.SrhFrameParams, **dict(dict(n_views=2, n_pos=7, n_normal=9, pos_cols=3, normal_cols=4),
                                                    **fields))


def _coords(**fields):
    return valid_params(_lib.SrhProjectCoordsParams, **dict(dict(n_views=2, n_points=7, cols=3, width=16, height=12,
                                                                 fovy=0.7, focal_length=0.5), **fields))


def _refused(lib, name, spec, p, a, code, shown, **given):
    assert call(getattr(lib, name), spec, p, a, **given) == code, (name, given)
    assert shown.encode() in lib.srh_last_error(), (name, given, lib.srh_last_error())


# ---- exported, bound, declared; refusals (no launch) -----------------------------------------------------------------
def test_entry_points_are_exported_bound_and_declared(lib):
    assert _lib.ABI_VERSION == 12 and lib.srh_abi_version() == 12           # added without a version change
    protos = declared_prototypes()
    for name, spec in TRANSFORM + PROJECT:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name in protos
        assert len(getattr(lib, name).argtypes) == len(spec) + 2 == len(protos[name][1])     # params, ..., stream
    assert C.sizeof(_lib.SrhFrameParams) == 5 * 4
    assert C.sizeof(_lib.SrhProjectCoordsParams) == 5 * 4 + 4 + 2 * 8


def test_null_arguments_are_refused_by_name(lib):
    for make, entries in ((_frame, TRANSFORM), (_coords, PROJECT)):
        p, a, _ = make()
        for name, spec in entries:
            fn = getattr(lib, name)
            assert fn(None, *[0 if k.endswith("_bytes") else a for k in spec], None) == NULL
            assert b"params" in lib.srh_last_error()
            for k in REQUIRED[name]:
                _refused(lib, name, spec, p, a, NULL, k, **{k: None})
            for group in NOT_ALL_NULL.get(name, ()):
                _refused(lib, name, spec, p, a, NULL, group[0], **{k: None for k in group})


def test_a_table_may_be_null_only_where_its_input_is_absent(lib):
    for absent, table, other in (("n_pos", "view_pos", "view_normal"), ("n_normal", "view_normal", "view_pos")):
        p, a, _ = _frame(**{absent: 0})
        for name, spec in TRANSFORM:
            # the absent input's table is not asked for: the refusal names the other one
            _refused(lib, name, spec, p, a, NULL, other, **{table: None, other: None})


def test_out_of_range_sizes_and_column_counts_are_refused_by_name(lib):
    rows = [("n_views", 0), ("n_views", 65536), ("n_pos", -1), ("n_pos", (1 << 24) + 1), ("n_normal", -1),
            ("n_normal", (1 << 24) + 1), ("pos_cols", 2), ("pos_cols", 5), ("normal_cols", 0), ("normal_cols", 5)]
    for field, value in rows:
        p, a, _ = _frame(**{field: value})
        for name, spec in TRANSFORM:
            _refused(lib, name, spec, p, a, RANGE, field)
    p, a, _ = _frame(n_pos=0, n_normal=0)
    for name, spec in TRANSFORM:
        _refused(lib, name, spec, p, a, RANGE, "both 0")
    rows = [("n_views", 0, RANGE), ("n_views", 65536, RANGE), ("n_points", 0, RANGE), ("n_points", (1 << 24) + 1, RANGE),
            ("cols", 2, RANGE), ("cols", 5, RANGE), ("width", 0, RANGE), ("height", 0, RANGE), ("width", 1 << 22, RANGE)]
    for field, value, code in rows + PINHOLE_ROWS + [("focal_length", -1.0, CAMERA)]:
        p, a, _ = _coords(**{field: value})
        for name, spec in PROJECT:
            _refused(lib, name, spec, p, a, code, {"width": "width x height", "height": "width x height"}.get(field, field))


def test_a_missing_small_or_misaligned_workspace_is_refused(lib):
    size = lib.srh_view_grad_workspace_bytes
    for make, name, spec, need in ((_frame, *TRANSFORM[2], 2 * size(2, 9, 1)), (_coords, *PROJECT[2], size(2, 7, 1))):
        p, a, _ = make()
        assert need > 0
        _refused(lib, name, spec, p, a, WORKSPACE, "view_workspace", view_workspace=None)
        _refused(lib, name, spec, p, a, WORKSPACE, "view_workspace", view_workspace_bytes=need - 1)
        _refused(lib, name, spec, p, a, WORKSPACE, "view_workspace", view_workspace=a + 4)
    p, a, _ = _frame()
    name, spec = TRANSFORM[2]
    assert size(2, 9, 1) == 2 * 1 * 12 * 8                                   # one workgroup covers max(n_pos, n_normal) = 9
    _refused(lib, name, spec, p, a, WORKSPACE, "grad_view_normal", grad_view_normal=a + 4)
    p, a, _ = _coords()
    _refused(lib, *PROJECT[2], p, a, WORKSPACE, "grad_view", grad_view=a + 4)


# ---- the kernels under hand-made tables (GPU) ------------------------------------------------------------------------
def guarded(shape, dtype=torch.float32):
    """(the whole allocation, its head in `shape`): GUARD sentinel words behind the head, and the head filled with the
    sentinel too, so an element the kernel does not write shows."""
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return whole, whole[:n].view(shape)


def untouched(*wholes):
    torch.cuda.synchronize()
    for w in wholes:
        assert bool((w[-GUARD:] == SENTINEL).all())


def table(rows, B):
    return torch.tensor(rows, dtype=torch.float64, device=DEV).reshape(1, 12).repeat(B, 1).contiguous()


IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
SHIFT = (0.75, -2.5, 1.0 / 3.0)
TRANSLATION = [1, 0, 0, SHIFT[0], 0, 1, 0, SHIFT[1], 0, 0, 1, SHIFT[2]]


def ptr(t):
    return None if t is None else t.data_ptr()


def draw(shape, seed):
    """fp32 values in +-[0.25, 2]: none is a zero, so x + 0 keeps every bit"""
    rng = np.random.RandomState(seed)
    v = rng.uniform(0.25, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def transform(lib, B, pos, normal, rows_pos, rows_normal=None):
    p = _lib.SrhFrameParams(n_views=B, n_pos=0 if pos is None else pos.shape[1],
                            n_normal=0 if normal is None else normal.shape[1],
                            pos_cols=3 if pos is None else pos.shape[2], normal_cols=3 if normal is None else normal.shape[2])
    whole_p, out_pos = (None, None) if pos is None else guarded((*pos.shape[:2], 4))
    whole_n, out_normal = (None, None) if normal is None else guarded((*normal.shape[:2], 3))
    view_pos = None if pos is None else table(rows_pos, B)              # a table is NULL where its input is absent
    view_normal = None if normal is None else table(rows_normal or rows_pos, B)
    _lib.check(lib.srh_frame_transform_fwd(C.byref(p), ptr(view_pos), ptr(view_normal), ptr(pos), ptr(normal),
                                           ptr(out_pos), ptr(out_normal), None))
    untouched(*(w for w in (whole_p, whole_n) if w is not None))
    return p, view_pos, view_normal, out_pos, out_normal


@gpu
@pytest.mark.parametrize("n_pos,n_normal,pos_cols,normal_cols", [(153, 192, 3, 4), (192, 153, 4, 3), (300, None, 4, 3),
                                                                 (None, 1, 3, 3)])
def test_the_identity_reproduces_the_inputs_and_a_translation_shifts_pos_only(lib, n_pos, n_normal, pos_cols, normal_cols):
    B = 2
    pos = None if n_pos is None else draw((B, n_pos, pos_cols), 1)
    normal = None if n_normal is None else draw((B, n_normal, normal_cols), 2)
    for rows in (IDENTITY, TRANSLATION):
        _, _, _, out_pos, out_normal = transform(lib, B, pos, normal, rows)
        if pos is not None:
            w = pos[..., 3] if pos_cols == 4 else torch.ones_like(pos[..., 0])
            assert torch.equal(out_pos[..., 3], w)
            shift = torch.tensor(SHIFT if rows is TRANSLATION else (0.0, 0.0, 0.0), dtype=torch.float64, device=DEV)
            want = (pos[..., :3].double() + shift * w.double()[..., None]).float()       # one product, one sum: exact
            assert torch.equal(out_pos[..., :3], want)
        if normal is not None:
            assert torch.equal(out_normal, normal[..., :3])              # column 3 of the table is not read


@gpu
def test_the_backward_under_the_identity_and_the_table_gradients(lib):
    B, n_pos, n_normal = 2, 300, 153
    pos, normal = draw((B, n_pos, 4), 3), draw((B, n_normal, 4), 4)
    g_pos, g_normal = draw((B, n_pos, 4), 5), draw((B, n_normal, 3), 6)
    p, view_pos, view_normal, _, _ = transform(lib, B, pos, normal, IDENTITY)
    whole_p, grad_pos = guarded(pos.shape)
    whole_n, grad_normal = guarded(normal.shape)
    _lib.check(lib.srh_frame_transform_bwd(C.byref(p), ptr(view_pos), ptr(view_normal), ptr(g_pos), ptr(g_normal),
                                           ptr(grad_pos), ptr(grad_normal), None))
    untouched(whole_p, whole_n)
    assert torch.equal(grad_pos, g_pos)                                  # column 3: g_w + g . (0, 0, 0)
    assert torch.equal(grad_normal[..., :3], g_normal) and bool((grad_normal[..., 3] == 0).all())

    need = 2 * lib.srh_view_grad_workspace_bytes(B, max(n_pos, n_normal), 1)
    whole_w, ws = guarded((need // 8,), torch.float64)
    whole_vp, gv_pos = guarded((B, 12), torch.float64)
    whole_vn, gv_normal = guarded((B, 12), torch.float64)
    whole_p2, grad_pos2 = guarded(pos.shape)
    _lib.check(lib.srh_frame_transform_bwd_view(C.byref(p), ptr(view_pos), ptr(view_normal), ptr(pos), ptr(normal),
                                                ptr(g_pos), ptr(g_normal), ptr(grad_pos2), None, ptr(gv_pos),
                                                ptr(gv_normal), ptr(ws), need, None))
    untouched(whole_w, whole_vp, whole_vn, whole_p2)
    assert torch.equal(grad_pos2, grad_pos)                              # the plain backward's bits
    want_pos = torch.einsum("bnr,bnc->brc", g_pos[..., :3].double(), pos.double()).reshape(B, 12)
    want_normal = torch.zeros(B, 3, 4, dtype=torch.float64, device=DEV)
    want_normal[..., :3] = torch.einsum("bni,bnj->bij", normal[..., :3].double(), g_normal.double())
    torch.testing.assert_close(gv_pos, want_pos, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gv_normal, want_normal.reshape(B, 12), rtol=1e-12, atol=1e-12)
    assert bool((gv_normal.reshape(B, 3, 4)[..., 3] == 0).all())         # exactly


# A pinhole whose pixel scales are small integers: tan(fovy / 2) = 1/2 exactly, f = 1 and a 5 x 5 frame give h = w = 1,
# px_coord = (-4 x + 2.5, 4 y + 2.5) and u = px_coord_x - 0.5 = -4 x + 2, so every tie is a dyadic x.
def tie_pinhole():
    half = math.atan(0.5)
    for _ in range(8):
        if math.tan(half) == 0.5:
            break
        half = math.nextafter(half, 1.0 if math.tan(half) < 0.5 else 0.0)
    assert math.tan(half) == 0.5
    return dict(width=5, height=5, fovy=2 * half, focal_length=1.0)


def project(lib, surfels, want=("plane", "px_coord", "px_idx"), **pinhole):
    B, N, cols = surfels.shape
    p = _lib.SrhProjectCoordsParams(n_views=B, n_points=N, cols=cols, **pinhole)
    bufs = {"plane": guarded((B, N, 3)), "px_coord": guarded((B, N, 3)), "px_idx": guarded((B, N), torch.int32)}
    view = table(IDENTITY, B)
    _lib.check(lib.srh_project_coordinates_fwd(C.byref(p), ptr(view), ptr(surfels),
                                               *[ptr(bufs[k][1]) if k in want else None for k in P_FWD[2:]], None))
    untouched(*(bufs[k][0] for k in want))
    for k in set(bufs) - set(want):                                      # a NULL output: nothing else was written either
        assert bool((bufs[k][0] == SENTINEL).all())
    return p, view, {k: bufs[k][1] for k in want}


@gpu
def test_coordinates_on_a_tie_round_half_to_even_and_strays_go_to_the_dump_slot(lib):
    pin = tie_pinhole()
    u = np.array([-1.5, -0.5, 0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 1.0, 2.25])         # wanted px_coord - 0.5
    rows = []
    for z in (1.0, 2.0, -0.5):                                                  # X / Z is exact for each
        for ux in u:
            for vy in u:
                rows.append(((2.0 - ux) / 4.0 * z, (vy - 2.0) / 4.0 * z, z))
    for bad in (float("nan"), 1e30, -1e30, float("inf")):
        rows += [(bad, 0.0, 1.0), (0.0, bad, 1.0), (0.0, 0.0, bad if math.isnan(bad) else 1.0 / bad)]
    s = torch.tensor(rows, dtype=torch.float32, device=DEV)[None].contiguous()
    n_ties = 3 * len(u) ** 2
    _, _, out = project(lib, s, **pin)
    ux, vy = np.tile(np.repeat(u, len(u)), 3), np.tile(np.tile(u, len(u)), 3)
    assert np.array_equal(out["px_coord"][0, :n_ties, 0].cpu().numpy(), (ux + 0.5).astype(np.float32))
    assert np.array_equal(out["px_coord"][0, :n_ties, 1].cpu().numpy(), (vy + 0.5).astype(np.float32))
    rx, ry = np.rint(ux), np.rint(vy)                                           # ties to even; -0.5 -> -0, inside
    inside = (rx >= 0) & (rx <= 4) & (ry >= 0) & (ry <= 4)
    want = np.where(inside, ry * 5 + rx, 25).astype(np.int32)
    assert {0, 2, 4} <= set(rx[inside]) and (~inside).any()
    assert np.array_equal(out["px_idx"][0, :n_ties].cpu().numpy(), want)
    stray = out["px_idx"][0, n_ties:].cpu().numpy()
    # 1 / 1e30 as Z is a finite, tiny depth under x = y = 0: the centre pixel; every NaN, 1e30 or inf coordinate is dumped
    centre = np.array([False, False, False] + [False, False, True] * 3)
    assert np.array_equal(stray[~centre], np.full((~centre).sum(), 25, np.int32)) and np.all(stray[centre] == 12)
    only = project(lib, s, want=("px_idx",), **pin)[2]
    assert torch.equal(only["px_idx"], out["px_idx"])


@gpu
def test_a_zero_depth_divides_by_one_and_gives_z_no_gradient_through_x_and_y(lib):
    pin = dict(width=16, height=12, fovy=0.7, focal_length=0.5)
    s = draw((2, 153, 4), 7)
    s[..., 3] = 1.0
    dead = torch.zeros(2, 153, dtype=torch.bool, device=DEV)
    dead[:, ::3] = True
    s[..., 2] = torch.where(dead, torch.zeros_like(s[..., 2]), s[..., 2])
    p, view, out = project(lib, s, **pin)
    f = torch.tensor(0.5, dtype=torch.float64)
    assert torch.equal(out["plane"][..., :2][dead], (s[..., :2][dead].double() * f).float())          # X / 1
    assert bool((out["plane"][..., 2][dead] == 0).all())
    g_plane, g_coord = draw((2, 153, 3), 8), draw((2, 153, 3), 9)
    g_plane[..., 2], g_coord[..., 2] = 0.0, 0.0                          # the loss reads x and y only
    need = lib.srh_view_grad_workspace_bytes(2, 153, 1)
    for with_view in (False, True):
        whole, grad = guarded(s.shape)
        if with_view:
            whole_w, ws = guarded((need // 8,), torch.float64)
            whole_v, gv = guarded((2, 12), torch.float64)
            _lib.check(lib.srh_project_coordinates_bwd_view(C.byref(p), ptr(view), ptr(s), ptr(g_plane), ptr(g_coord),
                                                            ptr(grad), ptr(gv), ptr(ws), need, None))
            untouched(whole, whole_w, whole_v)
            assert bool(torch.isfinite(gv).all())
        else:
            _lib.check(lib.srh_project_coordinates_bwd(C.byref(p), ptr(view), ptr(s), ptr(g_plane), ptr(g_coord),
                                                       ptr(grad), None))
            untouched(whole)
        assert bool((grad[..., 2][dead] == 0).all()) and bool((grad[..., 2][~dead] != 0).all())
        assert bool((grad[..., 3] == 0).all())                           # the identity's column 3 is zero
        assert bool(torch.isfinite(grad).all())
