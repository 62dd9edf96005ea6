"""The per-tile table of the occlusion cull's 1 / |D| bound (FrameDev::tile_rlen, include/srh.h: srh_tile_rlen).

k_prep writes one float per 16 x 16-pixel tile of a one-batch disc frame that runs one wave per tile (>= 3072 tiles,
which sets the smallest shapes usable here); the render kernel reads it instead of computing it in every tile's wave.
Checked: the table's contents against a numpy float64 evaluation of the same formula (exact), the outputs against the
all-pairs mode (exact), a re-used workspace, split stages, and the frames that have no table."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from surf_renderer_amd import _lib, renderer, synthetic

DEV = "cuda:0"
TILE = 16


def numpy_table(cam, rows):
    """tile_rlen_lo (srh_binned.h) for every tile of rows [r0, r1), in float64 with unfused multiply-adds in the
    source's order: the camera basis as camera_to_frame builds it for the numpy shading (srh.hip), pixel_plane_xy's
    linspace end-point rule, pixel_len2 at the four clamped corners, IEEE sqrt, division and the cast to float32."""
    W, H = cam.viewport[2] - cam.viewport[0], cam.viewport[3] - cam.viewport[1]
    r0, r1 = rows
    eye, at, up = list(cam.eye), list(cam.at), list(cam.up)
    z = [eye[i] - at[i] for i in range(4)]
    zl = 0.0
    for i in range(4):
        zl += z[i] * z[i]
    zl = math.sqrt(zl)
    ul = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    bz = [z[i] / zl for i in range(3)]
    by = [up[i] if cam.up_is_unit else up[i] / ul for i in range(3)]
    bx = [by[1] * bz[2] - by[2] * bz[1], by[2] * bz[0] - by[0] * bz[2], by[0] * bz[1] - by[1] * bz[0]]
    h = math.tan(cam.fovy / 2) * 2 * cam.focal_length
    half_w, half_h = h * (float(W) / float(H)) / 2, h / 2
    step_x = 2.0 / (W - 1) if W > 1 else 0.0
    step_y = -2.0 / (H - 1) if H > 1 else 0.0
    tiles_x, tiles_y = (W + TILE - 1) // TILE, (r1 - r0 + TILE - 1) // TILE
    tx, ty = np.meshgrid(np.arange(tiles_x), np.arange(tiles_y))
    ca, ra = TILE * tx, r0 + TILE * ty
    cb, rb = np.minimum(ca + TILE - 1, W - 1), np.minimum(ra + TILE - 1, r1 - 1)

    def len2(c, r):
        xs = np.where((W > 1) & (c == W - 1), 1.0, c.astype(np.float64) * step_x + -1.0)
        ys = np.where((H > 1) & (r == H - 1), -1.0, r.astype(np.float64) * step_y + 1.0)
        X, Y, Z = xs * half_w, ys * half_h, -cam.focal_length
        v = [(bx[i] * X + by[i] * Y) + bz[i] * Z for i in range(3)]
        return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]

    m2 = np.maximum(np.maximum(len2(ca, ra), len2(cb, ra)), np.maximum(len2(ca, rb), len2(cb, rb)))
    rl = (1.0 / np.sqrt(m2)).astype(np.float32)
    guard = (rl > np.float32(0.0)) & (rl < np.float32(1.0e30))
    return np.where(guard, rl, np.float32(0.0)).astype(np.float32), guard


def disc_scene(width, height, eye_z=4.0, fovy_deg=45.0, n=3000, radius=0.05):
    scene = synthetic.disk_cloud_scene(n, width, height, radius=radius)
    scene["camera"] = dict(scene["camera"], eye=[0.0, 0.0, eye_z, 1.0], fovy=float(np.deg2rad(fovy_deg)))
    return scene


class Case:
    """One shape: the scene on the GPU, the all-pairs outputs (computed once, never modified) and the binned frame with
    the workspace it ran in."""

    def __init__(self, width, height, rows, eye_z):
        self.rows = rows
        self.scene = disc_scene(width, height, eye_z)
        self.buf = renderer.flatten_scene(self.scene, device=DEV)
        self.cam = renderer.camera_struct(self.scene["camera"])
        self.ref = renderer.render_buffers(self.buf, self.cam, rows=rows, mode="fast")
        self.ws = self.buf.new_workspace(width, height)
        self.got = renderer.render_buffers(self.buf, self.cam, rows=rows, mode="binned", workspace=self.ws)
        torch.cuda.synchronize()


# 1000 x 790: 63 x 50 = 3150 tiles, neither side a multiple of 16 (clamped corners; the linspace end-point rule in the
# last column and the last row).  2048 wide, rows (37, 417) of 454: a slab with row0 > 0 whose last tile row is cut,
# 128 x 24 = 3072 tiles -- the fewest that still run one wave per tile.
SHAPES = {"frame": (1000, 790, (0, 790), 4.0), "slab": (2048, 454, (37, 417), 2.5)}
_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(*SHAPES[name])
    return _cases[name]


@pytest.fixture(params=sorted(SHAPES))
def case(request):
    return get_case(request.param)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_numpy_formula_has_no_guarded_tile():
    """The reference formula itself, on the CPU side of this test: no tile of the cameras used here hits the guard, so
    the device values are compared against real bounds, not zeros."""
    for width, height, rows, eye_z in SHAPES.values():
        cam = renderer.camera_struct(disc_scene(width, height, eye_z, n=1)["camera"])
        table, guard = numpy_table(cam, rows)
        assert guard.all() and np.isfinite(table).all() and (table > 0).all()
        assert table.shape == ((rows[1] - rows[0] + 15) // 16, (width + 15) // 16)
        assert table.size >= 3072


@pytest.mark.gpu
def test_table_equals_the_numpy_formula(case):
    got = renderer.tile_rlen_table(case.buf, case.cam, case.ws, rows=case.rows)
    want, guard = numpy_table(case.cam, case.rows)
    assert got is not None and got.shape == want.shape
    assert (want[~guard] == 0).all()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} tiles differ, first (ty, tx) = {bad[0]}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


@pytest.mark.gpu
def test_outputs_equal_all_pairs_with_the_cull_running(case):
    st = renderer.bin_statistics(case.buf, case.cam, rows=case.rows)
    entries = st["entries"][0]
    culled = int(((entries >= 9) & (entries <= 128)).sum())
    print(f"tiles with 9..128 entries: {culled} of {entries.size}, longest list {int(entries.max())}, frame-wide {st['wide']}")
    assert int(st["wide"].sum()) == 0 and culled >= 300      # the sorted sweep runs in a few hundred tiles
    for name, g, w in zip(("image", "depth", "nearest"), case.got, case.ref):
        assert torch.equal(g, w), name


@pytest.mark.gpu
def test_reused_workspace_holds_the_last_frames_table():
    """A workspace of 0xFF bytes renders camera A, then camera B (another eye and fovy): the table is B's, and B's
    outputs are those of a fresh workspace."""
    width, height, rows, _ = SHAPES["frame"]
    a = get_case("frame")
    scene_b = disc_scene(width, height, eye_z=3.1, fovy_deg=52.0)
    cam_b = renderer.camera_struct(scene_b["camera"])
    ws = a.buf.new_workspace(width, height)
    ws.fill_(0xFF)
    renderer.render_buffers(a.buf, a.cam, rows=rows, mode="binned", workspace=ws)
    got_b = renderer.render_buffers(a.buf, cam_b, rows=rows, mode="binned", workspace=ws)
    table_b = renderer.tile_rlen_table(a.buf, cam_b, ws, rows=rows)
    want_b, _ = numpy_table(cam_b, rows)
    want_a, _ = numpy_table(a.cam, rows)
    assert (want_a != want_b).any()
    assert np.array_equal(table_b.view(np.uint32), want_b.view(np.uint32))
    fresh = renderer.render_buffers(a.buf, cam_b, rows=rows, mode="binned", workspace=a.buf.new_workspace(width, height))
    assert same(got_b, fresh)
    assert same(got_b, renderer.render_buffers(a.buf, cam_b, rows=rows, mode="fast"))


@pytest.mark.gpu
def test_split_stages_give_the_single_calls_bits():
    width, height, rows, _ = SHAPES["frame"]
    a = get_case("frame")
    ws = a.buf.new_workspace(width, height)
    out = tuple(torch.zeros_like(t) for t in a.got)
    renderer.render_buffers(a.buf, a.cam, rows=rows, mode="binned", out=out, workspace=ws, stages=_lib.STAGE_BIN)
    renderer.render_buffers(a.buf, a.cam, rows=rows, mode="binned", out=out, workspace=ws, stages=_lib.STAGE_RENDER)
    assert same(out, a.got)


@pytest.mark.gpu
def test_frames_without_a_table():
    """A sphere batch (any size) and a 512 x 512 disc frame (1024 tiles: four waves per tile) have no table, and render
    as the all-pairs mode does."""
    spheres = synthetic.disk_cloud_scene(400, 1000, 790, radius=0.05)
    disk = spheres["objects"].pop("disk")
    spheres["objects"]["sphere"] = {"pos": disk["pos"], "radius": disk["radius"], "material_idx": disk["material_idx"]}
    for scene in (spheres, synthetic.disk_cloud_scene(3000, 512, 512, radius=0.05)):
        buf = renderer.flatten_scene(scene, device=DEV)
        cam = renderer.camera_struct(scene["camera"])
        width, height = renderer.frame_size(cam)
        ws = buf.new_workspace(width, height)
        got = renderer.render_buffers(buf, cam, mode="binned", workspace=ws)
        assert renderer.tile_rlen_table(buf, cam, ws) is None
        off, tx, ty = C.c_size_t(7), C.c_int32(), C.c_int32()
        rc = _lib.load().srh_tile_rlen(C.byref(buf.objects), width, height, 0, height, C.byref(off), C.byref(tx),
                                       C.byref(ty))
        assert rc == _lib.E_NOT_APPLICABLE and off.value == 0
        assert same(got, renderer.render_buffers(buf, cam, mode="fast"))


def test_no_table_is_reported_for_a_camera_without_near_clip():
    """With near <= 0 the cull is off and nobody writes the table; the library's helper sees no camera, so the wrapper
    answers for it (before it touches the library or the workspace)."""
    scene = disc_scene(1000, 790, n=1)
    scene["camera"]["near"] = 0.0
    assert renderer.tile_rlen_table(None, renderer.camera_struct(scene["camera"]), None) is None
