"""GPU: the front-to-back occlusion cull of the binned disc kernel (srh_binned.h, sweep_sorted) may only skip entries
that can neither win nor tie, so the binned frame must equal the all-pairs fp64 frame bit for bit -- image, depth and
nearest -- on scenes built to stress its certain-hit test, its depth bounds and its limits, and at the smallest
shapes that run one wave per tile by the tile count (>= 3072 tiles), where the sorted sweep runs by default: against
the all-pairs mode (exact), with a re-used workspace and with split stages."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from surf_renderer_amd import _lib, renderer, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _render(scene, **kw):
    from surf_renderer_amd import render
    res = render(scene, device="cuda:0", **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in ("image", "depth", "nearest")}


def _binned_equals_exact(scene):
    ref = _render(scene, mode="exact")
    for wpt in (0, 1):                                   # default launch shape, and one wave per tile (the culled path)
        got = _render(scene, mode="binned", waves_per_tile=wpt)
        for k in ("nearest", "depth", "image"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"binned (waves_per_tile {wpt}) vs exact: {k}")
    return ref


def _disc_scene(pos, nrm, rad, width=256, height=192, near=0.1, far=1000.0):
    from surf_renderer_amd import synthetic
    scene = synthetic.disk_cloud_scene(4, width, height)
    n = len(rad)
    scene["camera"]["near"], scene["camera"]["far"] = near, far
    scene["objects"]["disk"] = {
        "pos": np.concatenate([np.asarray(pos, np.float64), np.ones((n, 1))], axis=1).astype(np.float32),
        "normal": np.concatenate([np.asarray(nrm, np.float64), np.zeros((n, 1))], axis=1).astype(np.float32),
        "radius": np.asarray(rad, np.float32),
        "material_idx": np.zeros(n, dtype=np.int64)}
    return scene


def _facing(n):
    return np.tile([0.0, 0.0, 1.0], (n, 1))


def _cloud(rng, n, lo=-1.0, hi=0.0, radius=0.05):
    """small discs spread behind the stacks below (z in [lo, hi])"""
    pos = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.8, 0.8, n), rng.uniform(lo, hi, n)], axis=1)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[nrm[:, 2] < 0] *= -1.0
    return pos, nrm, np.full(n, radius)


def test_coplanar_stacks_cover_tiles_lowest_index_wins():
    """Stacks of identical discs (exact depth ties at every pixel) and of near-coplanar ones, each covering whole
    tiles, in front of a cloud: the certain hits make the cull skip the cloud, and the ties still go to the lowest index."""
    rng = np.random.RandomState(41)
    cp, cn, cr = _cloud(rng, 3000)
    k = 24
    same = np.tile([-0.4, 0.0, 0.5], (k, 1))                       # identical: ties everywhere
    near_cop = np.tile([0.4, 0.0, 0.5], (k, 1))
    near_cop[:, 2] += np.arange(k) * 1e-7                          # a few float ulps apart
    tilted = rng.normal(scale=1e-4, size=(k, 3)) + [0.0, 0.0, 1.0]
    tilted /= np.linalg.norm(tilted, axis=1, keepdims=True)
    pos = np.concatenate([cp[:1500], same, near_cop, cp[1500:]])
    nrm = np.concatenate([cn[:1500], _facing(k), tilted, cn[1500:]])
    rad = np.concatenate([cr[:1500], np.full(k, 0.45), np.full(k, 0.45), cr[1500:]])
    ref = _binned_equals_exact(_disc_scene(pos, nrm, rad))
    win = np.unique(ref["nearest"][np.isfinite(ref["depth"])])
    assert 1500 in win                                             # the lowest of the identical stack
    assert not np.isin(np.arange(1501, 1500 + k), win).any()


def test_front_discs_straddling_near_and_behind_far():
    """Discs whose balls cross the near plane (their hits may be clipped) and discs behind the far plane may give no
    certain hit; a cloud between them must still resolve exactly."""
    rng = np.random.RandomState(42)
    cp, cn, cr = _cloud(rng, 2500, lo=-0.6, hi=0.6)
    eye_z = 4.0
    straddle = np.stack([rng.uniform(-0.8, 0.8, 40), rng.uniform(-0.6, 0.6, 40), np.full(40, eye_z - 2.5)], axis=1)
    behind = np.stack([rng.uniform(-0.8, 0.8, 40), rng.uniform(-0.6, 0.6, 40), np.full(40, eye_z - 5.2)], axis=1)
    pos = np.concatenate([straddle, cp, behind])
    nrm = np.concatenate([_facing(40), cn, _facing(40)])
    rad = np.concatenate([np.full(40, 0.3), cr, np.full(40, 1.5)])
    _binned_equals_exact(_disc_scene(pos, nrm, rad, near=2.5, far=5.0))


def test_huge_and_non_finite_discs_in_front():
    """A disc of radius 2^30 (no usable ellipse: frame-wide list) and non-finite discs in front of small discs."""
    rng = np.random.RandomState(43)
    cp, cn, cr = _cloud(rng, 2000)
    bad = np.array([[0.0, 0.0, 0.8], [np.nan, 0.0, 0.8], [0.2, np.inf, 0.8], [0.1, 0.1, 0.9]])
    bad_n = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [np.nan, 0.0, 1.0]])
    pos = np.concatenate([bad, cp])
    nrm = np.concatenate([bad_n, cn])
    rad = np.concatenate([[0.3, 0.3, 0.3, 0.3], cr])
    _binned_equals_exact(_disc_scene(pos, nrm, rad))
    huge = np.concatenate([[[0.0, 0.0, 2.0 ** 30]], cp])          # its plane far beyond the eye
    _binned_equals_exact(_disc_scene(huge, np.concatenate([[[0.0, 1.0, 1e-3]], cn]),
                                     np.concatenate([[2.0 ** 30], cr])))
    wall = np.concatenate([[[0.0, 0.0, 0.9]], cp])                # a huge disc right in front of the cloud
    _binned_equals_exact(_disc_scene(wall, np.concatenate([_facing(1), cn]), np.concatenate([[2.0 ** 30], cr])))


def test_lists_beyond_the_sort_capacity():
    """Tiles with more than 128 entries keep the plain sweep; tiles with 65-128 sort two entries per lane."""
    from surf_renderer_amd import synthetic
    for n, radius in ((60000, 0.05), (12000, 0.05)):
        scene = synthetic.disk_cloud_scene(n, 256, 192, radius=radius, seed=44)
        ref = _binned_equals_exact(scene)
        assert np.isfinite(ref["depth"]).mean() > 0.3


def test_config2_bunny_splats():
    """Overlapping splats of one surface: many near ties in depth."""
    from surf_renderer_amd import synthetic
    for w, h in ((512, 512), (1024, 768)):
        _binned_equals_exact(synthetic.bunny_splat_scene(w, h))


# ---- the only shapes where the sorted sweep runs one wave per tile by the tile count (>= 3072 tiles) ------------------
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


def test_outputs_equal_all_pairs_with_the_cull_running(case):
    st = renderer.bin_statistics(case.buf, case.cam, rows=case.rows)
    entries = st["entries"][0]
    culled = int(((entries >= 9) & (entries <= 128)).sum())
    print(f"tiles with 9..128 entries: {culled} of {entries.size}, longest list {int(entries.max())}, frame-wide {st['wide']}")
    assert int(st["wide"].sum()) == 0 and culled >= 300      # the sorted sweep runs in a few hundred tiles
    for name, g, w in zip(("image", "depth", "nearest"), case.got, case.ref):
        assert torch.equal(g, w), name


def test_reused_workspace_renders_as_a_fresh_one():
    """A workspace of 0xFF bytes renders camera A, then camera B (another eye and fovy): B's outputs are those of a
    fresh workspace and of the all-pairs mode."""
    width, height, rows, _ = SHAPES["frame"]
    a = get_case("frame")
    scene_b = disc_scene(width, height, eye_z=3.1, fovy_deg=52.0)
    cam_b = renderer.camera_struct(scene_b["camera"])
    ws = a.buf.new_workspace(width, height)
    ws.fill_(0xFF)
    renderer.render_buffers(a.buf, a.cam, rows=rows, mode="binned", workspace=ws)
    got_b = renderer.render_buffers(a.buf, cam_b, rows=rows, mode="binned", workspace=ws)
    fresh = renderer.render_buffers(a.buf, cam_b, rows=rows, mode="binned", workspace=a.buf.new_workspace(width, height))
    assert same(got_b, fresh)
    assert same(got_b, renderer.render_buffers(a.buf, cam_b, rows=rows, mode="fast"))


def test_split_stages_give_the_single_calls_bits():
    width, height, rows, _ = SHAPES["frame"]
    a = get_case("frame")
    ws = a.buf.new_workspace(width, height)
    out = tuple(torch.zeros_like(t) for t in a.got)
    renderer.render_buffers(a.buf, a.cam, rows=rows, mode="binned", out=out, workspace=ws, stages=_lib.STAGE_BIN)
    renderer.render_buffers(a.buf, a.cam, rows=rows, mode="binned", out=out, workspace=ws, stages=_lib.STAGE_RENDER)
    assert same(out, a.got)


def test_sphere_batch_and_four_wave_disc_frame_equal_all_pairs():
    """A sphere batch (any size) and a 512 x 512 disc frame (1024 tiles: four waves per tile), on which the sorted sweep
    does not run, render as the all-pairs mode does."""
    spheres = synthetic.disk_cloud_scene(400, 1000, 790, radius=0.05)
    disk = spheres["objects"].pop("disk")
    spheres["objects"]["sphere"] = {"pos": disk["pos"], "radius": disk["radius"], "material_idx": disk["material_idx"]}
    for scene in (spheres, synthetic.disk_cloud_scene(3000, 512, 512, radius=0.05)):
        buf = renderer.flatten_scene(scene, device=DEV)
        cam = renderer.camera_struct(scene["camera"])
        width, height = renderer.frame_size(cam)
        ws = buf.new_workspace(width, height)
        got = renderer.render_buffers(buf, cam, mode="binned", workspace=ws)
        assert same(got, renderer.render_buffers(buf, cam, mode="fast"))


_DUMP = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from surf_renderer_amd import renderer, synthetic
scene = synthetic.disk_cloud_scene()
buf = renderer.flatten_scene(scene, "cuda:0")
cam = renderer.camera_struct(scene["camera"])
img, dep, near = renderer.render_buffers(buf, cam, mode="binned")
torch.cuda.synchronize()
np.savez(sys.argv[2], image=img.cpu().numpy(), depth=dep.cpu().numpy(), nearest=near.cpu().numpy())
"""


def test_config5_switch_on_and_off(tmp_path):
    """BASELINE config 5: the default build (cull on) and a build with -DSRH_OCCLUSION_CULL=0 render the same frame,
    equal to the all-pairs fp64 frame."""
    from surf_renderer_amd import build, renderer, synthetic
    lib_off = str(tmp_path / "libsrh_occl_off.so")
    proc = subprocess.run(build.command(["-DSRH_OCCLUSION_CULL=0"], out=lib_off), capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    out_off = str(tmp_path / "off.npz")
    env = dict(os.environ, SRH_LIB=lib_off)
    proc = subprocess.run([sys.executable, "-c", _DUMP, REPO, out_off], env=env, capture_output=True, text=True,
                          timeout=600)
    assert proc.returncode == 0, proc.stderr[-4000:]
    off = np.load(out_off)
    scene = synthetic.disk_cloud_scene()
    buf = renderer.flatten_scene(scene, "cuda:0")
    cam = renderer.camera_struct(scene["camera"])
    frames = {}
    for mode in ("exact", "binned"):
        img, dep, near = renderer.render_buffers(buf, cam, mode=mode)
        torch.cuda.synchronize()
        frames[mode] = {"image": img.cpu().numpy(), "depth": dep.cpu().numpy(), "nearest": near.cpu().numpy()}
    for k in ("nearest", "depth", "image"):
        np.testing.assert_array_equal(frames["binned"][k], frames["exact"][k], err_msg=f"cull on vs exact: {k}")
        np.testing.assert_array_equal(off[k], frames["exact"][k], err_msg=f"cull off vs exact: {k}")
