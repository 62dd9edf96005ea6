"""bin_place picks a disc's tiles row by row from the closed form of its stored ellipse (ConicSpans, srh_reject.h).
Whatever it picks must hold every tile a hit can fall in -- so `binned` must reproduce the all-pairs fp64 mode bit for bit
-- and for slanted, elongated discs it must really leave the box corners out, tile for tile as the numpy model of the
rule says (tests/bin_spans_model.py; the model is compared only where it is 1e-3 away from every threshold, checked
without a GPU below, so that the kernel's Newton-refined arithmetic cannot decide differently).

Frames are 100 x 70 and 96 x 80 pixels (7 x 5 and 6 x 5 tiles: a diagonal disc crosses the whole frame's box, the nearest
these frames have to 6 x 6), the 100 x 70 scenes again as the row slab (5, 61); only the two discs whose boxes hold 8 x 8
and 9 x 8 tiles need a frame of 160 x 144."""
import functools

import numpy as np
import pytest

import bin_spans_model as M
from shadow_scenes import _base, light_views, shadow_both_ways
from test_hip_prep_bounds import _camera, _unit, f32, pixel_basis

EYE, AT = (0.3, 0.2, 4.0), (0.0, 0.0, 0.0)
FRAMES = {"100x70": (100, 70, None), "96x80": (96, 80, None), "100x70_rows_5_61": (100, 70, (5, 61))}


def _at_pixel(basis, c, r, depth=3.0):
    """world point on the ray of pixel (c, r), `depth` ray-direction lengths from the eye; the view direction and the
    image's right and down directions there (unit, perpendicular to the view direction); world length of one pixel"""
    eye, D0, Dc, Dr = basis
    D = D0 + c * Dc + r * Dr
    v = _unit(D)
    right = _unit(Dc - np.dot(Dc, v) * v)
    down = _unit(Dr - np.dot(Dr, v) * v)
    return eye + depth * D, v, right, down, depth * np.linalg.norm(Dc)


def facing(basis, c, r, radius_px, depth=3.0):
    p, v, _, _, px = _at_pixel(basis, c, r, depth)
    return p, -v, radius_px * px


def elongated(basis, c, r, half_px, ratio, deg, depth=3.0):
    """a disc seen asin(1 / ratio) from edge-on: its image is an ellipse of about that axis ratio whose major axis, about
    half_px pixels either way, makes `deg` degrees with the image's rows"""
    p, v, right, down, px = _at_pixel(basis, c, r, depth)
    major = np.cos(np.deg2rad(deg)) * right + np.sin(np.deg2rad(deg)) * down
    a = np.arcsin(1.0 / ratio)
    return p, np.sin(a) * v + np.cos(a) * np.cross(v, major), half_px * px


def scene_of_discs(cam, discs, seed=0, filler=0):
    rng = np.random.RandomState(seed)
    pos = [d[0] for d in discs] + list(np.array(cam["at"][:3]) + rng.uniform(-1.2, 1.2, (filler, 3)))
    nrm = [d[1] for d in discs] + list(rng.normal(size=(filler, 3)))
    rad = [d[2] for d in discs] + list(np.exp(rng.uniform(np.log(0.02), np.log(0.25), filler)))
    n = len(rad)
    order = rng.permutation(n)
    disk = {"pos": f32(np.concatenate([np.array(pos), np.ones((n, 1))], 1)[order]),
            "normal": f32(np.concatenate([np.array(nrm), np.zeros((n, 1))], 1)[order]), "radius": f32(np.array(rad)[order]),
            "material_idx": rng.randint(0, 3, n)}
    return {"camera": cam, "lights": {"pos": f32([[3, 4, 5, 1], [-4, 2, 3, 1]]), "color_idx": np.array([1, 2])},
            "colors": f32([[0, 0, 0], [.8, .5, .4], [.3, .6, .9]]),
            "materials": {"albedo": f32([[.5, .5, .5], [.9, .3, .2], [.2, .7, .4]])},
            "objects": {"disk": disk}, "tonemap": {"type": "gamma", "gamma": 0.8}}


# (axis ratio, degrees): about 100 and about 500 (the record's limit is 512), along the rows, the columns and both diagonals
DIAGONALS = [(ratio, deg) for ratio in (100.0, 470.0) for deg in (0.0, 45.0, 90.0, 135.0)]


def stored_axis_ratio(form):
    lam = np.linalg.eigvalsh(np.array([[form["A11"][0], form["A12"][0]], [form["A12"][0], form["A22"][0]]]))
    return float(np.sqrt(lam[1] / lam[0]))


def diagonal_disc(cam, ratio, deg):
    return _diagonal_disc(cam["viewport"][2], cam["viewport"][3], cam["near"], ratio, deg)


@functools.lru_cache(maxsize=None)
def _diagonal_disc(W, H, near, ratio, deg):
    """A disc 75 px either way is tens of degrees wide in these frames, and perspective rounds its image: the slant is
    bisected until the STORED form has the axis ratio asked for."""
    basis = pixel_basis(_camera(W, H, EYE, AT, near=near))[:4]
    lo, hi = ratio, 40.0 * ratio
    for _ in range(40):
        mid = np.sqrt(lo * hi)
        # off the tile corners and off the frame's centre, so that no tile edge runs along the ellipse's axis
        p, n, r = elongated(basis, 0.5 * W - 3.3, 0.5 * H + 2.7, 75.0, mid, deg)
        try:
            got = stored_axis_ratio(M.disc_records(basis, W, H, f32([p]), f32([n]), f32([r]))[0])
        except AssertionError:                     # no record of its own at that slant: too far
            got = np.inf
        lo, hi = (mid, hi) if got < ratio else (lo, mid)
    return elongated(basis, 0.5 * W - 3.3, 0.5 * H + 2.7, 75.0, lo, deg)


def special_discs(cam):
    """name -> discs, on the frame of `cam`"""
    W, H = cam["viewport"][2:]
    basis = pixel_basis(cam)[:4]
    g = {}
    # sub-pixel discs whose centres sit on a tile's first column / row, half a pixel before it, and on the half pixel
    # behind its last one
    g["sub_pixel_on_tile_edges"] = [facing(basis, c, r, rad) for k in range(1, 5) for c in (16.0 * k, 16.0 * k - 0.5, 16.0 * k + 15.5)
                                    for r, rad in ((16.0 * ((k % 3) + 1), 0.2), (16.0 * ((k % 3) + 1) - 0.5, 0.45), (16.0 * (k % 3) + 15.5, 0.05))
                                    if c < W and r < H]
    g["diagonal"] = [diagonal_disc(cam, ratio, deg) for ratio, deg in DIAGONALS]
    # discs that cut every edge and every corner of the image
    g["cut_every_edge"] = [facing(basis, c, r, 14.0) for c, r in ((0.0, 0.5 * H), (W - 1.0, 0.4 * H), (0.45 * W, 0.0), (0.6 * W, H - 1.0),
                                                                  (-3.0, -2.0), (W + 2.0, -4.0), (-5.0, H + 3.0), (W + 1.0, H + 1.0))]
    # slanted enough for the plane's horizon (n.D = 0) to run through the disc's box, beside its image
    g["plane_behind_the_eye_in_its_box"] = [elongated(basis, 0.3 * W, 0.6 * H, 40.0, 12.0, 40.0, depth=2.0),
                                            elongated(basis, 0.7 * W, 0.4 * H, 35.0, 30.0, 120.0, depth=2.5)]
    return g


@functools.lru_cache(maxsize=None)
def combined(frame, near):
    W, H, rows = FRAMES[frame]
    cam = _camera(W, H, EYE, AT, near=near)
    groups = special_discs(cam)
    return scene_of_discs(cam, [d for grp in groups.values() for d in grp], seed=11, filler=400), rows


def _render(scene, rows, mode):
    import torch
    from surf_renderer_amd import render
    res = render(scene, device="cuda:0", mode=mode, **({} if rows is None else {"rows": rows}))
    torch.cuda.synchronize()
    return {k: res[k].clone() for k in ("image", "depth", "nearest")}


def _assert_binned_equals_exact(tag, scene, rows, need_hit=True):
    import torch
    ref, got = _render(scene, rows, "exact"), _render(scene, rows, "binned")
    hit = int((ref["depth"] < 3e38).sum())
    print(f"{tag}: {hit} of {ref['depth'].numel()} pixels hit")
    assert hit > 0 or not need_hit
    for k in ("nearest", "depth", "image"):
        assert torch.equal(got[k], ref[k]), f"{tag}: {k} differs on {int((got[k] != ref[k]).sum())} values"


# ---- what the model says about the diagonal discs (no GPU) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_tiles(frame, ratio, deg, near=1.0):
    """(reached (tile rows, tile columns) bool, in the box bool, margin) for the one-disc scene: `margin` is the distance
    of the nearest tile decision from its threshold (q against 1.000001, the `behind` value against hi in units of the
    estimate's terms)."""
    W, H, rows = FRAMES[frame]
    cam = _camera(W, H, EYE, AT, near=near)
    p, n, r = diagonal_disc(cam, ratio, deg)
    form, est, (hc, hr) = M.disc_records(pixel_basis(cam)[:4], W, H, f32([p]), f32([n]), f32([r]))
    grid = M.Grid(W, rows or (0, H), 0.0)
    box = M.tile_box(form, grid, hc, hr)
    inside = M.in_box(box, grid)
    qmin = M.per_tile_min(form, grid)
    reached = inside & (qmin <= M.LAMBDA)
    by_spans, usable = M.span_set(form, grid, box)
    assert usable.all() and np.array_equal(by_spans, reached)
    margin = np.abs(qmin - M.LAMBDA)[inside].min()
    if near > 0.0:
        e = lambda v: v[:, None, None]                                 # noqa: E731
        den = e(est["u0"]) + np.maximum(e(est["u1"]) * grid.pc0[None, None, :], e(est["u1"]) * grid.pc1[None, None, :]) + \
            np.maximum(e(est["u2"]) * grid.pr0[None, :, None], e(est["u2"]) * grid.pr1[None, :, None])
        scale = abs(est["u0"][0]) + abs(est["u1"][0]) * W + abs(est["u2"][0]) * H
        # (only where the ellipse reaches: the other tiles are out whatever the estimate says)
        margin = min(margin, (np.abs(den - e(est["hi"])) / scale)[reached].min())
        reached = reached & ~M.behind_tiles(est, grid)
    return reached[0], inside[0], float(margin), stored_axis_ratio(form)


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("ratio,deg", DIAGONALS)
def test_model_keeps_the_diagonal_discs_off_every_threshold(frame, ratio, deg):
    reached, inside, margin, got_ratio = expected_tiles(frame, ratio, deg)
    W, H, rows = FRAMES[frame]
    print(f"{frame} ratio {ratio} at {deg}: stored axis ratio {got_ratio:.1f}, box {int(inside.sum())} tiles, reached {int(reached.sum())}, "
          f"margin {margin:.2e}")
    assert margin >= 1e-3
    assert 0.8 * ratio < got_ratio < 512.0
    if deg in (45.0, 135.0):
        # the whole frame's box, and most of it dropped
        assert inside.sum() >= 0.8 * inside.size and reached.sum() <= 0.5 * inside.sum()
    assert reached.sum() >= 4


@pytest.mark.parametrize("frame", list(FRAMES))
def test_the_horizon_runs_through_the_boxes_of_the_slanted_discs(frame):
    """The discs of `plane_behind_the_eye_in_its_box` do what their name says: the worst corner of either box is behind the
    eye, so the kernel takes the per-row `behind` test for them (behind_runs counts them), and whole tiles of the box are
    behind.  No row of theirs is MIXED, and none can be: a tile that lies wholly behind the eye holds no point of the
    disc's own image, so the ellipse's run never reaches one.  The shortcut's equality with the per-tile expression on
    mixed rows rests on tests/test_bin_spans_model.py; here the GPU run shows that the path drops no tile it must keep."""
    W, H, rows = FRAMES[frame]
    cam = _camera(W, H, EYE, AT, near=1.0)
    discs = special_discs(cam)["plane_behind_the_eye_in_its_box"]
    form, est, (hc, hr) = M.disc_records(pixel_basis(cam)[:4], W, H, f32([d[0] for d in discs]), f32([d[1] for d in discs]),
                                         f32([d[2] for d in discs]))
    grid = M.Grid(W, rows or (0, H), 0.0)
    box = M.tile_box(form, grid, hc, hr)
    assert box[4].all()
    ta, tb, usable = M.span_runs(form, grid, box)
    ty = np.arange(grid.tiles_y)[None, :]
    in_rows = (ty >= box[2][:, None]) & (ty <= box[3][:, None])
    ta, tb = np.where(in_rows, ta, 1), np.where(in_rows, tb, 0)
    ta2, tb2, mixed, tested = M.behind_runs(est, grid, ta, tb, box)
    behind = (M.behind_tiles(est, grid) & M.in_box(box, grid)).sum(axis=(1, 2))
    print(f"{frame}: tiles of the boxes behind the eye {behind.tolist()}, discs that take the test {tested}, mixed rows {mixed}")
    assert usable.all() and tested == len(discs) and (behind >= 2).all()
    assert mixed == 0 and np.array_equal(ta2, ta) and np.array_equal(tb2, tb)


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("near", [1.0, 0.0])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_binned_equals_exact(frame, near):
    scene, rows = combined(frame, near)
    _assert_binned_equals_exact(f"{frame} near {near}", scene, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("near", [1.0, 0.0])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_diagonal_discs_drop_the_box_corners(frame, near):
    """One disc per scene: the bins' lengths are the disc's tile set."""
    from surf_renderer_amd import renderer
    W, H, rows = FRAMES[frame]
    cam = _camera(W, H, EYE, AT, near=near)
    for ratio, deg in DIAGONALS:
        scene = scene_of_discs(cam, [diagonal_disc(cam, ratio, deg)])
        want, inside, margin, _ = expected_tiles(frame, ratio, deg, near)
        assert margin >= 1e-3
        buf = renderer.flatten_scene(scene, device="cuda:0")
        st = renderer.bin_statistics(buf, renderer.camera_struct(scene["camera"]), rows=rows)
        got = st["entries"][0]
        print(f"{frame} near {near} ratio {ratio} at {deg}: box {int(inside.sum())} tiles, {int(got.sum())} entries, model {int(want.sum())}")
        assert int(st["wide"].sum()) == 0
        assert np.array_equal(got, want.astype(got.dtype)), (got, want.astype(int))
        # (an ellipse a third of a pixel wide along a row may pass between the pixel centres: no hit is asked for)
        _assert_binned_equals_exact(f"{frame} ratio {ratio} at {deg}", scene, rows, need_hit=False)


@pytest.mark.gpu
def test_boxes_of_64_and_72_tiles():
    """A disc facing the camera at the image's centre line projects to a circle: radius 60 px around (80, 80) has the box
    19..141 both ways, 8 x 8 tiles, and is placed; around (72, 80) its columns are 11..133, 9 tiles: the frame-wide list."""
    from surf_renderer_amd import renderer
    cam = _camera(160, 144, (0.0, 0.0, 4.0), (0.0, 0.0, 0.0))
    eye, D0, Dc, Dr, m = pixel_basis(cam)
    fwd = -m[:, 2]
    for cx, wide, cols in ((80.0, 0, 8), (72.0, 1, 9)):
        # parallel to the image plane, 3 focal lengths away: |Dc| world units per pixel and focal length
        p = eye + 3.0 * (D0 + cx * Dc + 80.0 * Dr)
        scene = scene_of_discs(cam, [(p, -fwd, 60.0 * 3.0 * np.linalg.norm(Dc))])
        buf = renderer.flatten_scene(scene, device="cuda:0")
        st = renderer.bin_statistics(buf, renderer.camera_struct(scene["camera"]))
        got = st["entries"][0]
        print(f"centre column {cx}: {int(got.sum())} entries, frame-wide {st['wide']}")
        assert int(st["wide"].sum()) == wide
        if not wide:
            ys, xs = np.nonzero(got)
            assert (xs.min(), xs.max(), ys.min(), ys.max()) == (1, 8, 1, 8) and got.max() == 1
            assert got[1, 1] == 0 and got[8, 8] == 0 and got[1, 8] == 0 and got[8, 1] == 0       # a circle's box corners
        else:
            assert got.sum() == 0
        _assert_binned_equals_exact(f"box of {cols} x 8 tiles", scene, None)


@pytest.mark.gpu
def test_shadow_pass_with_elongated_splats():
    """The light views bin with bin_pad = 1: discs seen nearly edge-on FROM THE LIGHTS (axis ratios 20-400 in their views),
    over a large receiver, the binned shadow pass against all pairs."""
    import torch
    rng = np.random.RandomState(5)
    lights = [(4.0, -4.8, 9.6), (-6.4, 1.6, 8.0)]
    n = 240
    pos = rng.uniform(-0.9, 0.9, (n, 3)) + np.array([0.0, 0.0, 1.0])
    nrm = np.empty((n, 3))
    for i in range(n):
        v = _unit(pos[i] - np.array(lights[i % 2]))
        w = _unit(np.cross(v, rng.normal(size=3)))
        a = np.arcsin(1.0 / np.exp(rng.uniform(np.log(20.0), np.log(400.0))))
        nrm[i] = np.sin(a) * v + np.cos(a) * w
    rad = np.exp(rng.uniform(np.log(0.05), np.log(0.6), n))
    disk = {"pos": f32(np.concatenate([np.concatenate([pos, [[0.0, 0.0, 0.0]]]), np.ones((n + 1, 1))], 1)),
            "normal": f32(np.concatenate([np.concatenate([nrm, [[0.0, 0.0, 1.0]]]), np.zeros((n + 1, 1))], 1)),
            "radius": f32(np.concatenate([rad, [3.0]])), "material_idx": rng.randint(0, 3, n + 1)}
    scene = _base(97, 65, (0.5, -4.0, 3.0), (0.0, 0.0, 0.5), {"disk": disk}, lights)
    views = light_views(scene)
    assert all(v is not None for v in views), "every light must have a view of its own: that is the path with bin_pad = 1"
    for rows in (None, (5, 61)):
        (img_b, vis_b, depth), (img_a, vis_a, _) = shadow_both_ways(scene, rows=rows)
        hit = torch.isfinite(depth) & (depth < 1e30)
        blocked = int(((vis_a & 3) != 3)[hit].sum())
        print(f"rows {rows}: {int(hit.sum())} hit pixels, {blocked} with a blocked light")
        assert blocked > 100
        assert torch.equal(vis_b, vis_a), int((vis_b != vis_a).sum())
        assert torch.equal(img_b, img_a)
