"""bin_place claims the bin counters of tiles t and t ^ 1 with ONE 64-bit atomic on the aligned pair (srh_binned.h, pass 2).
The pairing must change nothing anybody can see: the bins hold the same (tile, primitive) sets as the numpy model of the
row-span rule says (tests/bin_spans_model.py, inputs 1e-3 from every threshold), and `binned` reproduces the all-pairs fp64
mode bit for bit.  Each case is the smallest frame that has its property: a pair word that straddles two tile rows (odd
tiles_x), runs that start on either half of a word, an odd tile count (the last word's other half is padding), one half
of a word past the bin's capacity, a second object batch, a light view (bin_pad = 1), and the counters left at zero.

As in test_hip_bin_spans.py the bins are read through their lengths: with one disc per scene the lengths ARE its tile set.
The model's count of pair words (tests/bin_pairs_model.py) is checked without a GPU at the end."""
import numpy as np
import pytest

import bin_pairs_model as P
import bin_spans_model as M
from shadow_scenes import _base, light_views, shadow_both_ways
from test_hip_bin_spans import AT, EYE, _assert_binned_equals_exact, facing, scene_of_discs
from test_hip_prep_bounds import _camera, _unit, f32, pixel_basis


# ---- the model's tile set of one disc ----------------------------------------------------------------------------------
def expected(cam, disc, rows=None):
    """(reached (tile rows, tile columns) bool, margin): the row-span rule's tile set of one disc, which must equal the
    per-tile rule's, and the distance of the nearest tile decision from its threshold."""
    W, H = cam["viewport"][2:]
    p, n, r = disc
    form, est, (hc, hr) = M.disc_records(pixel_basis(cam)[:4], W, H, f32([p]), f32([n]), f32([r]))
    grid = M.Grid(W, rows or (0, H), 0.0)
    box = M.tile_box(form, grid, hc, hr)
    inside = M.in_box(box, grid)
    qmin = M.per_tile_min(form, grid)
    reached = inside & (qmin <= M.LAMBDA)
    by_spans, usable = M.span_set(form, grid, box)
    assert usable.all() and np.array_equal(by_spans, reached)
    margin = np.abs(qmin - M.LAMBDA)[inside].min()
    # facing discs three ray lengths in front of the eye: no tile of their boxes is behind it
    assert not (M.behind_tiles(est, grid) & reached).any()
    return reached[0], float(margin)


def _bins(scene, rows=None):
    from surf_renderer_amd import renderer
    buf = renderer.flatten_scene(scene, device="cuda:0")
    return renderer.bin_statistics(buf, renderer.camera_struct(scene["camera"]), rows=rows)


def _counter_words(buf, cam, rows, ws):
    """the workspace's bin counters as the kernels index them, (batches, ntiles_pad), with (tiles_x, tiles_y, bin_cap)"""
    import ctypes as C
    import torch
    from surf_renderer_amd import _lib
    from surf_renderer_amd.frame import frame_size
    lib = _lib.load()
    width, height = frame_size(cam)
    r0, r1 = (0, height) if rows is None else rows
    off, tx, ty, pad, cap = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(lib.srh_bin_counters(C.byref(buf.objects), width, height, r0, r1, C.byref(off), C.byref(tx), C.byref(ty),
                                    C.byref(pad), C.byref(cap)))
    torch.cuda.synchronize()
    nseg = buf.objects.n_segments
    assert off.value % 8 == 0 and pad.value % 4 == 0          # what makes the 64-bit view of a pair legal
    words = ws[off.value:off.value + 4 * (64 + nseg * pad.value)].view(torch.int32).cpu().numpy().astype(np.int64)
    return words[64:].reshape(nseg, pad.value), (tx.value, ty.value, cap.value)


def _one_disc_case(tag, cam, disc, rows=None):
    """the disc alone: bins == model, binned == exact; returns the model's tile set"""
    want, margin = expected(cam, disc, rows)
    assert margin >= 1e-3, (tag, margin)
    scene = scene_of_discs(cam, [disc])
    st = _bins(scene, rows)
    got = st["entries"][0]
    print(f"{tag}: model {int(want.sum())} tiles, bins {int(got.sum())} entries, margin {margin:.2e}")
    assert int(st["wide"].sum()) == 0
    assert np.array_equal(got, want.astype(got.dtype)), (tag, got, want.astype(int))
    _assert_binned_equals_exact(tag, scene, rows)
    return want


# ---- a pair word across a row end --------------------------------------------------------------------------------------
# (W, disc whose run ends at the row's last tile, disc whose run starts at column 0 of the next row): (column, row, radius)
# in pixels.  W = 48: tiles 2 (row 0, last column) and 3 (row 1, column 0) share a word; W = 16: every word is two rows.
ROW_ENDS = {48: ((30.3, 7.4, 6.0), (7.6, 24.3, 5.0)), 16: ((7.7, 7.4, 5.0), (8.3, 24.3, 5.0))}


@pytest.mark.gpu
@pytest.mark.parametrize("W", sorted(ROW_ENDS))
def test_pair_across_a_row_end(W):
    cam = _camera(W, 48, EYE, AT)
    basis = pixel_basis(cam)[:4]
    a, b = (facing(basis, *d) for d in ROW_ENDS[W])
    last = (W + 15) // 16 - 1
    want_a = _one_disc_case(f"W {W} row end", cam, a)
    want_b = _one_disc_case(f"W {W} next row's start", cam, b)
    # the cases are what they claim to be: a ends row 0 at its last tile and stays out of row 1, b is tile (1, 0) alone
    assert want_a[0, last] and not want_a[1:].any() and (last == 0 or want_a[0, last - 1])
    assert want_b[1, 0] and int(want_b.sum()) == 1
    assert ((0 * (last + 1) + last) ^ 1) == 1 * (last + 1) + 0, "the two tiles share a pair word"
    both = scene_of_discs(cam, [a, b])
    st = _bins(both)
    got = st["entries"][0]
    assert np.array_equal(got, (want_a.astype(got.dtype) + want_b.astype(got.dtype))), got      # nobody gained an entry
    assert int(st["wide"].sum()) == 0
    _assert_binned_equals_exact(f"W {W} both", both, None)


# ---- runs that start on either half of a word ---------------------------------------------------------------------------
# 96 x 80: 6 x 5 tiles, so a tile's parity is its column's.  A disc facing the camera on tile row 2: radius 5 stays in one
# tile, radius 6 on a tile boundary takes two, radius 10 around a tile's centre three (and one tile above and below).
def _run_disc(basis, start, length):
    c = {1: 16.0 * start + 7.6, 2: 16.0 * start + 15.4, 3: 16.0 * start + 23.6}[length]
    return facing(basis, c, 39.4, {1: 5.0, 2: 6.0, 3: 10.0}[length])


@pytest.mark.gpu
@pytest.mark.parametrize("length", [1, 2, 3])
@pytest.mark.parametrize("start", [2, 1])
def test_run_shapes(start, length):
    cam = _camera(96, 80, EYE, AT)
    want = _one_disc_case(f"run of {length} from tile column {start}", cam, _run_disc(pixel_basis(cam)[:4], start, length))
    cols = np.nonzero(want[2])[0]
    assert (cols.min(), cols.max()) == (start, start + length - 1), cols


# ---- an odd tile count ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,rows", [(48, (5, 37)), (16, None)])
def test_last_tile_and_the_word_beyond(H, rows):
    """48 x 16 has three tiles: the last one is the low half of a word whose high half is padding.  The slab (5, 37) of
    48 x 48 bins six tiles in a workspace laid out for nine."""
    import torch
    from surf_renderer_amd import _lib, renderer
    W = 48
    cam = _camera(W, H, EYE, AT)
    basis = pixel_basis(cam)[:4]
    r0, r1 = rows or (0, H)
    discs = [facing(basis, W - 8.4, r1 - 7.6, 5.0), facing(basis, 24.3, r1 - 8.3, 11.0), facing(basis, 8.6, r0 + 7.7, 6.5)]
    want = sum(expected(cam, d, rows)[0].astype(np.int64) for d in discs)
    assert all(expected(cam, d, rows)[1] >= 1e-3 for d in discs)
    scene = scene_of_discs(cam, discs)
    buf = renderer.flatten_scene(scene, device="cuda:0")
    cs = renderer.camera_struct(scene["camera"])
    ws = buf.new_workspace(W, H)
    out = renderer.render_buffers(buf, cs, rows=rows, mode="binned", workspace=ws, stages=_lib.STAGE_BIN)
    words, (tx, ty, cap) = _counter_words(buf, cs, rows, ws)
    ntiles = tx * ty
    print(f"{W} x {H} rows {rows}: {ntiles} tiles, padded to {words.shape[1]}, counters {words[0].tolist()}")
    assert np.array_equal(words[0, :ntiles].reshape(ty, tx), want), (words[0], want)
    assert words[0, ntiles - 1] >= 1, "the last tile is filled"
    assert words.shape[1] > ntiles and not words[0, ntiles:].any(), "the counters beyond the last tile stay zero"
    del out
    # ... and after the frame's render stage every counter is zero again
    renderer.render_buffers(buf, cs, rows=rows, mode="binned", workspace=ws, stages=_lib.STAGE_RENDER)
    words, _ = _counter_words(buf, cs, rows, ws)
    assert not words.any()
    torch.cuda.synchronize()
    _assert_binned_equals_exact(f"{W} x {H} rows {rows}", scene, rows)


# ---- one half of a word past the bin's capacity ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("full_tile_column", [4, 5])
def test_full_bin_beside_its_partner(full_tile_column):
    """160 x 144 (90 tiles, padded to 92) and 100 discs leave a bin 6400 / 92 = 69 slots (a smaller frame or fewer discs
    leave it more than there are discs).  95 identical discs inside one tile and 5 identical ones across the border to
    its partner: the full tile keeps `cap` entries and its surplus goes to the frame-wide list once
    per primitive; the partner holds its five -- in the same claims, since the five take both halves of the word."""
    cam = _camera(160, 144, EYE, AT)
    basis = pixel_basis(cam)[:4]
    full, partner = full_tile_column, full_tile_column ^ 1
    row = 4 * 16 + 7.6
    inside = facing(basis, 16.0 * full + 7.4, row, 3.0)
    across = facing(basis, 16.0 * max(full, partner) - 0.4 + (1.5 if full > partner else -1.5), row, 4.0)
    w_in, m_in = expected(cam, inside)
    w_ac, m_ac = expected(cam, across)
    assert min(m_in, m_ac) >= 1e-3
    assert int(w_in.sum()) == 1 and w_in[4, full] and int(w_ac.sum()) == 2 and w_ac[4, full] and w_ac[4, partner]
    scene = scene_of_discs(cam, [inside] * 95 + [across] * 5)
    st = _bins(scene)
    cap, got = st["bin_capacity"], st["entries"][0]
    print(f"full tile column {full}: capacity {cap}, entries {int(got[4, full])} and {int(got[4, partner])}, frame-wide {st['wide']}")
    assert 5 < cap < 100, "the case needs the 100 claims to overflow the bin and the 5 not to"
    assert got[4, full] == cap and got[4, partner] == 5 and int(got.sum()) == cap + 5
    assert int(st["wide"].sum()) == 100 - cap
    _assert_binned_equals_exact(f"full tile column {full}", scene, None)


# ---- two batches ----------------------------------------------------------------------------------------------------------
def _two_batches(cam):
    basis = pixel_basis(cam)[:4]
    W, H = cam["viewport"][2:]
    discs = [facing(basis, 30.3, 7.4, 6.0), facing(basis, 7.6, 24.3, 5.0), facing(basis, W - 8.4, H - 7.6, 5.0)]
    scene = scene_of_discs(cam, discs)

    def at(c, r, depth):
        eye, D0, Dc, Dr = basis
        return eye + depth * (D0 + c * Dc + r * Dr)
    # triangles (pixel corners, depth): across a row end into the next row's first tile, a sliver along the last tile
    # row, one over the frame's middle
    tris = [((34.0, 3.0), (46.5, 12.0), (3.0, 29.5), 2.5), ((2.0, 40.5), (46.0, 44.0), (20.0, 46.5), 2.8),
            ((10.0, 10.0), (40.0, 18.0), (22.0, 40.0), 3.4)]
    v = np.array([[at(*a, d), at(*b, d), at(*c, d)] for a, b, c, d in tris])
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    scene["objects"]["triangle"] = {"face": f32(np.concatenate([v, np.ones((len(tris), 3, 1))], 2)),
                                    "normal": f32(np.concatenate([fn, np.zeros((len(tris), 1))], 1)),
                                    "material_idx": np.array([1, 2, 0])}
    return scene


@pytest.mark.gpu
def test_two_batches():
    """48 x 48: nine tiles padded to twelve, so the triangles' counters start 12 words after the discs' (a multiple of four:
    8-byte aligned, asserted in _counter_words).  Each batch's bins are what the batch gets alone, every tile with a pixel
    the exact mode gives to a triangle is in that triangle's batch's bins, and the frame equals the exact mode."""
    import torch
    from surf_renderer_amd import _lib, render, renderer
    cam = _camera(48, 48, EYE, AT)
    scene = _two_batches(cam)
    buf = renderer.flatten_scene(scene, device="cuda:0")
    cs = renderer.camera_struct(scene["camera"])
    ws = buf.new_workspace(48, 48)
    renderer.render_buffers(buf, cs, mode="binned", workspace=ws, stages=_lib.STAGE_BIN)
    words, (tx, ty, cap) = _counter_words(buf, cs, None, ws)
    assert words.shape == (2, 12) and not words[:, 9:].any()
    kinds = list(scene["objects"])
    both = _bins(scene)["entries"]
    assert np.array_equal(both.reshape(2, 9), words[:, :9])
    for s, kind in enumerate(kinds):
        alone = dict(scene, objects={kind: scene["objects"][kind]})
        assert np.array_equal(_bins(alone)["entries"][0], both[s]), kind
    tri = both[kinds.index("triangle")]
    assert tri.max() >= 2 and (tri > 0).sum() >= 7 and tri[0, 2] and tri[1, 0]        # the first triangle crosses the row end
    ref = render(dict(scene, objects={"triangle": scene["objects"]["triangle"]}), device="cuda:0", mode="exact")
    torch.cuda.synchronize()
    hit = (ref["nearest"].cpu().numpy() >= 0).reshape(3, 16, 3, 16).any(axis=(1, 3))
    assert hit.sum() >= 7 and not (hit & (tri == 0)).any()
    _assert_binned_equals_exact("two batches", scene, None)


# ---- a light view -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_light_views_pair_their_claims():
    """The light views bin with bin_pad = 1 through k_prep_views: small and elongated discs over a receiver, the binned
    shadow pass against all pairs."""
    import torch
    rng = np.random.RandomState(9)
    lights = [(4.0, -4.8, 9.6), (-6.4, 1.6, 8.0)]
    n = 160
    pos = rng.uniform(-0.9, 0.9, (n, 3)) + np.array([0.0, 0.0, 1.0])
    nrm = np.empty((n, 3))
    for i in range(n):
        v = _unit(pos[i] - np.array(lights[i % 2]))
        w = _unit(np.cross(v, rng.normal(size=3)))
        a = np.arcsin(1.0 / np.exp(rng.uniform(np.log(1.0), np.log(100.0))))
        nrm[i] = np.sin(a) * v + np.cos(a) * w
    rad = np.exp(rng.uniform(np.log(0.03), np.log(0.4), n))
    disk = {"pos": f32(np.concatenate([np.concatenate([pos, [[0.0, 0.0, 0.0]]]), np.ones((n + 1, 1))], 1)),
            "normal": f32(np.concatenate([np.concatenate([nrm, [[0.0, 0.0, 1.0]]]), np.zeros((n + 1, 1))], 1)),
            "radius": f32(np.concatenate([rad, [3.0]])), "material_idx": rng.randint(0, 3, n + 1)}
    scene = _base(65, 49, (0.5, -4.0, 3.0), (0.0, 0.0, 0.5), {"disk": disk}, lights)
    assert all(v is not None for v in light_views(scene)), "every light must have a view of its own"
    (img_b, vis_b, depth), (img_a, vis_a, _) = shadow_both_ways(scene)
    hit = torch.isfinite(depth) & (depth < 1e30)
    blocked = int(((vis_a & 3) != 3)[hit].sum())
    print(f"{int(hit.sum())} hit pixels, {blocked} with a blocked light")
    assert blocked > 100
    assert torch.equal(vis_b, vis_a), int((vis_b != vis_a).sum())
    assert torch.equal(img_b, img_a)


# ---- the counters are left clean ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_counters_clean_after_a_frame():
    """After a whole frame every counter word is zero (the render kernel zeroes its tile's, as 32-bit words), and a second
    frame's binning on the same workspace -- which then skips the clearing launch -- gives the bins of a fresh one."""
    from surf_renderer_amd import _lib, renderer
    cam = _camera(48, 48, EYE, AT)
    scene = _two_batches(cam)
    buf = renderer.flatten_scene(scene, device="cuda:0")
    cs = renderer.camera_struct(scene["camera"])
    ws = buf.new_workspace(48, 48)
    first = renderer.render_buffers(buf, cs, mode="binned", workspace=ws)
    words, _ = _counter_words(buf, cs, None, ws)
    assert not words.any(), words
    renderer.render_buffers(buf, cs, mode="binned", workspace=ws, stages=_lib.STAGE_BIN)
    again, _ = _counter_words(buf, cs, None, ws)
    assert np.array_equal(again[:, :9].reshape(2, 3, 3), _bins(scene)["entries"])
    renderer.render_buffers(buf, cs, mode="binned", workspace=ws, stages=_lib.STAGE_RENDER)
    second = renderer.render_buffers(buf, cs, mode="binned", workspace=ws)
    import torch
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ---- the model's count of pair words (no GPU) -----------------------------------------------------------------------------
def test_pair_word_count_of_hand_made_runs():
    # tiles_x = 6 (even): a word never leaves its row.  Runs from an even column: 1, 2, 3 tiles -> 1, 1, 2 words
    assert [P.pair_words(6, [(2, range(2, 2 + n))]) for n in (1, 2, 3)] == [(1, 1), (2, 1), (3, 2)]
    # ... from an odd column: the first tile is the high half of its word -> 1, 2, 2 words
    assert [P.pair_words(6, [(2, range(1, 1 + n))]) for n in (1, 2, 3)] == [(1, 1), (2, 2), (3, 2)]
    # tiles_x = 3: tile 2 (row 0, last column) and tile 3 (row 1, column 0) share a word, which is claimed once per row
    assert P.pair_words(3, [(0, [1, 2]), (1, [0])]) == (3, 3)
    assert P.pair_words(3, [(0, [2])]) == (1, 1) and P.pair_words(3, [(1, [0, 1, 2])]) == (3, 2)
    # tiles_x = 1: every word is two rows, nothing pairs
    assert P.pair_words(1, [(0, [0]), (1, [0]), (2, [0])]) == (3, 3)
    # a tile-loop mask with a gap: columns 0, 1 and 3 of an even row start -> words {0, 1}
    assert P.pair_words(4, [(1, [0, 1, 3])]) == (3, 2)
    # the vectorised form on the same runs (rows 0 and 1 of a 3-column frame), and the round count
    claims, words = P.pair_words_of_runs(3, np.array([[1, 0], [2, 0], [1, 1]]), np.array([[2, 0], [2, 2], [0, 0]]))
    assert claims.tolist() == [3, 4, 0] and words.tolist() == [3, 3, 0]
    assert P.rounds([5] * 64 + [7] + [0] * 63, 4) == 2.0 and P.rounds([5] * 64 + [7] + [0] * 63, 6) == 1.5
