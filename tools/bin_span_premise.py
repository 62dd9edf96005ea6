#!/usr/bin/env python3
"""How many iterations pass 1 of bin_place runs at config 5 (bench.py's workload), from a numpy restatement of the disc
records and their tile boxes (tests/bin_spans_model.py).  No GPU.

Per wave of 64 consecutive discs: the largest box in tiles (iterations of the parent's per-tile loop), the
largest box in tile rows (iterations of the row loop), and the discs whose box has its worst corner behind the eye (the
only ones whose rows take the `behind` test).  Discs without an ellipse record of their own (the sphere stand-in) are
not modelled and count as "no box".  profiles/bin_spans_pmc.json quotes the output.

--claims: pass 2 instead -- the returning atomics per disc with one claim per tile and with one per aligned pair of
tiles, and the round trips per wave (see claims(); profiles/prep_claims_premise.json)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import bin_spans_model as M                                   # noqa: E402
from surf_renderer_amd import synthetic                       # noqa: E402
from test_hip_prep_bounds import pixel_basis                  # noqa: E402

WAVE = 64


def box_of(basis, grid, W, H, disc, i):
    """(tiles, tile rows, tile rows if the box's worst corner is behind the eye) of disc i; None: no record of its own"""
    try:
        form, est, (hc, hr) = M.disc_records(basis, W, H, disc["pos"][i:i + 1], disc["normal"][i:i + 1], disc["radius"][i:i + 1])
    except AssertionError:
        return None
    tx0, tx1, ty0, ty1, placed = (v[0] for v in M.tile_box(form, grid, hc, hr))
    if not placed:
        return 0, 0, 0
    u0, u1, u2, hi = (est[k][0] for k in ("u0", "u1", "u2", "hi"))
    wx, wy = (tx0 if u1 >= 0 else tx1), (ty0 if u2 >= 0 else ty1)
    den = u0 + max(u1 * grid.pc0[wx], u1 * grid.pc1[wx]) + max(u2 * grid.pr0[wy], u2 * grid.pr1[wy])
    rows = ty1 - ty0 + 1
    return (tx1 - tx0 + 1) * rows, rows, rows if den <= hi else 0


def per_wave_max(values):
    pad = (-len(values)) % WAVE
    return np.concatenate([values, np.zeros(pad, dtype=values.dtype)]).reshape(-1, WAVE).max(axis=1)


def main():
    W = H = 2048
    scene = synthetic.disk_cloud_scene(100000, W, H)
    basis = pixel_basis(scene["camera"])[:4]
    disc = scene["objects"]["disk"]
    grid = M.Grid(W, (0, H), 0.0)
    n = len(disc["radius"])
    boxes = [box_of(basis, grid, W, H, disc, i) for i in range(n)]
    no_record = sum(b is None for b in boxes)
    tiles, rows, hidden_rows = (np.array([b[k] if b else 0 for b in boxes], dtype=np.int64) for k in range(3))
    print(json.dumps({
        "discs": n,
        "without_a_record_of_their_own": no_record,
        "placed": int((tiles > 0).sum()),
        "box_tiles_total": int(tiles.sum()),
        "waves": len(per_wave_max(tiles)),
        "sum_over_waves_of_max_tiles": int(per_wave_max(tiles).sum()),
        "mean_max_tiles_per_wave": float(per_wave_max(tiles).mean()),
        "sum_over_waves_of_max_rows": int(per_wave_max(rows).sum()),
        "mean_max_rows_per_wave": float(per_wave_max(rows).mean()),
        "discs_whose_box_corner_is_behind_the_eye": int((hidden_rows > 0).sum()),
        "sum_over_waves_of_max_rows_of_such_discs": int(per_wave_max(hidden_rows).sum()),
    }, indent=1))


def claims():
    """Pass 2 at config 5, all discs: returning atomics per disc with one claim per tile and with one per aligned pair
    of tiles (tests/bin_pairs_model.py), the per-wave maxima of both (the busiest lane sets a wave's pace), and the mean
    round trips per wave with 4, 6 and 8 claims in flight.  profiles/prep_claims_premise.json is this output."""
    import bin_pairs_model as P
    W = H = 2048
    scene = synthetic.disk_cloud_scene(100000, W, H)
    cam = scene["camera"]
    basis = pixel_basis(cam)[:4]
    disc = scene["objects"]["disk"]
    grid = M.Grid(W, (0, H), 0.0)
    n = len(disc["radius"])
    tiles, words = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    no_record = 0
    for i in range(n):
        try:
            form, est, (hc, hr) = M.disc_records(basis, W, H, disc["pos"][i:i + 1], disc["normal"][i:i + 1], disc["radius"][i:i + 1])
        except AssertionError:
            no_record += 1
            continue
        box = M.tile_box(form, grid, hc, hr)
        if not box[4][0]:
            continue
        # only the box's tile rows: a frame of 128 x 128 tiles per disc is what makes the vectorised form slow
        ty0, ty1 = int(box[2][0]), int(box[3][0])
        sub = M.Grid(W, (ty0 * M.TILE, min((ty1 + 1) * M.TILE, H)), 0.0)
        sbox = (box[0], box[1], box[2] - ty0, box[3] - ty0, box[4])
        ta, tb, usable = M.span_runs(form, sub, sbox)
        if not usable[0]:
            no_record += 1
            continue
        if cam.get("near", 0.0) > 0.0:
            ta, tb, _, _ = M.behind_runs(est, sub, ta, tb, sbox)
        # tile ids of the whole frame: row ty0 + k of the sub-grid
        c, w = P.pair_words(grid.tiles_x, [(ty0 + k, range(int(a), int(b) + 1)) for k, (a, b) in enumerate(zip(ta[0], tb[0]))])
        tiles[i], words[i] = c, w
    wt, ww = per_wave_max(tiles), per_wave_max(words)
    print(json.dumps({
        "discs": n,
        "not_modelled": no_record,
        "tile_claims_total": int(tiles.sum()),
        "pair_words_total": int(words.sum()),
        "pair_words_over_tile_claims": float(words.sum() / tiles.sum()),
        "mean_per_disc": {"tile_claims": float(tiles.mean()), "pair_words": float(words.mean())},
        "max_per_disc": {"tile_claims": int(tiles.max()), "pair_words": int(words.max())},
        "waves": len(wt),
        "mean_per_wave_max": {"tile_claims": float(wt.mean()), "pair_words": float(ww.mean())},
        "share_of_waves_whose_max_is_at_most": {
            str(c): {"tile_claims": float((wt <= c).mean()), "pair_words": float((ww <= c).mean())} for c in (4, 6, 8)},
        "mean_rounds_per_wave_in_flight": {
            str(c): {"tile_claims": P.rounds(tiles, c, WAVE), "pair_words": P.rounds(words, c, WAVE)} for c in (4, 6, 8)},
    }, indent=1))


if __name__ == "__main__":
    claims() if "--claims" in sys.argv[1:] else main()
