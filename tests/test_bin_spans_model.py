"""The row-span rule by which bin_place picks a conic's tiles (ConicSpans, srh_reject.h) against the per-tile rule it
replaces (RectTest::reaches), both restated in numpy float64 (tests/bin_spans_model.py).  No GPU.

120 000 random stored forms: major half extent 0.3-300 px (log-uniform), axis ratio 1-512 (log-uniform; the minor half
extent goes down to 0.3 / 512 px), every orientation with 0 / 45 / 90 / 135 degrees forced on one form in eight, the
coefficients and the centre rounded to fp32 as the record stores them; centres inside the frame, exactly on and half a
pixel off its edges, and up to two boxes outside it; a 100 x 70 image and its row slab (5, 61), bin_pad 0 and 1.

For every form and every tile:
    per-tile minimum <= 1          implies  the tile is in the span set     (no true candidate is lost)
    the tile is in the span set    implies  per-tile minimum <= 1.00001     (the widening costs next to nothing)
The second bound is not fitted: the span rule's threshold is 1.000001, and its outward margin 2^-30 (1 + dc_max) px raises
q by at most 2^-29 (sqrt(A11) + sqrt(A11 A22 / det)) (srh_reject.h), which is 2^-29 (1707 + 257) = 3.7e-6 for the thinnest
and most elongated form drawn here: 4.7e-6 together.

The `behind` shortcut is held to EQUALITY with the per-tile expression on the same runs, with mixed rows present."""
import functools

import numpy as np
import pytest

import bin_spans_model as M

N_PER_CONFIG = 30000
CONFIGS = [(100, (0, 70), 0.0), (100, (0, 70), 1.0), (100, (5, 61), 0.0), (100, (5, 61), 1.0)]


def random_forms(rng, n, W, rows):
    major = np.exp(rng.uniform(np.log(0.3), np.log(300.0), n))
    ratio = np.exp(rng.uniform(0.0, np.log(512.0), n))
    ratio[rng.randint(0, 16, n) == 0] = 512.0
    ratio[rng.randint(0, 16, n) == 0] = 1.0
    minor = major / ratio
    th = rng.uniform(0.0, np.pi, n)
    forced = rng.randint(0, 8, n) == 0
    th[forced] = np.deg2rad(rng.choice([0.0, 45.0, 90.0, 135.0], int(forced.sum())))
    c, s = np.cos(th), np.sin(th)
    l1, l2 = 1.0 / major ** 2, 1.0 / minor ** 2
    A11 = M.f32(c * c * l1 + s * s * l2).astype(np.float64)
    B = M.f32(2.0 * c * s * (l1 - l2)).astype(np.float64)            # rec[3] = 2 A12
    A22 = M.f32(s * s * l1 + c * c * l2).astype(np.float64)
    form = {"A11": A11, "A12": 0.5 * B, "A22": A22, "x0": np.zeros(n), "y0": np.zeros(n)}
    hc, hr = M.extents(form)
    # centres: 0 inside, 1 on / half a pixel off an edge, 2 outside by up to two boxes
    kind = rng.randint(0, 3, n)
    x = rng.uniform(0.0, W - 1.0, n)
    y = rng.uniform(rows[0], rows[1] - 1.0, n)
    edge = rng.randint(0, 4, n)
    off = rng.choice([-0.5, 0.0, 0.5], n)
    on = kind == 1
    x = np.where(on & (edge == 0), 0.0 + off, np.where(on & (edge == 1), W - 1.0 + off, x))
    y = np.where(on & (edge == 2), rows[0] + off, np.where(on & (edge == 3), rows[1] - 1.0 + off, y))
    out = kind == 2
    far = rng.uniform(0.0, 2.0, n)
    x = np.where(out & (edge == 0), -far * 2.0 * hc, np.where(out & (edge == 1), W - 1.0 + far * 2.0 * hc, x))
    y = np.where(out & (edge == 2), rows[0] - far * 2.0 * hr, np.where(out & (edge == 3), rows[1] - 1.0 + far * 2.0 * hr, y))
    form["x0"], form["y0"] = M.f32(x).astype(np.float64), M.f32(y).astype(np.float64)
    return form, kind, ratio


def random_estimates(rng, n, W, rows):
    """Depth-estimate fields whose horizon den = hi crosses the frame: mixed rows by construction."""
    u1, u2 = rng.normal(size=n), rng.normal(size=n)
    u1[rng.randint(0, 10, n) == 0] = 0.0
    u2[rng.randint(0, 10, n) == 0] = 0.0
    cx, cy = rng.uniform(-20.0, W + 20.0, n), rng.uniform(rows[0] - 20.0, rows[1] + 20.0, n)
    hi = -np.abs(rng.normal(size=n)) * 1e-3
    u0 = hi - (u1 * cx + u2 * cy)
    return {k: M.f32(v).astype(np.float64) for k, v in (("u0", u0), ("u1", u1), ("u2", u2), ("hi", hi))}


@functools.lru_cache(maxsize=None)
def _config(i):
    W, rows, pad = CONFIGS[i]
    rng = np.random.RandomState(7100 + i)
    form, kind, ratio = random_forms(rng, N_PER_CONFIG, W, rows)
    est = random_estimates(rng, N_PER_CONFIG, W, rows)
    grid = M.Grid(W, rows, pad)
    box = M.tile_box(form, grid)
    return form, kind, ratio, est, grid, box


def test_the_generator_covers_what_it_claims():
    assert N_PER_CONFIG * len(CONFIGS) >= 100000
    for i in range(len(CONFIGS)):
        form, kind, ratio, est, grid, box = _config(i)
        placed = box[4]
        assert ratio.min() == 1.0 and ratio.max() == 512.0
        for k in range(3):
            assert (placed & (kind == k)).sum() > 1000, (i, k)
        tiles = (box[1] - box[0] + 1) * (box[3] - box[2] + 1)
        assert (placed & (tiles >= 20)).sum() > 1000 and (placed & (tiles == 1)).sum() > 100


@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_span_set_against_the_per_tile_minimum(i):
    form, kind, ratio, est, grid, box = _config(i)
    qmin = M.per_tile_min(form, grid)
    reached, usable = M.span_set(form, grid, box)
    fallback = int((~usable).sum())
    assert fallback == 0, f"{fallback} forms would take the kernel's per-tile fallback"
    inside = M.in_box(box, grid)
    lost = (qmin <= 1.0) & inside & ~reached
    extra = reached & ~(qmin <= 1.00001)
    old = (qmin <= M.LAMBDA) & inside
    print(f"config {CONFIGS[i]}: {int(box[4].sum())} placed forms, {int(inside.sum())} box tiles, {int(old.sum())} reached per tile, "
          f"{int(reached.sum())} by spans, {int((old != reached).sum())} differ; largest q_min of a span tile "
          f"{qmin[reached].max():.9f}")
    assert not lost.any(), f"{int(lost.sum())} tiles with a candidate are not in the span set"
    assert not extra.any(), f"{int(extra.sum())} span tiles have q_min up to {qmin[extra].max()}"
    # a box corner of a slanted ellipse is really dropped, by either rule
    assert (inside & ~reached).sum() > 0.05 * inside.sum()


@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_behind_shortcut_equals_the_per_tile_expression(i):
    form, kind, ratio, est, grid, box = _config(i)
    ta, tb, usable = M.span_runs(form, grid, box)
    placed = box[4][:, None] & (np.arange(grid.tiles_y)[None, :] >= box[2][:, None]) & (np.arange(grid.tiles_y)[None, :] <= box[3][:, None])
    ta, tb = np.where(placed, ta, 1), np.where(placed, tb, 0)
    want = M.runs_to_set(ta, tb, grid) & ~M.behind_tiles(est, grid)
    ta2, tb2, mixed, tested = M.behind_runs(est, grid, ta, tb, box)
    got = M.runs_to_set(ta2, tb2, grid)
    rows_all = int((ta <= tb).sum())
    rows_dropped = int(((ta <= tb) & (ta2 > tb2)).sum())
    print(f"config {CONFIGS[i]}: {rows_all} runs, {rows_dropped} dropped whole, {mixed} mixed; {tested} of {int(box[4].sum())} placed "
          f"forms have their box's worst corner behind the eye")
    assert mixed > 500 and rows_dropped > 500 and rows_all - rows_dropped - mixed > 500
    assert 1000 < tested < box[4].sum() - 1000
    assert np.array_equal(got, want), f"{int((got != want).sum())} tiles differ"
