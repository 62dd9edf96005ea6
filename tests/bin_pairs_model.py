"""numpy model of bin_place's pass 2 (srh_binned.h): how many returning atomics a primitive's tile set costs when one
64-bit add claims the aligned pair of bin counters (t & ~1, t | 1) at once (importable without a GPU).

Tiles are numbered row-major over the frame, t = ty * tiles_x + tx.  bin_place walks the primitive's tile mask in that
order; a tile's partner rides in the same claim only where it is the neighbouring bit of the SAME box row, so per box row
the claims are the distinct words t >> 1 among the row's tiles.  With an odd tiles_x a word can straddle two tile rows:
it is then claimed once per row, each time with +1 in one half only."""
import numpy as np


def pair_words(tiles_x, rows):
    """`rows`: iterable of (ty, tile columns of that box row).  Returns (tile claims, pair words)."""
    claims = words = 0
    for ty, cols in rows:
        cols = sorted(set(int(c) for c in cols))
        claims += len(cols)
        words += len({(ty * tiles_x + tx) >> 1 for tx in cols})
    return claims, words


def pair_words_of_runs(tiles_x, ta, tb):
    """Vectorised over (forms, tile rows) runs [ta, tb] of tile columns (ta > tb: none): (tile claims, pair words) per form.
    A run [ta, tb] in row ty covers the words (ty tiles_x + ta) >> 1 .. (ty tiles_x + tb) >> 1."""
    ta, tb = np.asarray(ta, dtype=np.int64), np.asarray(tb, dtype=np.int64)
    some = ta <= tb
    base = np.arange(ta.shape[1], dtype=np.int64)[None, :] * tiles_x
    claims = np.where(some, tb - ta + 1, 0)
    words = np.where(some, ((base + tb) >> 1) - ((base + ta) >> 1) + 1, 0)
    return claims.sum(axis=1), words.sum(axis=1)


def rounds(per_lane, in_flight, wave=64):
    """Mean over the waves of `wave` consecutive primitives of the round trips the busiest lane needs."""
    per_lane = np.asarray(per_lane, dtype=np.int64)
    pad = (-len(per_lane)) % wave
    worst = np.concatenate([per_lane, np.zeros(pad, dtype=np.int64)]).reshape(-1, wave).max(axis=1)
    return float(np.mean(-(-worst // in_flight)))
