"""A numpy model of the association tree of srh_mesh.h's k_mesh_scan -- test infrastructure, used by
tests/test_mesh_scan_cases_cpu.py alone, to show that the ranged inputs of tests/mesh_scan_cases.py catch a scan of
the same tree that forgets the running maximum.  No GPU assertion depends on it: a later scan of another shape need
not mirror it.

Per tile of 1024 faces: a lane adds its 4 consecutive weights serially, the 64 lane totals of a wave are scanned by
Hillis-Steele steps (the earlier lanes' value the left operand), the four wave totals are added left to right, and a
carry runs from tile to tile; a face's prefix is (carry + (wave offset + lane offset)) + its serial sum.  With
`running_max` the value of a face is the largest prefix of the positive-weight faces up to it (0 in front of the first)
and the total is the last value; without it, every face keeps its own prefix."""
import numpy as np

ITEMS, LANES, WAVES = 4, 64, 4
TILE = ITEMS * LANES * WAVES


def prefixes(weight):
    """[F] float64: every face's own prefix sum, formed by the scan's tree"""
    w = np.asarray(weight, np.float64)
    out, carry = np.empty(len(w)), 0.0
    for base in range(0, len(w), TILE):
        x = np.zeros(TILE)
        n = min(TILE, len(w) - base)
        x[:n] = w[base:base + n]
        x = x.reshape(WAVES, LANES, ITEMS)
        s = x.copy()
        for k in range(1, ITEMS):
            s[..., k] = s[..., k - 1] + x[..., k]
        inc = s[..., ITEMS - 1].copy()                                  # [waves, lanes]
        d = 1
        while d < LANES:
            inc[:, d:] = inc[:, :-d] + inc[:, d:]                       # numpy evaluates the right side first
            d *= 2
        exc = np.concatenate([np.zeros((WAVES, 1)), inc[:, :-1]], axis=1)
        tile, woff = 0.0, np.zeros(WAVES)
        for j in range(WAVES):
            woff[j] = tile
            tile = tile + inc[j, LANES - 1]
        before = carry + (woff[:, None] + exc)
        out[base:base + n] = (before[..., None] + s).reshape(-1)[:n]
        carry = carry + tile
    return out


def scan(weight, running_max=True):
    """(values [F], total): what the scan leaves in front of its division"""
    w = np.asarray(weight, np.float64)
    p = prefixes(w)
    if not running_max:
        return p, p[-1]
    m = np.maximum.accumulate(np.where(w > 0, p, 0.0))                  # the maximum is exact: any order gives this
    return m, m[-1]


def cdf(weight, running_max=True):
    values, total = scan(weight, running_max)
    return values / total
