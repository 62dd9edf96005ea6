"""numpy float64 model of the two ways bin_place (srh_binned.h) picks the tiles of a stored ellipse record (importable
without a GPU).

`per_tile_min`   the per-tile rule (RectTest::reaches): the exact minimum of the stored form
                 q(dc, dr) = A11 dc^2 + 2 A12 dc dr + A22 dr^2 over a tile's pixel rectangle, by the clamped vertices of
                 its four edges; the tile is reached iff the minimum is <= 1.000001.
`span_set`       the row-span rule (ConicSpans): per tile row the column interval of the region q <= 1.000001 over the
                 row's band, widened by 2^-30 (1 + dc_max) pixels, turned into a run of tile columns.
`behind_tiles`   the `behind` expression per tile, and `behind_runs` its per-row shortcut (decided at the run's ends).
`disc_records`   the record k_prep stores for a disc (disk_reject_record, conic_record, plane_estimate_record) in IEEE
                 arithmetic: the stored fp32 values agree with the kernel's up to its 2^-44 Newton forms, which is why
                 the callers keep their inputs 1e-3 away from every threshold.

A `form` is a dict of float64 arrays x0, y0, A11, A12, A22 (the VALUES of the fp32 record; A12 = rec[3] / 2)."""
import numpy as np

TILE = 16
LAMBDA = 1.000001
M30 = 2.0 ** -30
MAX_TILES = 64


class Grid:
    """The tiles of a W-pixel-wide frame's rows [row0, row1) and their padded pixel rectangles, as bin_place forms them."""

    def __init__(self, W, rows, pad):
        self.W, (self.row0, self.row1), self.pad = W, rows, float(pad)
        self.tiles_x, self.tiles_y = (W + TILE - 1) // TILE, (self.row1 - self.row0 + TILE - 1) // TILE
        tx, ty = np.arange(self.tiles_x), np.arange(self.tiles_y)
        self.pc0 = tx * TILE - self.pad
        self.pc1 = np.minimum(tx * TILE + TILE - 1, float(W - 1)) + self.pad
        self.pr0 = self.row0 + ty * TILE - self.pad
        self.pr1 = np.minimum(self.row0 + ty * TILE + TILE - 1, float(self.row1 - 1)) + self.pad


def extents(form):
    """Half extents of the stored form's box (a hair above the exact ones, like conic_record's)."""
    det = form["A11"] * form["A22"] - form["A12"] ** 2
    return np.sqrt(form["A22"] / det) * (1.0 + 2.0 ** -20), np.sqrt(form["A11"] / det) * (1.0 + 2.0 ** -20)


def tile_box(form, grid, hc=None, hr=None):
    """bin_primitive's inclusive tile box per form: (tx0, tx1, ty0, ty1, placed); placed = False where the box is empty
    or holds more than 64 tiles (the frame-wide list: bin_place never sees those)."""
    if hc is None:
        hc, hr = extents(form)
    c_lo, c_hi = np.maximum(np.floor(form["x0"] - hc - 1.0), 0.0), np.minimum(np.ceil(form["x0"] + hc + 1.0), grid.W - 1.0)
    r_lo = np.maximum(np.floor(form["y0"] - hr - 1.0), float(grid.row0))
    r_hi = np.minimum(np.ceil(form["y0"] + hr + 1.0), grid.row1 - 1.0)
    some = (c_lo <= c_hi) & (r_lo <= r_hi)
    z = lambda v: np.where(some, v, 0.0).astype(np.int64)          # noqa: E731
    tx0, tx1 = z(c_lo) // TILE, z(c_hi) // TILE
    ty0, ty1 = (z(r_lo) - grid.row0) // TILE, (z(r_hi) - grid.row0) // TILE
    placed = some & ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) <= MAX_TILES)
    return tx0, tx1, ty0, ty1, placed


def in_box(box, grid):
    tx0, tx1, ty0, ty1, placed = box
    tx, ty = np.arange(grid.tiles_x)[None, None, :], np.arange(grid.tiles_y)[None, :, None]
    e = lambda v: v[:, None, None]                                 # noqa: E731
    return e(placed) & (tx >= e(tx0)) & (tx <= e(tx1)) & (ty >= e(ty0)) & (ty <= e(ty1))


def per_tile_min(form, grid):
    """(forms, tile rows, tile columns): the exact minimum of q over each tile's rectangle."""
    e = lambda v: v[:, None, None]                                 # noqa: E731
    x0, y0, A11, A12, A22 = (e(form[k]) for k in ("x0", "y0", "A11", "A12", "A22"))
    c0, c1 = grid.pc0[None, None, :], grid.pc1[None, None, :]
    r0, r1 = grid.pr0[None, :, None], grid.pr1[None, :, None]
    inside = (x0 >= c0) & (x0 <= c1) & (y0 >= r0) & (y0 <= r1)
    qmin = np.full(np.broadcast(x0, c0, r0).shape, np.inf)
    for edge in (0, 1):
        dc = (c1 if edge else c0) - x0
        dr = np.minimum(np.maximum(-A12 * dc / A22, r0 - y0), r1 - y0)
        qmin = np.minimum(qmin, A11 * dc * dc + 2.0 * A12 * dc * dr + A22 * dr * dr)
        dr2 = (r1 if edge else r0) - y0
        dc2 = np.minimum(np.maximum(-A12 * dr2 / A11, c0 - x0), c1 - x0)
        qmin = np.minimum(qmin, A11 * dc2 * dc2 + 2.0 * A12 * dc2 * dr2 + A22 * dr2 * dr2)
    return np.where(inside, 0.0, qmin)


def span_runs(form, grid, box):
    """ConicSpans and bin_place's row loop: per form and tile row the run [ta, tb] of tile columns (ta > tb: none), and
    `usable` (False: the kernel keeps the per-tile loop for that form)."""
    tx0, tx1 = box[0][:, None], box[1][:, None]
    e = lambda v: v[:, None]                                       # noqa: E731
    x0, y0, A11, A12, A22 = (e(form[k]) for k in ("x0", "y0", "A11", "A12", "A22"))
    with np.errstate(all="ignore"):
        p = A11 * A22
        det = p - A12 * A12
        usable = (A11 > 0) & (A22 > 0) & (det > M30 * p)
        dc_max, ry = np.sqrt(LAMBDA * A22 / det), np.sqrt(LAMBDA * A11 / det)
        usable &= (dc_max < 1e30) & (ry < 1e30)
        m = M30 * (1.0 + dc_max)
        dr_star, dr_max, lam11 = -A12 * dc_max / A22, ry * (1.0 + M30), LAMBDA * A11
        a, b = grid.pr0[None, :] - y0, grid.pr1[None, :] - y0
        some = (a <= dr_max) & (b >= -dr_max)
        dR, dL = np.minimum(np.maximum(dr_star, a), b), np.minimum(np.maximum(-dr_star, a), b)
        sR, sL = np.sqrt(np.maximum(lam11 - det * dR * dR, 0.0)), np.sqrt(np.maximum(lam11 - det * dL * dL, 0.0))
        hi, lo = (-A12 * dR + sR) / A11 + (x0 + m), (-A12 * dL - sL) / A11 + (x0 - m)
        ta = np.minimum(np.maximum(np.ceil((lo - grid.pad - (TILE - 1)) / TILE), tx0), tx1 + 1)
        tb = np.maximum(np.minimum(np.floor((hi + grid.pad) / TILE), tx1), tx0 - 1)
        ta, tb = np.nan_to_num(ta).astype(np.int64), np.nan_to_num(tb).astype(np.int64)
        last = (ta * TILE + TILE - 1 > grid.W - 1) & ~((grid.W - 1.0) + grid.pad >= lo)
    none = ~some | last | ~usable
    return np.where(none, 1, ta), np.where(none, 0, tb), usable[:, 0]


def runs_to_set(ta, tb, grid):
    tx = np.arange(grid.tiles_x)[None, None, :]
    return (tx >= ta[:, :, None]) & (tx <= tb[:, :, None])


def span_set(form, grid, box):
    """(reached (forms, tile rows, tile columns) bool inside the box, usable (forms,))"""
    ta, tb, usable = span_runs(form, grid, box)
    return runs_to_set(ta, tb, grid) & in_box(box, grid), usable


def behind_tiles(est, grid):
    """(forms, tile rows, tile columns) bool: reaches' `behind` expression, u0 + max(u1 c0, u1 c1) + max(u2 r0, u2 r1) <= hi."""
    e = lambda v: v[:, None, None]                                 # noqa: E731
    u0, u1, u2, hi = (e(est[k]) for k in ("u0", "u1", "u2", "hi"))
    c0, c1 = grid.pc0[None, None, :], grid.pc1[None, None, :]
    r0, r1 = grid.pr0[None, :, None], grid.pr1[None, :, None]
    return u0 + np.maximum(u1 * c0, u1 * c1) + np.maximum(u2 * r0, u2 * r1) <= hi


def behind_runs(est, grid, ta, tb, box):
    """bin_place's shortcut on the runs [ta, tb]: a form whose box has its worst corner (smallest value of the
    expression) in front of the eye skips the test; otherwise, per row, the run's best end decides "drop the row", its
    worst end "keep it all", and only rows where the two disagree are walked tile by tile from the worst end.  Returns
    the shortened runs, the number of such mixed rows and the number of forms that took the test at all."""
    ta, tb = ta.copy(), tb.copy()
    e = lambda v: v[:, None]                                       # noqa: E731
    u0, u1, u2, hi = (e(est[k]) for k in ("u0", "u1", "u2", "hi"))
    rterms = np.maximum(u2 * grid.pr0[None, :], u2 * grid.pr1[None, :])

    def behind(tx, rterm):
        c0 = tx * TILE - grid.pad
        c1 = np.minimum(tx * TILE + TILE - 1, grid.W - 1.0) + grid.pad
        return u0 + np.maximum(u1 * c0, u1 * c1) + rterm <= hi
    rising = u1 >= 0.0
    wx = np.where(rising, e(box[0]), e(box[1]))
    wy = np.where(u2 >= 0.0, e(box[2]), e(box[3]))
    hides = behind(wx, np.take_along_axis(rterms, np.clip(wy, 0, grid.tiles_y - 1), axis=1))
    rising = np.broadcast_to(rising, ta.shape)
    live = (ta <= tb) & hides
    drop = live & behind(np.where(rising, tb, ta), rterms)
    ta[drop], tb[drop] = 1, 0
    live &= ~drop
    mixed = None
    while True:
        cut = live & behind(np.where(rising, ta, tb), rterms)
        if mixed is None:
            mixed = int(cut.sum())
        if not cut.any():
            return ta, tb, mixed, int(hides.sum())
        ta[cut & rising] += 1
        tb[cut & ~rising] -= 1


# ---- the record k_prep stores for a disc -----------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, dtype=np.float32)


def disc_records(basis, W, H, pos, normal, radius):
    """(form, estimate, (hc, hr)) of discs as disk_reject_record leaves them for a camera with pixel basis
    (eye, D0, Dc, Dr): every disc must have a trusted, well-conditioned ellipse (asserted)."""
    eye, D0, Dc, Dr = basis
    P = [D0, Dc, Dr]
    keys = ("x0", "y0", "A11", "A12", "A22", "u0", "u1", "u2", "hi", "hc", "hr")
    out = {k: [] for k in keys}
    for p, nv, r in zip(np.asarray(pos, dtype=np.float32).astype(np.float64), np.asarray(normal, dtype=np.float32).astype(np.float64),
                        np.asarray(radius, dtype=np.float32).astype(np.float64)):
        n = nv[:3] / np.sqrt(np.sum(nv * nv))
        p = p[:3]
        k = np.dot(p, n) - np.dot(n, eye)
        oc, r2 = eye - p, r * r
        nu = [np.dot(n, pj) for pj in P]
        u = [oc * nu[j] + k * P[j] for j in range(3)]
        T = np.array([[np.dot(u[a], u[b]) - r2 * nu[a] * nu[b] for b in range(3)] for a in range(3)])
        det = T[1, 1] * T[2, 2] - T[1, 2] ** 2
        assert T[1, 1] > 0 and det > 0
        c0 = -(T[2, 2] * T[0, 1] - T[1, 2] * T[0, 2]) / det
        r0 = -(T[1, 1] * T[0, 2] - T[1, 2] * T[0, 1]) / det
        F0 = T[0, 0] + T[0, 1] * c0 + T[0, 2] * r0
        assert F0 < 0
        A11, A12, A22 = T[1, 1] / -F0, T[1, 2] / -F0, T[2, 2] / -F0
        mean, dev = 0.5 * (A11 + A22), np.sqrt(0.25 * (A11 - A22) ** 2 + A12 * A12)
        lmax, lmin = mean + dev, mean - dev
        assert lmin > 0 and lmax <= 262144.0 * lmin, "axis ratio beyond 512: the kernel stores the sphere stand-in"
        dA = A11 * A22 - A12 * A12
        hx, hy = np.sqrt(A22 / dA), np.sqrt(A11 / dA)
        X, Y = hx + 34.0, hy + 34.0
        Tm = A11 * X * X + 2.0 * abs(A12) * X * Y + A22 * Y * Y + 1.0
        delta = 2.0 ** -12 + 2.0 ** -22 * (abs(c0) + abs(r0) + W + H)
        rel = 2.0 ** -18 * Tm
        grow = 1.0 + delta * np.sqrt(lmax)
        thr = grow * grow * (1.0 + rel)
        assert thr < 1.0e6
        s = [float(np.float32(v)) for v in (c0, r0, A11 / thr, 2.0 * A12 / thr, A22 / thr)]
        x = 1.1933e-7 * ((A11 * A22 + A12 * A12) / dA)
        widen = np.sqrt(thr) * (1.0 + 2.0 ** -22 + x)
        hc, hr = np.float32(hx * widen) * np.float32(1.0000002), np.float32(hy * widen) * np.float32(1.0000002)
        # plane_estimate_record
        a, b, c = (np.dot(n, pj) for pj in P)
        sg = np.sign(k)
        ab3 = lambda v: float(np.sum(np.abs(n * v)))                # noqa: E731
        e = 2.0 ** -19 * (abs(a) + abs(b) * W + abs(c) * H) + 2.0 ** -48 * (ab3(D0) + ab3(Dc) * W + ab3(Dr) * H)
        K = abs(k) * (1.0 - 2.0 ** -20)
        est = [np.float32((sg * a + e) / K), np.float32(sg * b / K), np.float32(sg * c / K),
               np.float32(-1023.0 * e / K) * np.float32(1.0000002)]
        for key, v in zip(keys, [s[0], s[1], s[2], 0.5 * s[3], s[4], *map(float, est), float(hc), float(hr)]):
            out[key].append(v)
    out = {k: np.array(v, dtype=np.float64) for k, v in out.items()}
    return ({k: out[k] for k in ("x0", "y0", "A11", "A12", "A22")}, {k: out[k] for k in ("u0", "u1", "u2", "hi")},
            (out["hc"], out["hr"]))
