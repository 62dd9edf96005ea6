"""What the GPU tests of the point-wise layers share -- the frame transforms, the point projection, the depth lift, the
plane-fit normals and the hard projection: one bound per entry, against the fp64 restatement and the restatement's own
sum of magnitudes.  Test infrastructure: tests/test_entry_checks_cpu.py holds the helper to its own edges and shows on
the committed fixtures that the reference's float32 results, which pass projection_checks, fail it.

  |got - ref| <= 2^-24 |ref| + C A + 2^-149 [A > 0]      per output element and per gradient entry

  2^-24 |ref|   the one float32 store
  C A           A = the sum of the absolute values of the terms the entry is a sum of (the oracles' `magnitudes`), or a
                stated bound on it no more than 2^8 above.  C = 2^-40 wherever A really bounds the terms: that sits far
                above what a few dozen fp64 roundings lose (about 64 * 2^-53 A, tests/sh9_checks.py) and 2^16 below what
                float32 accumulation loses (about 2^-24 A), so it separates the two without depending on the device
                libm's last bits.  The plane fit, whose determinant cancels, passes a measured C (NORMALS_C64 below)
  2^-149        a subnormal result: the store then rounds to a multiple of 2^-149 and not to 2^-24 of the value

An entry with A == 0 is a sum of nothing and must be exactly 0.  Where `ref` is not finite, `got` must show the same
pattern: NaN where it is NaN, the same infinity where it is one."""
import numpy as np

EPS32, C, TINY = 2.0 ** -24, 2.0 ** -40, 2.0 ** -149

# The plane fit (tests/normals_oracle.py) divides by a d - b^2 + 1e-12, which cancels: no plain sum of magnitudes bounds
# its fp64 error, so its A is max|ref| of the entry's own array and its C is measured, as tests/splat_entry_bounds.py
# does for the sibling plane_fit of srh_splat.h: 4 x the largest (|got - ref| - 2^-24 |ref|) / max|ref| over every entry
# of every normals case on the MI355X, against the fp64 oracle.  The cap is a condition on that measurement, not a
# tolerance: an entry that would need more is ill-conditioned in the oracle itself and is listed by
# ill_conditioned (profiles/entry_bounds.txt).
NORMALS_C64_CAP = 2.0 ** -36
NORMALS_C64_MEASURED = 2.45633e-17      # = 2^-55.18: vertical_plane_5x6's pos.grad; every other array of every case: 0
NORMALS_C64 = 4 * NORMALS_C64_MEASURED
assert NORMALS_C64 <= NORMALS_C64_CAP


def to_np(t):
    """A tensor as the array it is: nothing is widened, so `check` sees the dtype the layer returned."""
    return None if t is None else t.detach().cpu().numpy()


def narrowed(a):
    """A float64 array that holds float32 values -- the gradient of a float64 leaf, which autograd widened from the
    kernel's float32 store -- as float32; asserts that nothing is lost."""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return a
    n = a.astype(np.float32)
    assert a.dtype == np.float64 and np.array_equal(n.astype(np.float64), a, equal_nan=True), "not float32 values"
    return n


def bound(ref, A, floor=C):
    ref, A = np.asarray(ref, np.float64), np.asarray(A, np.float64)
    return EPS32 * np.abs(ref) + floor * A + TINY * (A > 0)


def ratios(got, ref, A, floor=C):
    """error / bound per entry, fp64; 0 where both vanish, inf where the bound vanishes and the error does not.  Finite
    entries of `ref` only make sense here: `check` masks the others."""
    err, b = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)), bound(ref, A, floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))


def check(got, ref, A, where="", floor=C, held=None):
    """float32 `got` against the oracle's fp64 `ref` under the module's bound, A per entry (a scalar is broadcast).
    `held`: a boolean mask of the entries the bound is asserted on (None = all); the dtype, the shape and the
    non-finite pattern are asserted on every entry.  Returns the worst ratio of an error to its bound."""
    got = np.asarray(got)
    assert got.dtype == np.float32, (where, got.dtype)
    ref = np.asarray(ref, np.float64)
    A = np.broadcast_to(np.asarray(A, np.float64), ref.shape)
    assert got.shape == ref.shape, (where, got.shape, ref.shape)
    got = got.astype(np.float64)
    odd = ~np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (where, "NaN pattern")
    inf = odd & ~np.isnan(ref)
    assert np.array_equal(got[inf], ref[inf]), (where, "infinities")
    ok = ~odd if held is None else ~odd & np.broadcast_to(held, ref.shape)
    assert np.all(np.abs(ref[ok]) <= A[ok] * (1 + 2.0 ** -40)), (where, "A below |ref|")
    assert np.all(got[ok & (A == 0)] == 0), (where, "not exactly 0 where A is")
    with np.errstate(invalid="ignore", over="ignore"):
        r = ratios(got, np.where(ok, ref, 0.0), np.where(ok, A, 0.0), floor)[ok]
    worst = float(r.max(initial=0.0))
    assert worst <= 1.0, (where, worst, int((r > 1).sum()), r.size)
    return worst


def check_all(got, ref, A, where="", floor=C):
    """`check` on every array of `ref`; `got` and `A` hold the same names.  Prints and returns the worst ratio."""
    assert set(ref) <= set(got) and set(ref) <= set(A), (where, sorted(got), sorted(ref), sorted(A))
    worst = max([check(got[k], ref[k], A[k], f"{where} {k}", floor) for k in ref], default=0.0)
    print(f"{where}: worst error / bound {worst:.3g}")
    return worst


def check_plane_fit(got, ref, second, where="", floor=None):
    """An array of the plane fit -- normals or pos.grad -- against the fp64 restatement `ref` and the restatement's
    second evaluation `second` (normals_oracle.turned_gradients): A = max|ref| over the finite entries, C = NORMALS_C64.
    The entries ill_conditioned lists keep the array-scale tolerance (rtol 2e-6, atol 2e-7 of the scale: never wider
    than projection_checks').  Returns (the worst ratio, the number of entries left on the old tolerance)."""
    ref, second = np.asarray(ref, np.float64), np.asarray(second, np.float64)
    fin = np.isfinite(ref)
    scale = float(np.abs(ref[fin]).max()) if fin.any() else 0.0
    with np.errstate(invalid="ignore"):
        ill = fin & ill_conditioned(ref, second, scale)
    worst = check(got, ref, scale, where, NORMALS_C64 if floor is None else floor, held=~ill)
    g = np.asarray(got, np.float64)
    assert np.all(np.abs(g[ill] - ref[ill]) <= 2e-6 * np.abs(ref[ill]) + 2e-7 * scale), (where, "ill-conditioned entries")
    print(f"{where}: worst error / bound {worst:.3g}, {int(ill.sum())} of {ref.size} entries on the array-scale tolerance")
    return worst, int(ill.sum())


def share_beyond(got, ref, A, floor=C):
    """(entries beyond the bound, finite entries) of `got` against `ref`: what the CPU test counts on the recorded
    float32 results."""
    ref = np.asarray(ref, np.float64)
    assert np.shape(got) == ref.shape, (np.shape(got), ref.shape)
    ok = np.isfinite(ref)
    A = np.broadcast_to(np.asarray(A, np.float64), ref.shape)
    r = ratios(np.where(ok, got, 0.0), np.where(ok, ref, 0.0), np.where(ok, A, 0.0), floor)[ok]
    return int((r > 1).sum()), int(r.size)


def camera_jacobian(table_fn, camera):
    """[B, 12, 9] fp64: d table[b] / d (eye, at, up)[b] of `table_fn(eye, at, up) -> [B, 3, 4]`, one of the oracle's own
    lookat / lookat_inv compositions, by torch.autograd.functional.jacobian per view."""
    import torch
    vec = [np.asarray(camera[k], np.float64)[..., :3] for k in ("eye", "at", "up")]
    out = []
    for b in range(vec[0].shape[0]):
        x = torch.tensor(np.concatenate([v[b] for v in vec]))
        J = torch.autograd.functional.jacobian(lambda x: table_fn(x[None, 0:3], x[None, 3:6], x[None, 6:9])[0].reshape(12), x)
        out.append(J.numpy())
    return np.stack(out)


def camera_magnitudes(tables, camera):
    """{eye, at, up: A in the entry's own shape}: A_cam = sum over the tables of |J|^T A_M.  `tables` is a list of
    (table_fn, A_M [B, 3, 4]): each entry of a table gradient d loss / dM[r][c] is a fp64 sum over the points with
    A_M = sum |g_r| |v_c|, and the chain from M to eye / at / up is fp64 on the host, a contraction with the 12 x 9
    Jacobian J.  The w column of a homogeneous entry gets A = 0: it is dropped before lookat."""
    B = np.asarray(camera["eye"]).shape[0]
    total = np.zeros((B, 9))
    for table_fn, A_M in tables:
        J = camera_jacobian(table_fn, camera)
        total += np.einsum("bkj,bk->bj", np.abs(J), np.asarray(A_M, np.float64).reshape(B, 12))
    out = {}
    for i, k in enumerate(("eye", "at", "up")):
        A = np.zeros(np.asarray(camera[k]).shape)
        A[..., :3] = total[:, 3 * i:3 * i + 3]
        out[k] = A
    return out


def ill_conditioned(first, second, scale, cap=NORMALS_C64_CAP):
    """Boolean mask of the entries whose two fp64 evaluations -- the oracle on the map as given and on the map turned by
    180 degrees, turned back -- differ by more than cap * scale / 4: there the oracle's own fp64 rounding reaches the
    floor, so no kernel can be held to it."""
    return np.abs(np.asarray(first, np.float64) - np.asarray(second, np.float64)) > cap * scale / 4
