"""A numpy fp64 brute force of surf_renderer_amd.pointsets with exactly its rules -- test infrastructure, one view at a
time.  The (N, M) matrix the kernels never form is formed here.

  d2(i, j) = ((u_i0 - v_j0)^2 + (u_i1 - v_j1)^2) + ...      fp64 on the float32 values, components ascending
  winner   = the lowest index among the smallest FINITE d2; without one, idx = 0 and dist = +inf
  dir(p, o) = (p - o) / |p - o|  (2 (p - o) under `squared`), exactly 0 where d2 is 0 or not finite
  grad_u[i] = g_u[i] dir(u_i, v_idx_u[i]) + sum over { j : idx_v[j] = i } of g_v[j] dir(u_i, v_j),  grad_v likewise
and for each gradient entry S = the sum of |terms|, which scales its rounding bound.  The kernels square and add with
FMAs and this file without: the values agree to a few fp64 ulp, the indices wherever the best d2 has a margin or the
tie is exact in both (equal points, small integers)."""
import numpy as np


def pair_d2(q, t):
    """d2 [N, M] of q [N, D] against t [M, D]"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, None, :] - t[None, :, :]
        s = d[..., 0] * d[..., 0]
        for c in range(1, d.shape[-1]):
            s = s + d[..., c] * d[..., c]
    return s


def one_sided(q, t, squared=False):
    """(dist [N] fp64, idx [N] int64, d2 [N, M]) of every q_i's nearest t"""
    s = pair_d2(q, t)
    finite = np.where(np.isfinite(s), s, np.inf)
    idx = np.argmin(finite, axis=1)                       # the first of equal minima; 0 for a row of +inf
    best = finite[np.arange(len(idx)), idx]
    return (best if squared else np.sqrt(best)), idx.astype(np.int64), s


def nearest(u, v, squared=False):
    """{dist_u, idx_u, dist_v, idx_v} of one view, dist in fp64 (the layer stores float32(dist))"""
    dist_u, idx_u, _ = one_sided(u, v, squared)
    dist_v, idx_v, _ = one_sided(v, u, squared)
    return {"dist_u": dist_u, "idx_u": idx_u, "dist_v": dist_v, "idx_v": idx_v}


def _terms(p, o, g, squared):
    """g dir(p, o) row by row: p, o [K, D], g [K] -> [K, D]"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = p - o
        s = d[:, 0] * d[:, 0]
        for c in range(1, d.shape[1]):
            s = s + d[:, c] * d[:, c]
        ok = np.isfinite(s) & (s > 0)
        w = 2.0 * g if squared else g / np.sqrt(np.where(ok, s, 1.0))
        return np.where(ok[:, None], w[:, None] * np.where(ok[:, None], d, 0.0), 0.0)


def gradients(u, v, idx_u, idx_v, g_u, g_v, squared=False):
    """{grad_u, grad_v, S_u, S_v} of one view for the upstream gradients g_u [N] of dist_u and g_v [M] of dist_v; either
    may be None = zero, and idx_v is then not needed (the directed call)."""
    u, v = np.asarray(u, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    grad = {"u": np.zeros_like(u), "v": np.zeros_like(v)}
    S = {"u": np.zeros_like(u), "v": np.zeros_like(v)}
    for own, other, p, o, idx, g in (("u", "v", u, v, idx_u, g_u), ("v", "u", v, u, idx_v, g_v)):
        if g is None:
            continue
        t = _terms(p, o[idx], np.asarray(g, np.float64), squared)        # d dist_own[i] / d p_i
        grad[own] += t
        S[own] += np.abs(t)
        np.add.at(grad[other], idx, -t)                                  # ... / d o_idx[i], the fan-in
        np.add.at(S[other], idx, np.abs(t))
    return {"grad_u": grad["u"], "grad_v": grad["v"], "S_u": S["u"], "S_v": S["v"]}


def hausdorff(r):
    """(sym, uv, vu) of nearest()'s result in the reference's orientation: uv = max_j dist_v[j]"""
    uv, vu = r["dist_v"].max(), r["dist_u"].max()
    return max(uv, vu), uv, vu


def hausdorff_upstreams(r, g3):
    """(g_u, g_v): the upstream gradients of dist_u and dist_v under the loss g3 . (sym, uv, vu), as torch carries them:
    maximum(a, b) halves a tie, and a whole-tensor max shares its gradient evenly among tied maxima."""
    sym, uv, vu = hausdorff(r)
    to_uv = g3[1] + g3[0] * (1.0 if uv > vu else 0.5 if uv == vu else 0.0)
    to_vu = g3[2] + g3[0] * (1.0 if vu > uv else 0.5 if uv == vu else 0.0)
    at_v, at_u = r["dist_v"] == uv, r["dist_u"] == vu
    return to_vu * at_u / at_u.sum(), to_uv * at_v / at_v.sum()


def ulp32(x):
    """the spacing of float32 at |x| (of the smallest normal below it)"""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)
