"""What the two GPU test files of the point-set layer share -- test infrastructure: running the layer on numpy inputs,
the oracle's result for a view, and the two bounds.

  values:    |got - want| <= 1 float32 ulp at want.  The fp64 distance is within (D + 3) 2^-53 relative of exact, so
             after the one rounding to float32 it is the nearest or a neighbouring float32 of the oracle's value.
  gradients: |got - ref| <= 2^-23 |ref| + 2^-40 S per entry, S = the oracle's sum of |terms|: one float32 rounding
             (half an ulp is at most 2^-24 relative; 2^-23 also covers a subnormal's spacing up to the first normal
             binade) plus the fp64 accumulation of at most 2^24 terms of relative error a few 2^-53 each.  Below
             float32's subnormals the store itself is off by up to its spacing there, 2^-149, whatever the value
             (extreme_magnitudes has a gradient entry of 4e-79, stored as 0): that absolute term is added."""
import numpy as np
import torch

import pointsets_oracle as oracle

DEV = "cuda:0"


def leaf(a, dtype=torch.float32, device=DEV, requires_grad=True):
    return torch.tensor(np.asarray(a), dtype=dtype, device=device).requires_grad_(requires_grad)


def run(u, v, g_u=None, g_v=None, **kw):
    """nearest_points on numpy inputs with the loss sum(dist_u g_u) + sum(dist_v g_v) (a None upstream leaves its output
    out of the loss): ({dist_u, idx_u, dist_v, idx_v, grad_u, grad_v} as numpy arrays, None where there is none)."""
    from surf_renderer_amd import nearest_points
    tu, tv = leaf(u), leaf(v)
    r = nearest_points(tu, tv, **kw)
    terms = [(d * torch.tensor(g, device=DEV)).sum() for d, g in ((r.dist_u, g_u), (r.dist_v, g_v))
             if g is not None and d is not None]
    if terms:
        torch.autograd.backward(sum(terms))
    out = {k: (None if t is None else t.detach().cpu().numpy()) for k, t in r._asdict().items()}
    out["grad_u"], out["grad_v"] = (None if t.grad is None else t.grad.cpu().numpy() for t in (tu, tv))
    return out


def view_oracle(u, v, g_u=None, g_v=None, squared=False):
    r = oracle.nearest(u, v, squared)
    r.update(oracle.gradients(u, v, r["idx_u"], r["idx_v"], g_u, g_v, squared))
    return r


def check_values(got, want, where=""):
    """float32 `got` against the oracle's fp64 `want`: equal where want is inf or 0, else within one float32 ulp.
    Returns the worst error in ulp."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    exact = ~np.isfinite(want) | (want == 0)
    assert np.array_equal(got[exact], want[exact]), where
    err = np.abs(got[~exact] - want[~exact]) / oracle.ulp32(want[~exact])
    assert (err <= 1.0).all(), (where, err.max())
    return err.max(initial=0.0)


def check_grads(got, ref, S, where=""):
    """Every entry finite, within its bound, and exactly 0 where the oracle has no non-zero term.  Returns the worst
    ratio of an error to its bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), where
    assert (got[S == 0] == 0).all(), where
    err, bound = np.abs(got - ref), 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * S + 2.0 ** -149 * (S > 0)
    assert (err <= bound).all(), (where, (err / np.where(bound > 0, bound, 1)).max())
    return (err[bound > 0] / bound[bound > 0]).max(initial=0.0)
