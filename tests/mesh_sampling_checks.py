"""What the two GPU test files of the mesh-sampling layer share -- test infrastructure: running the layer on numpy
inputs, the oracle's result for a view, and the two bounds.

  values:    |got - want| <= 2^-24 |want| + 2^-50 S per entry of bary, pos and normal, S = the oracle's sum of |terms|
             of that entry: the one rounding to float32 is at most half an ulp, 2^-24 relative, and the fp64 arithmetic
             in front of it -- a handful of operations of relative error 2^-53 each, on terms whose absolute sum is S
             -- differs from the oracle's by its order of operations at the most.
  gradients: |got - ref| <= 2^-23 |ref| + 2^-40 S per entry, the bound and the shape of tests/pointsets_checks.py: one
             float32 rounding plus the fp64 accumulation of at most 2^24 terms of relative error a few 2^-53 each.
  `subnormal`: inputs that reach below float32's normal range (vertices of 1e-30).  There the store itself is off by up
             to float32's spacing 2^-149, whatever the value: that absolute term is added, as in the point-set edge tests."""
import numpy as np
import torch

import mesh_sampling_cases as cases
import mesh_sampling_oracle as oracle

DEV = "cuda:0"


def leaf(a, dtype=torch.float32, device=DEV, requires_grad=True):
    return torch.tensor(np.asarray(a), dtype=dtype, device=device).requires_grad_(requires_grad)


def run(v, f, uniforms, eye=None, g_pos=None, g_normal=None, topology=None):
    """sample_mesh_batched on numpy inputs with the loss sum(pos g_pos) + sum(normal g_normal) (a None upstream leaves
    its output out of the loss): {pos, normal, face, bary, grad_v} as numpy arrays, grad_v None without a loss."""
    from surf_renderer_amd import sample_mesh_batched
    tv = leaf(v)
    uniforms, eye = np.array(uniforms), (None if eye is None else np.array(eye))      # the cases' arrays are read-only
    r = sample_mesh_batched(tv, f, uniforms, eye=eye, topology=topology)
    terms = [(x * torch.tensor(np.asarray(g), device=DEV)).sum() for x, g in ((r.pos, g_pos), (r.normal, g_normal))
             if g is not None]
    if terms:
        torch.autograd.backward(sum(terms))
    out = {k: t.detach().cpu().numpy() for k, t in r._asdict().items()}
    out["grad_v"] = None if tv.grad is None else tv.grad.cpu().numpy()
    return out


def run_case(c, views=slice(None), upstream=("g_pos", "g_normal"), **kw):
    """run() on the views `views` (a slice, or an int for the unbatched call) of a regular case"""
    f = c["f"] if c["f"].ndim == 2 else c["f"][views]
    eye = c["eye"] if c["eye"] is None or c["eye"].ndim == 1 else c["eye"][views]
    ups = {k: (c[k][views] if k in upstream else None) for k in ("g_pos", "g_normal")}
    return run(c["v"][views], f, c["uniforms"][views], eye, ups["g_pos"], ups["g_normal"], **kw)


def view_oracle(v, f, uniforms, eye=None, g_pos=None, g_normal=None):
    r = oracle.forward(v, f, uniforms, eye)
    r.update(oracle.gradients(v, f, r["face"], r["bary"], g_pos, g_normal))
    return r


def check_values(got, want, S, where="", subnormal=False):
    """float32 `got` against the oracle's fp64 `want`, NaN where it is NaN.  Returns the worst ratio of an error to
    its bound."""
    got, want, S = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(S, np.float64)
    assert got.shape == want.shape, where
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), where
    err = np.abs(got - want)[~nan]
    bound = (2.0 ** -24 * np.abs(want) + 2.0 ** -50 * S)[~nan] + (2.0 ** -149 if subnormal else 0.0)
    assert (err <= bound).all(), (where, (err / np.where(bound > 0, bound, 1)).max())
    return (err[bound > 0] / bound[bound > 0]).max(initial=0.0)


def check_grads(got, ref, S, where="", subnormal=False):
    """Every entry finite, within its bound, and exactly 0 where the oracle has no non-zero term.  Returns the worst
    ratio of an error to its bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), where
    assert (got[S == 0] == 0).all(), where
    err = np.abs(got - ref)
    bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * S + (2.0 ** -149 * (S > 0) if subnormal else 0.0)
    assert (err <= bound).all(), (where, (err / np.where(bound > 0, bound, 1)).max())
    return (err[bound > 0] / bound[bound > 0]).max(initial=0.0)


def check_view(got, T, b=None, where="", subnormal=False):
    """view b of a batch's results (or an unbatched result) against the oracle's view T.  Returns (values, gradients):
    the worst ratios."""
    pick = (lambda a: a) if b is None else (lambda a: a[b])
    assert np.array_equal(pick(got["face"]), T["face"]), where
    worst = max(check_values(pick(got[k]), T[k], T["S_" + k], f"{where} {k}", subnormal) for k in ("bary", "pos", "normal"))
    worst_g = 0.0
    if got["grad_v"] is not None:
        worst_g = check_grads(pick(got["grad_v"]), T["grad_v"], T["S_v"], f"{where} grad_v", subnormal)
    return worst, worst_g


def uniforms_for(v, f, n_samples, seed, eye=None):
    """seeded uniforms whose r0 keep their distance from the view's CDF (cases.seeded_uniforms)"""
    w = oracle.face_quantities(v, f, eye)["weight"]
    return cases.seeded_uniforms(w, n_samples, seed)[0]
