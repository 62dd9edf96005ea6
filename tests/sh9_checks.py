"""What the two GPU test files of the SH9 lighting layer share -- test infrastructure: running the layer on numpy inputs,
the oracle's results per case, and the one bound.

  |got - ref| <= 2^-24 |ref| + 2^-40 A per output element and per gradient entry, A = the oracle's sum of |terms| of
  that entry.  The first term is the one float32 store.  The second sits 2^13 above what fp64 evaluation can lose
  (about 64 * 2^-53 * A) and 2^16 below what float32 accumulation loses (about 2^-24 * A): it separates the two without
  depending on the device libm's last bits.  Where the oracle's entry is not finite, `got` must show the same pattern
  (NaN, +Inf or -Inf)."""
import functools

import numpy as np
import torch

import sh9_cases as cases
import sh9_oracle as oracle

DEV = "cuda:0"


def leaf(a, dtype=torch.float32, device=DEV, requires_grad=True):
    return torch.tensor(np.asarray(a), dtype=dtype, device=device).requires_grad_(requires_grad)


def numpy_of(t):
    return None if t is None else t.detach().cpu().numpy()


def check(got, ref, A, where=""):
    """float32 `got` against the oracle's fp64 `ref`.  Returns the worst ratio of an error to its bound."""
    assert got.dtype == np.float32, where
    got, ref, A = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(A, np.float64)
    assert got.shape == ref.shape == A.shape, (where, got.shape, ref.shape, A.shape)
    odd = ~np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), where
    assert np.array_equal(got[odd & ~np.isnan(ref)], ref[odd & ~np.isnan(ref)]), where                # the infinities' signs
    err = np.abs(got - ref)[~odd]
    bound = (2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * A)[~odd]
    assert (err <= bound).all(), (where, (err / np.where(bound > 0, bound, 1)).max())
    return (err[bound > 0] / bound[bound > 0]).max(initial=0.0)


def run_projection(envmap, g_L=None, batched=True):
    """radiance_SH9_batched (or radiance_SH9 on one probe) with the loss sum(L g_L): {L, grad_envmap}"""
    from surf_renderer_amd import radiance_SH9, radiance_SH9_batched
    env = leaf(envmap)
    L = (radiance_SH9_batched if batched else radiance_SH9)(env)
    if g_L is not None:
        (L * torch.tensor(np.asarray(g_L), device=DEV)).sum().backward()
    return {"L": numpy_of(L), "grad_envmap": numpy_of(env.grad)}


def run_irradiance(M, normal, g_E=None, leaves=("M", "normal")):
    """irradiance_batched with the loss sum(E g_E): {E, grad_M, grad_normal}; an input not among `leaves` does not
    require grad and gets None"""
    from surf_renderer_amd import irradiance_batched
    tM, tn = leaf(M, requires_grad="M" in leaves), leaf(normal, requires_grad="normal" in leaves)
    E = irradiance_batched(tM, tn)
    if g_E is not None and leaves:
        (E * torch.tensor(np.asarray(g_E), device=DEV)).sum().backward()
    return {"E": numpy_of(E), "grad_M": numpy_of(tM.grad), "grad_normal": numpy_of(tn.grad)}


def projection_truth_of(envmap, g_L):
    """per view {L, A_L, grad_envmap, A_envmap}"""
    out = []
    for env, g in zip(envmap, g_L):
        L, A = oracle.project(env)
        grad, A_g = oracle.project_grad(env.shape, g)
        out.append({"L": L, "A_L": A, "grad_envmap": grad, "A_envmap": A_g})
    return out


def irradiance_truth_of(c):
    """per view oracle.irradiance_view, and under "shared" the views' grad_M and A_M added in ascending view order"""
    views = [oracle.irradiance_view(cases.view_M(c, b), c["normal"][b], c["g_E"][b]) for b in range(len(c["normal"]))]
    shared = {"grad_M": functools.reduce(np.add, [v["grad_M"] for v in views]),
              "A_M": functools.reduce(np.add, [v["A_M"] for v in views])}
    return views, shared


@functools.lru_cache(maxsize=None)
def projection_truth(k):
    c = cases.projection(k)
    return projection_truth_of(c["envmap"], c["g_L"])


@functools.lru_cache(maxsize=None)
def irradiance_truth(k):
    return irradiance_truth_of(cases.irradiance(k))


def check_projection(got, T, where=""):
    worst = 0.0
    for b, t in enumerate(T):
        worst = max(worst, check(got["L"][b], t["L"], t["A_L"], f"{where} L, view {b}"))
        if got["grad_envmap"] is not None:
            worst = max(worst, check(got["grad_envmap"][b], t["grad_envmap"], t["A_envmap"], f"{where} grad_envmap, view {b}"))
            assert (got["grad_envmap"][b][t["A_envmap"] == 0] == 0).all(), where          # exactly 0 outside the disc
    return worst


def check_irradiance(got, c, T, where=""):
    views, shared = T
    worst = 0.0
    for b, t in enumerate(views):
        worst = max(worst, check(got["E"][b], t["E"], t["A_E"], f"{where} E, view {b}"))
        if got["grad_normal"] is not None:
            worst = max(worst, check(got["grad_normal"][b], t["grad_normal"], t["A_normal"], f"{where} grad_normal, view {b}"))
        if got["grad_M"] is not None and c["M"].ndim == 4:
            worst = max(worst, check(got["grad_M"][b], t["grad_M"], t["A_M"], f"{where} grad_M, view {b}"))
    if got["grad_M"] is not None and c["M"].ndim == 3:
        worst = max(worst, check(got["grad_M"], shared["grad_M"], shared["A_M"], f"{where} shared grad_M"))
    return worst
