"""Shared by the gradient tests (GPU and CPU): fixtures and upstream gradients, scenes whose leaves are torch tensors,
the masked loss every backward is driven with, the winners a frame hands to the fp64 oracle, and the per-array
comparison.  Every helper takes ``device``, so tests/test_grad_cases_cpu.py exercises them on CPU tensors."""
import copy
import json
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from oracle.golden_io import unpack_scene
from oracle.torch_oracle import LEAF_KEYS, OUTPUTS
from views_cases import get_leaf, set_leaf

DEV = "cuda:0"
CAM = ("eye", "at", "up")
NP_KEYS = ("lights.pos", "colors", "materials.albedo")                      # beside the object leaves: numpy shading
TCH_KEYS = ("lights.pos", "lights.attenuation", "lights.ambient", "colors", "materials.albedo", "materials.coeffs")
# two runs of the same backward differ by the order of their fp32 atomic additions (<= 2e-5 of the largest
# entry); a leaked 1e30 or a changed gradient is many orders above that
RUN_TO_RUN = 2e-5


def load(case):
    """(npz, scene, render kwargs) of a reference gradient fixture."""
    npz = np.load(os.path.join(GOLDEN_DIR, case + ".npz"), allow_pickle=False)
    return npz, unpack_scene(npz), json.loads(str(npz["kwargs"]))


def upstream(npz, *keys):
    """The fixture's own upstream gradients {output: fp64 ndarray}, all four by default."""
    return {k: npz["grad_in/" + k].astype(np.float64) for k in keys or OUTPUTS}


def random_upstream(H=36, W=48):
    rng = np.random.RandomState(7)
    g = {"image": rng.uniform(-1, 1, size=(H, W, 3)), "depth": rng.uniform(-1, 1, size=(H, W))}
    rng = np.random.RandomState(11)
    g["normal"] = rng.uniform(-1, 1, size=(H, W, 3))
    g["pos"] = rng.uniform(-1, 1, size=(H, W, 3))
    return {k: v.astype(np.float32).astype(np.float64) for k, v in g.items()}


def grad_kwargs(g):
    """{output: upstream} as the oracle's keyword arguments grad_<output>."""
    return {"grad_" + k: v for k, v in g.items()}


def full_scene(ortho=False, plane=True):
    """The g10 / n1 fixture scene with its spheres (ndarray leaves, from the n1 fixtures); plane=False: without the
    background plane."""
    sc = load("n1_aux_grad_ortho" if ortho else "n1_aux_grad_phong")[1]
    if not plane:
        del sc["objects"]["plane"]
    return sc


def gpu_tensor(a, grad=True, device=DEV):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=device, requires_grad=grad)


def gpu_leaf_scene(scene, extra, skip=(), grad=True, device=DEV):
    """Copy of `scene` whose differentiable arrays (the object leaves and `extra`: NP_KEYS for numpy shading, TCH_KEYS
    for torch shading) are float32 tensors on `device`; those not in `skip` require grad.  Returns (scene, {key: tensor
    that requires grad})."""
    sc = copy.deepcopy(scene)
    leaves = {}
    for key in [f"{kind}.{name}" for kind in sc["objects"] for name in LEAF_KEYS[kind]] + list(extra):
        t = gpu_tensor(get_leaf(sc, key), grad and key not in skip, device)
        set_leaf(sc, key, t)
        if t.requires_grad:
            leaves[key] = t
    return sc, leaves


def camera_leaves(camera, device=DEV, dtype=torch.float32):
    return {k: torch.tensor(np.asarray(camera[k], dtype=np.float64), dtype=dtype, device=device, requires_grad=True)
            for k in CAM}


def masked_loss(res, g, far=None, mask=True):
    """sum image g_i + sum_hit (depth g_d + normal . g_n + pos . g_p) over the outputs named in g (None entries are left
    out); hit = depth <= far under torch shading, far=None: depth finite (numpy shading); mask=False: the sums run over
    every pixel.  `res` is a frame or a batch, g's arrays shaped like its outputs."""
    dep = res["depth"].detach()
    hit = torch.isfinite(dep) if far is None else dep <= float(far)
    loss = torch.zeros((), device=dep.device)
    for k, up in g.items():
        if up is None:
            continue
        term = res[k] * torch.as_tensor(up, dtype=torch.float32, device=dep.device)
        if k != "image" and mask:
            term = torch.where(hit if k == "depth" else hit[..., None], term, torch.zeros_like(term))
        loss = loss + term.sum()
    return loss


def to_np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def winners(res):
    """The frame's own winners, for the oracle to differentiate the same selection."""
    return {"nearest": res["nearest"].cpu().numpy(), "depth": to_np(res["depth"])}


def view_winners(out):
    """winners() per view of a batch."""
    near, dep = out["nearest"].cpu().numpy(), to_np(out["depth"])
    return [{"nearest": near[v], "depth": dep[v]} for v in range(near.shape[0])]


def leaf_grads(leaves):
    """{leaf: fp64 ndarray of its grad}, zeros where it has none."""
    return {k: (to_np(t.grad) if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}


def hip_gradients(scene, g_img, g_dep, device=DEV):
    """render() under numpy shading with leaves on `device`, then masked_loss backward; ({leaf: grad ndarray}, winners)."""
    from surf_renderer_amd import render
    sc, leaves = gpu_leaf_scene(scene, NP_KEYS, device=device)
    res = render(sc, device=device)
    assert res["image"].requires_grad and res["depth"].requires_grad
    masked_loss(res, {"image": g_img, "depth": g_dep}).backward()
    torch.cuda.synchronize()
    assert all(t.grad is not None for t in leaves.values())
    return leaf_grads(leaves), winners(res)


def assert_array_close(got, want, tol, tag=""):
    """|got - want| <= tol * max|want| + 1e-6, `want` finite; prints the figures before it judges them."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    assert np.all(np.isfinite(want)), tag
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{tag}: max|want| {scale:.4g}  max err {err:.3g}  ({err / max(scale, 1e-30):.2g} of max)")
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * scale + 1e-6, err_msg=tag)


def assert_grads_close(got, want, tol, tag="", keys=None):
    """assert_array_close for every array of `want` (those named in `keys`, if given) against got's of the same key."""
    for key, w in want.items():
        if keys is None or key in keys:
            assert_array_close(got[key], w, tol, f"{tag} {key}")


def entry_bounds(absolute, atomics, eps_term):
    """(bound, accumulation part) per gradient entry for the backward kernels' fp32 sums (csrc/srh_backward.h):
    (eps_term + D 2^-24) absolute (1 + 2^-20) and D 2^-24 absolute (1 + 2^-20), where `absolute` is the fp64 oracle's
    sum of the |per-pixel terms| of the entry (torch_oracle.gradient_terms / gradient_terms_tch), eps_term the relative
    error of one term and D = 1 (the cast of the term) + 6 (the run scan or wave_sum) + 2 (the workgroup merge) +
    `atomics` (the atomic additions the entry receives, backward_run_cases.atomic_counts) counts the sequential fp32
    additions on the way to the address."""
    absolute = np.asarray(absolute, dtype=np.float64)
    d = 9.0 + np.broadcast_to(np.asarray(atomics, dtype=np.float64), absolute.shape)
    acc = d * 2.0 ** -24 * absolute * (1.0 + 2.0 ** -20)
    return eps_term * absolute * (1.0 + 2.0 ** -20) + acc, acc


def assert_entries_close(got, want, bound, tag=""):
    """|got - want| <= bound for every entry on its own (an entry whose bound is 0 must be equal); prints and returns the
    largest error over its bound."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)), tag
    err = np.abs(got - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
    bad = np.argwhere(err > bound)
    print(f"{tag}: worst error / bound {ratio:.3g} over {want.size} entries")
    assert not len(bad), (f"{tag}: {len(bad)} entries over their bound, first {tuple(bad[0])}: got {got[tuple(bad[0])]:.9g} "
                          f"want {want[tuple(bad[0])]:.9g} bound {bound[tuple(bad[0])]:.3g}")
    return ratio
