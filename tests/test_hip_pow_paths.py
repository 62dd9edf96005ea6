"""GPU: the kernels' fp32 power functions on both sides of their switches -- tonemap_f32 / tonemap_zero / spec_pow_f32
(csrc/srh_device.h) and the tonemap slope of the two backward kernels (csrc/srh_backward.h) -- against the fp64 oracles,
on the scenes of tests/pow_scenes.py (tests/test_pow_scenes_cpu.py proves that they reach every branch).

Tolerances
  forward   tests/test_hip_parity.py's budget for every pixel: nearest identical, depth one fp32 ulp, image
            2e-7 + 2e-6 |x|; a specular lobe adds the bound derived at spec_pow_f32 (_lobe_reference below).
  backward  materials.albedo (ladder) and materials.coeffs (lobes) PER ENTRY, 2e-4 |want[m, c]|: every entry is a sum of
            same-sign terms of one magnitude, so the project's 2e-4 of fp32 accumulation applies to the entry itself and
            not only to the array's largest one -- which on the ladder is 1e20 times the smallest.  Other leaves as in
            tests/test_hip_backward.py: 2e-4 max|want| + 1e-6 per array.

Checked by making them fail (scratch copies of the kernels, one edit each; the rest of the GPU suite stayed green):
  tonemap_slope's fallback pow(x, gamma) for pow(x, gamma - 1)   test_tonemap_slope_sweep[numpy] at 0.25, 1/2.2, 1.5, 2.2, 4
  tonemap_f32's fallback powf(x, 0.8f) for powf(x, g)            test_tonemap_forward_sweep at every gamma but 0.8, and
                                                                 all of test_tonemap_non_positive_gamma
  tonemap_zero's 0 for 1 at gamma == 0                           test_tonemap_non_positive_gamma[0.0-*]
"""
import functools

import numpy as np
import pytest
import torch

from grad_cases import TCH_KEYS, gpu_leaf_scene, hip_gradients, leaf_grads, masked_loss
from oracle import np_oracle, np_oracle_tch, torch_oracle
from pow_scenes import EXPONENTS, GAMMAS, ladder_scene, lobe_scene, without_tonemap
from test_hip_parity import IMAGE_ATOL, IMAGE_RTOL, assert_parity

pytestmark = pytest.mark.gpu

SHADINGS = ("numpy", "torch")
GAMMA_IDS = [f"{g:.3g}" for g in GAMMAS]


def _render(scene, shading, **kw):
    from surf_renderer_amd import render
    res = render(scene, device="cuda:0", **({"shading": "torch"} if shading == "torch" else {}), **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in ("image", "depth", "nearest")}


def _oracle(scene, shading, **kw):
    from surf_renderer_amd.scene import scene_to_numpy
    sc = scene_to_numpy(scene, round_fp32=True)
    with np.errstate(all="ignore"):
        return np_oracle_tch.render(sc, **kw) if shading == "torch" else np_oracle.render(sc)


def _report(tag, got, want):
    """The figures an assertion is about to judge: worst image error in units of the 2e-7 + 2e-6 |x| budget."""
    with np.errstate(all="ignore"):
        err = np.abs(got["image"].astype(np.float64) - want["image"]) / (IMAGE_ATOL + IMAGE_RTOL * np.abs(want["image"]))
    err = np.where(np.isfinite(err), err, 0.0)
    print(f"{tag}: worst image error {err.max():.3f} of the budget, nearest differs on "
          f"{(got['nearest'] != want['nearest']).sum()} pixels")


def _modes_identical(scene, shading, ref, **kw):
    for wpt in (1, 4):
        got = _render(scene, shading, mode="binned", waves_per_tile=wpt, **kw)
        for k in ("nearest", "depth", "image"):
            assert np.array_equal(got[k], ref[k], equal_nan=True), f"binned (waves_per_tile {wpt}) vs exact: {k}"


# ---- a. the tonemap, forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shading", SHADINGS)
@pytest.mark.parametrize("gamma", GAMMAS, ids=GAMMA_IDS)
def test_tonemap_forward_sweep(gamma, shading):
    """Pixel values from 2e-31 to 1e15 and exact zeros under every gamma: the hardware path, its underflow end and the
    library powf beyond gamma * log2 x = 12, every pixel against the oracle; all render modes bit-identical."""
    scene = ladder_scene(gamma, shading=shading)
    want = _oracle(scene, shading)
    got = _render(scene, shading, mode="exact")
    _report(f"gamma {gamma:.4g} {shading}", got, want)
    assert_parity(got, want)
    _modes_identical(scene, shading, got)


@pytest.mark.parametrize("shading", SHADINGS)
def test_tonemap_forward_denormal_values(shading):
    """Light colour 1e-12: pixel values down to 2e-43, denormal once cast to fp32.  The hardware log2 may flush them;
    the image must stay within the absolute budget all the same."""
    scene = ladder_scene(0.8, shading=shading, light_colour=1e-12)
    want = _oracle(scene, shading)
    got = _render(scene, shading, mode="exact")
    _report(f"denormal ladder {shading}", got, want)
    assert_parity(got, want)
    _modes_identical(scene, shading, got)


# ---- b. gamma <= 0, forward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "binned"])
@pytest.mark.parametrize("shading", SHADINGS)
@pytest.mark.parametrize("gamma", [0.0, -1.0])
def test_tonemap_non_positive_gamma(gamma, shading, mode):
    """0 ** 0 = 1 and 0 ** -1 = +inf: tonemap_zero on background pixels (the binned kernel's own background store in
    mode 'binned', shade_pixel's masked pixel in mode 'exact') and powf's special values on the hit pixels of the
    albedo-0 disc; x ** -1 on the others."""
    scene = ladder_scene(gamma, shading=shading)
    want = _oracle(scene, shading)
    got = _render(scene, shading, mode=mode)
    np.testing.assert_array_equal(got["nearest"], want["nearest"])
    want32 = want["image"].astype(np.float32)
    hit = want["depth"] <= scene["camera"]["far"]
    background = 1.0 if gamma == 0.0 else np.inf
    assert (~hit).any() and (got["image"][~hit] == background).all()
    assert (want32 == background).sum() >= 27 + 3 * (~hit).sum()
    np.testing.assert_array_equal(got["image"] == background, want32 == background)
    np.testing.assert_array_equal(np.isfinite(got["image"]), np.isfinite(want32))
    np.testing.assert_allclose(got["image"], want32, rtol=IMAGE_RTOL, atol=IMAGE_ATOL, equal_nan=True)


# ---- c. the tonemap's slope, backward ----------------------------------------------------------------------------------
def _assert_gradients(tag, got, want, per_entry):
    """`per_entry`: |got - want| <= 2e-4 |want| + 1e-30 entry by entry; every other leaf 2e-4 max|want| + 1e-6.  Every
    figure is printed before the first assertion."""
    failures = []
    for key, w in sorted(want.items(), key=lambda kv: kv[0] != per_entry):
        g = got[key].reshape(w.shape)
        assert np.isfinite(w).all() and np.isfinite(g).all(), f"{tag} {key}: not finite"
        err = np.abs(g - w)
        if key == per_entry:
            with np.errstate(all="ignore"):
                rel = np.where(w != 0, err / np.abs(w), 0.0)
            print(f"{tag} {key}: worst per-entry error {rel.max():.3e} |want| at entry "
                  f"{tuple(int(i) for i in np.unravel_index(rel.argmax(), rel.shape))}, |want| from "
                  f"{np.abs(w[w != 0]).min():.3e} to {np.abs(w).max():.3e}")
            bad = err > 2e-4 * np.abs(w) + 1e-30
        else:
            scale = np.abs(w).max()
            print(f"{tag} {key}: worst error {err.max() / max(scale, 1e-300):.3e} max|want|, max|want| = {scale:.3e}")
            bad = err > 2e-4 * scale + 1e-6
        if bad.any():
            i = tuple(int(k) for k in np.argwhere(bad)[0])
            failures.append(f"{key}: {bad.sum()} entries beyond the tolerance, first {i}: got {g[i]!r}, want {w[i]!r}")
    assert not failures, f"{tag}: " + "; ".join(failures)


def _upstream(scene, seed):
    vp = scene["camera"]["viewport"]
    return np.random.RandomState(seed).uniform(0.5, 1.0, size=(vp[3], vp[2], 3)).astype(np.float32).astype(np.float64)


def _gradients_tch(scene, g_img, **kw):
    """render(shading='torch') under autograd on GPU leaves, and the gradient oracle on the same winners."""
    from surf_renderer_amd import render
    ref = np_oracle_tch.render(scene, **kw)
    leaf_scene, leaves = gpu_leaf_scene(scene, TCH_KEYS)
    res = render(leaf_scene, device="cuda:0", shading="torch", **kw)
    np.testing.assert_array_equal(res["nearest"].cpu().numpy(), ref["nearest"])
    masked_loss(res, {"image": g_img}).backward()
    torch.cuda.synchronize()
    return leaf_grads(leaves), torch_oracle.gradients_tch(scene, g_img, None, ref=ref, **kw)


@pytest.mark.parametrize("shading", SHADINGS)
@pytest.mark.parametrize("gamma", GAMMAS, ids=GAMMA_IDS)
def test_tonemap_slope_sweep(gamma, shading):
    """d image / d albedo of every rung of the ladder, per entry: the dim rungs are where tonemap_slope (numpy shading)
    leaves its hardware path for the fp64 pow and where the torch-shading kernel's powf(im, gamma - 1) meets small
    arguments.  An all-positive upstream gradient and no depth loss keep every entry a same-sign sum."""
    scene = ladder_scene(gamma, lo=-12.0, hi=min(4.0, 30.0 / gamma), shading=shading)
    g_img = _upstream(scene, 7)
    if shading == "torch":
        got, want = _gradients_tch(scene, g_img)
    else:
        got, fwd = hip_gradients(scene, g_img, None)
        want = torch_oracle.gradients(scene, g_img, None, ref=fwd)
    w = want["materials.albedo"]
    assert np.all(w[0] == 0) and np.all(w[1:] > 0)          # albedo 0: the clip's side of the tonemap, gradient 0
    assert np.all(got["materials.albedo"][0] == 0)
    _assert_gradients(f"gamma {gamma:.4g} {shading}", got, want, "materials.albedo")


# ---- d. the specular lobe ----------------------------------------------------------------------------------------------
LOBE_EVAL = (1.5 * 12.0 * np.log(2.0) + 1.0) * 2.0 ** -23      # exp2(n * log2 x) on |y| <= 12, see spec_pow_f32


@functools.lru_cache(maxsize=None)
def _lobe_reference(double_sided):
    """The oracle's frame of the lobe scene and, per pixel, the bound on |image error| derived at spec_pow_f32
    (csrc/srh_device.h): the lobe term of exponent n carries a relative error of n 2^-24 (its base rounded to fp32) plus
    LOBE_EVAL (log2, product and exp2 at 1 ulp each on |y| <= 12; powf's 2 ulp on the fallback are less).  The lobes'
    share of a pixel before the tonemap is the difference between the frames with and without specular coefficients;
    x ** gamma passes a small error d on as gamma x ** (gamma - 1) d.  All of it on top of the project's budget."""
    scene = lobe_scene()
    want = _oracle(scene, "torch", double_sided=double_sided)
    pre = _oracle(without_tonemap(scene), "torch", double_sided=double_sided)["image"]
    diffuse = without_tonemap(scene)
    diffuse["materials"]["coeffs"] = diffuse["materials"]["coeffs"] * np.array([1.0, 0.0, 1.0])
    spec = pre - _oracle(diffuse, "torch", double_sided=double_sided)["image"]
    assert (spec >= 0).all() and (spec > 0).any()
    hit = want["depth"] <= scene["camera"]["far"]
    n = np.asarray(EXPONENTS, dtype=np.float64)[want["nearest"]]
    eps = np.where(hit, n * 2.0 ** -24 + LOBE_EVAL, 0.0)[..., None]
    gamma = scene["tonemap"]["gamma"]
    with np.errstate(all="ignore"):
        slope = np.where(pre > 0, gamma * want["image"] / pre, 0.0)
    bound = IMAGE_ATOL + IMAGE_RTOL * np.abs(want["image"]) + slope * eps * spec
    return scene, want, bound


@pytest.mark.parametrize("double_sided", [False, True])
def test_specular_lobe_forward(double_sided):
    scene, want, bound = _lobe_reference(double_sided)
    got = _render(scene, "torch", mode="exact", double_sided=double_sided)
    _report(f"lobes double_sided={double_sided}", got, want)
    np.testing.assert_array_equal(got["nearest"], want["nearest"])
    np.testing.assert_allclose(got["depth"], want["depth"], rtol=1.2e-7)
    err = np.abs(got["image"].astype(np.float64) - want["image"])
    for m, n in enumerate(EXPONENTS):
        own = want["nearest"] == m
        print(f"  n = {n}: worst error {np.max(err[own] / bound[own]):.3f} of the derived bound, "
              f"{np.max(err[own] / (IMAGE_ATOL + IMAGE_RTOL * want['image'][own])):.3f} of the plain budget")
    assert (err <= bound).all(), f"{(err > bound).sum()} values beyond the derived bound, worst {np.max(err / bound):.3f} of it"
    _modes_identical(scene, "torch", got, double_sided=double_sided)


@pytest.mark.parametrize("double_sided", [False, True])
def test_specular_lobe_backward(double_sided):
    """d image / d (c0, c1, n) of every material, per entry: c0 and c1 collect non-negative terms, n collects
    lobe * ln rdotc <= 0 -- also at n = 0, where the lobe is 1 and torch gives the base-0 pixels no gradient."""
    scene = lobe_scene()
    got, want = _gradients_tch(scene, _upstream(scene, 11), double_sided=double_sided)
    w = want["materials.coeffs"]
    assert np.all(w[:, :2] > 0) and np.all(w[:, 2] < 0)
    _assert_gradients(f"lobes double_sided={double_sided}", got, want, "materials.coeffs")
