"""CPU only: the scenes of tests/pow_scenes.py reach every branch of the kernels' power functions.  Asserted with the
oracles alone, so that no assertion of tests/test_hip_pow_paths.py can pass for want of pixels on one side of a switch.

The switches (csrc/srh_device.h, csrc/srh_backward.h), for a pixel value x before the tonemap:
  tonemap_f32    hardware path iff gamma > 0 and gamma * log2 x <= 12 (x = 0 included), library powf otherwise
  tonemap_slope  hardware path iff 1e-30 <= x <= 1e30 and |(gamma - 1) * log2 x| <= 12, fp64 library pow otherwise
  spec_pow_f32   as tonemap_slope with (rdotc, n) in place of (x, gamma - 1); rdotc = 0 with n > 0 is 0 directly
"""
import numpy as np
import pytest

from oracle import np_oracle, np_oracle_tch
from pow_scenes import EXPONENTS, GAMMAS, LADDER_NX, LADDER_NY, SWITCH, ladder_scene, lobe_rdotc, lobe_scene, \
    without_tonemap


def _ladder_values(scene, shading):
    """Hit pixels' values before the tonemap, (n, 3), and the result they come from."""
    sc = without_tonemap(scene)
    if shading == "torch":
        res = np_oracle_tch.render(sc)
        hit = res["depth"] <= sc["camera"]["far"]
    else:
        res = np_oracle.render(sc)
        hit = np.isfinite(res["depth"])
    return res["image"][hit], res, hit


@pytest.mark.parametrize("shading", ["numpy", "torch"])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_ladder_reaches_both_sides_of_every_tonemap_switch(gamma, shading):
    x, res, hit = _ladder_values(ladder_scene(gamma, shading=shading), shading)
    assert set(np.unique(res["nearest"][hit])) == set(range(LADDER_NX * LADDER_NY))      # every disc is seen
    assert 0.4 < 1.0 - hit.mean() < 0.5                                                   # and so is the background
    assert (x == 0).sum() == 27                               # disc 0: nine pixels of albedo 0
    pos = x[x > 0]
    y = gamma * np.log2(pos)
    assert (y < -SWITCH).any() and (np.abs(y) <= SWITCH).any() and (y > SWITCH).any()
    assert np.isfinite((pos ** gamma).astype(np.float32)).all()                           # x ** gamma fits fp32
    s = np.abs((gamma - 1.0) * np.log2(pos))
    if gamma == 1.0:
        assert (s <= SWITCH).all()
    else:
        assert (s > SWITCH).any() and (s <= SWITCH).any()
    assert pos.min() < 1e-30                                  # tonemap_slope's range test on x itself


@pytest.mark.parametrize("gamma", GAMMAS)
def test_gradient_ladder_reaches_the_slope_fallback(gamma):
    """The ladder of the backward sweep (lo = -12, hi = min(4, 30 / gamma): gradients of the whole ladder would leave
    fp32).  Its dimmest pixel is 2e-13 = 2 ** -42, so the fallback of tonemap_slope is reached wherever
    |gamma - 1| > 12 / 42: every gamma of the sweep but 0.8 (which needs x < 2 ** -60) and 1.0 (never)."""
    x, _, _ = _ladder_values(ladder_scene(gamma, lo=-12.0, hi=min(4.0, 30.0 / gamma)), "numpy")
    pos = x[x > 0]
    s = np.abs((gamma - 1.0) * np.log2(pos))
    assert (s <= SWITCH).any()
    assert (s > SWITCH).any() == (gamma not in (0.8, 1.0))
    assert (x == 0).sum() == 27


def test_dim_light_ladder_holds_fp32_denormals():
    x, _, _ = _ladder_values(ladder_scene(0.8, light_colour=1e-12), "numpy")
    pos = x[x > 0]
    assert pos.min() < 1e-42 and ((pos < 1.1754944e-38) & (pos.astype(np.float32) > 0)).any()


@pytest.mark.parametrize("gamma,background", [(0.0, 1.0), (-1.0, np.inf)])
def test_oracles_accept_non_positive_gammas(gamma, background):
    for shading, oracle in (("numpy", np_oracle), ("torch", np_oracle_tch)):
        scene = ladder_scene(gamma, shading=shading)
        res = oracle.render(scene)
        hit = (res["depth"] <= scene["camera"]["far"])
        assert (res["image"][~hit] == background).all() and (~hit).any()
        img = res["image"][hit]
        assert not np.isnan(img).any()
        # 0 ** gamma on disc 0's 27 values; x ** 0 = 1 on all the others, 1 / x finite
        assert (img == background).sum() == (img.size if gamma == 0.0 else 27)


@pytest.fixture(scope="module")
def lobes():
    scene = lobe_scene()
    return scene, {ds: np_oracle_tch.render(scene, double_sided=ds) for ds in (False, True)}


@pytest.mark.parametrize("double_sided", [False, True])
def test_lobe_scene_reaches_both_sides_of_the_lobe_switch(lobes, double_sided):
    scene, results = lobes
    res = results[double_sided]
    hit = res["depth"] <= scene["camera"]["far"]
    rdotc = lobe_rdotc(scene, res, double_sided)
    assert len(EXPONENTS) == len(scene["materials"]["coeffs"])
    for m, n in enumerate(EXPONENTS):
        own = hit & (res["nearest"] == m)
        assert own.sum() >= 200, (n, own.sum())
        r = rdotc[:, own]
        assert (r[0] > 1.0 - 1e-6).any(), n                    # the light at the eye, at the sphere's centre pixel
        assert r.min() == 0.0 and r.max() <= 1.0 + 1e-12
        if n > 0:
            edge = 2.0 ** (-SWITCH / n)
            assert (r == 0).any() and ((r > 0) & (r < edge)).any() and ((r >= edge) & (r < 1)).any(), n
            # ... also after the kernel's rounding of the base to fp32
            r32 = r.astype(np.float32)
            assert ((r32 > 0) & (n * np.log2(np.maximum(r32, 1e-45).astype(np.float64)) < -SWITCH)).any(), n
