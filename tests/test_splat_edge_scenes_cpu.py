"""CPU only: every case of tests/splat_edge_scenes.py reaches the branch of csrc/srh_splat.h it is named for.  Asserted
with the fp64 oracle (tests/splat_oracle.py) alone, so that no comparison of tests/test_hip_splats_edges.py can pass for
want of a clamped splat, a clipped pixel or a light with w != 1.

Upstream gradients are uniform in [-1, 1] on all four outputs (splat_edge_scenes.upstream)."""
import numpy as np
import pytest

import splat_oracle
from splat_edge_scenes import CASES, clamped_rows, reference, shininess_rd


def _z(scene):
    pos = np.asarray(scene["objects"]["disk"]["pos"])
    return pos if pos.ndim == 1 else pos[:, 2]


@pytest.mark.parametrize("name", [c for c in CASES if c != "clamped_given_k2"])
def test_oracle_outputs_and_gradients_are_finite(name):
    scene, kw, notes, up, out, grads = reference(name)
    H, W = notes["grid"]
    K = kw.get("samples", 1)
    assert scene["camera"]["viewport"] == [0, 0, W, H]
    assert ("normal" in scene["objects"]["disk"]) == notes["given"]
    assert out["image"].shape == (K * H, K * W, 3) and out["depth"].shape == (K * H, K * W)
    for k in splat_oracle.OUTPUTS:
        assert np.isfinite(out[k]).all(), k
    for k, g in grads.items():
        assert np.isfinite(g).all(), k
        assert np.abs(g).max() > 0, k                         # every leaf takes part
    assert set(up) == set(splat_oracle.OUTPUTS) and all(np.abs(u).max() <= 1 for u in up.values())


@pytest.mark.parametrize("name,K", [("k4_given", 4), ("k4_est", 4), ("k8_given", 8), ("k8_est", 8)])
def test_sample_cases_carry_light_vis_that_matters(name, K):
    scene, kw, notes, up, out, grads = reference(name)
    assert kw["samples"] == K and out["image"].shape == (5 * K, 7 * K, 3)
    vis = scene["objects"]["disk"]["light_vis"]
    assert vis.shape == (2, 35) and 0 < vis.min() < vis.max() <= 1
    # each entry is a sum over the K x K sub-pixels (0 only where a tilted given normal turns away from the light)
    assert (grads["disk.light_vis"] != 0).mean() > 0.9


def test_partial_wave_cases_leave_one_live_lane():
    sizes = {name: int(np.prod(reference(name)[2]["grid"])) for name in ("wave_5x13", "block_1x257", "odd_17x13")}
    assert sizes == {"wave_5x13": 65, "block_1x257": 257, "odd_17x13": 221}
    assert sizes["wave_5x13"] % 64 == 1 and sizes["block_1x257"] % 256 == 1 and 0 < sizes["odd_17x13"] % 64 < 64
    for name in sizes:                                        # both materials among the live lanes and at pixel 0's wave
        m = np.asarray(reference(name)[0]["objects"]["disk"]["material_idx"])
        assert set(np.unique(m)) == {0, 1}, name


def test_clamped_given_normals_oracle_is_non_finite_exactly_on_the_clamped_rows():
    scene, kw, notes, up, out, grads = reference("clamped_given_k2")
    clamped = np.where(_z(scene) >= 0)[0]
    assert kw["samples"] == 2 and np.array_equal(clamped, notes["clamped"]) and clamped.size == 10
    bad = np.where(~np.isfinite(grads["disk.normal"]).all(axis=1))[0]
    assert np.array_equal(bad, clamped)                       # sqrt'(0) * 0 on the depth path of the origin splats
    for k, g in grads.items():
        if k != "disk.normal":
            assert np.isfinite(g).all(), k
    assert np.all(grads["disk.pos"][clamped] == 0)
    assert np.all(grads["disk.pos"][np.setdiff1d(np.arange(99), clamped)] != 0)
    for k in splat_oracle.OUTPUTS:
        assert np.isfinite(out[k]).all(), k
    depth = out["depth"].reshape(9, 2, 11, 2)
    assert np.all(depth[clamped // 11, :, clamped % 11, :] == 0)


def test_clamped_estimated_normals_have_clamped_and_unclamped_neighbours():
    scene, kw, notes, up, out, grads = reference("clamped_est")
    z = _z(scene)
    zero, behind = clamped_rows()
    assert np.all(z[zero] == 0.0) and np.all(z[behind] == 0.75) and zero.size == behind.size == 5
    clamped = z >= 0
    assert clamped.sum() == 10 and np.array_equal(np.where(clamped)[0], notes["clamped"])
    assert np.all(grads["disk.pos"][clamped] == 0) and np.all(grads["disk.pos"][~clamped] != 0)
    assert np.all(out["depth"].reshape(-1)[clamped] == 0)
    grid = clamped.reshape(9, 11)
    n_clamped = []
    for i, j in zip(*np.where(grid)):
        nb = grid[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2]
        n_clamped.append((int(nb.sum()) - 1, nb.size - 1))
    assert any(c == 0 for c, _ in n_clamped)                  # a clamped splat among unclamped ones
    assert any(c > 0 for c, _ in n_clamped)                   # two clamped splats in one stencil: P_k - P_c = 0
    assert all(c < n for c, n in n_clamped)                   # never a stencil without any unclamped splat


def test_negative_colours_clip_a_good_share_of_the_image_away_from_the_threshold():
    scene, kw, notes, up, out, grads = reference("negative_colours")
    assert scene["colors"].min() < 0 and scene["lights"]["ambient"].min() < 0 and kw["samples"] == 2
    im = out["image"]
    share = float((im == 0).mean())
    assert 0.05 <= share <= 0.60, share                       # 43 % with seed 43
    assert np.abs(im[im != 0]).min() > 1e-5                   # 3.3e-4: no entry where fp32 rounding could flip the mask


def test_shininess_0_and_1_see_clipped_and_unclipped_reflections():
    scene, kw, notes, up, out, grads = reference("shininess_0_1")
    np.testing.assert_array_equal(scene["materials"]["coeffs"], np.array([[.8, .2, 0], [.6, .4, 1]], np.float32))
    rd = shininess_rd(scene, kw)                              # (L, H, W), after the relu
    mat = np.asarray(scene["objects"]["disk"]["material_idx"]).reshape(9, 11)
    for m in (0, 1):
        assert (rd[:, mat == m] == 0).any() and (rd[:, mat == m] > 0).any(), m
    # 0 ** 0 = 1: a shininess-0 pixel whose every reflection is clipped still gets cf[1] * colour * albedo from it
    assert np.abs(grads["materials.coeffs"]).min() > 0


@pytest.mark.parametrize("name", ["lights_1", "lights_5"])
def test_lights_with_w_other_than_one_have_a_w_gradient(name):
    scene, kw, notes, up, out, grads = reference(name)
    w = np.asarray(scene["lights"]["pos"])[:, 3]
    assert w.tolist() == notes["w"] and w.size == int(name[-1])
    assert 0.0 in w and (name == "lights_1" or 0.5 in w)
    for l in np.where(w != 1.0)[0]:
        assert grads["lights.pos"][l, 3] != 0, l
    att = np.asarray(scene["lights"]["attenuation"])
    assert len({tuple(a) for a in att}) == w.size             # a different attenuation per light


def test_zpos_cols3_reads_column_two_only():
    scene, kw, notes, up, out, grads = reference("zpos_cols3")
    pos = scene["objects"]["disk"]["pos"]
    assert pos.shape == (30, 3) and np.abs(pos[:, :2]).max() > 5
    assert np.all(grads["disk.pos"][:, :2] == 0) and np.all(grads["disk.pos"][:, 2] != 0)
