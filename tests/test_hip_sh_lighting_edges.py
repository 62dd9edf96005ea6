"""The SH9 lighting layer's edges on the GPU: non-finite probe values outside and inside the disc, non-finite and zero
normals, the one-pixel probe, four channels, [B, H, W, 3] normals, leaves of another dtype and device, and the
single-item calls under the reference's names (a probe file, a 2-D M, the two grid functions).  Bounds as in
tests/sh9_checks.py."""
import os

import numpy as np
import pytest
import torch

import sh9_cases as cases
import sh9_oracle as oracle
from conftest import GOLDEN_DIR
from sh9_checks import DEV, check, leaf, projection_truth, run_irradiance, run_projection

pytestmark = pytest.mark.gpu


def fixture(tag):
    return dict(np.load(os.path.join(GOLDEN_DIR, "sh_lighting", "sh1_" + tag + ".npz")))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_a_non_finite_pixel_outside_the_disc_is_not_read(bad):
    c = cases.projection(0)
    inside = oracle.grid(16, 16)["inside"]
    assert not inside[0, 0] and not inside[15, 15] and not inside[0, 15]
    env = np.array(c["envmap"])
    env[:, ~inside] = bad                                                  # every pixel outside, every channel
    clean, got = run_projection(c["envmap"], c["g_L"]), run_projection(env, c["g_L"])
    assert np.array_equal(got["L"], clean["L"])                             # no coefficient changes a bit
    assert np.array_equal(got["grad_envmap"], clean["grad_envmap"]) and (got["grad_envmap"][:, ~inside] == 0).all()


@pytest.mark.parametrize("at", [(8, 8), (5, 6)], ids=["r0", "generic"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_a_non_finite_pixel_inside_the_disc_gives_its_channel_the_oracles_pattern_and_leaves_the_others_bits(at, bad):
    c = cases.projection(0)
    assert oracle.grid(16, 16)["inside"][at]
    env = np.array(c["envmap"])
    env[1, at[0], at[1], 1] = bad                                           # view 1, channel 1
    clean, got = run_projection(c["envmap"], c["g_L"]), run_projection(env, c["g_L"])
    L, _ = oracle.project(env[1])
    assert not np.isfinite(L[1]).any() and np.isfinite(L[[0, 2]]).all()
    if at == (8, 8) and np.isinf(bad):                                      # Inf * 0 where a harmonic is exactly 0
        assert np.isnan(L[1, [1, 3, 4, 5, 7, 8]]).all() and (L[1, [0, 2, 6]] == bad).all()
    for k in range(9):                                                      # NaN, +Inf or -Inf, per coefficient
        assert np.array_equal(got["L"][1, 1, k], np.float32(L[1, k]), equal_nan=True), k
    assert np.array_equal(got["L"][0], clean["L"][0]) and np.array_equal(got["L"][1, [0, 2]], clean["L"][1, [0, 2]])
    assert np.array_equal(got["grad_envmap"], clean["grad_envmap"])         # linear in the probe: it does not see the values


def test_a_non_finite_normal_poisons_its_own_rows_and_its_views_sums():
    c = cases.irradiance(3)                                                 # 257 normals, an M per view
    n = np.array(c["normal"])
    n[1, 100] = np.nan
    n[1, 200, 2] = np.inf
    clean, got = run_irradiance(c["M"], c["normal"], c["g_E"]), run_irradiance(c["M"], n, c["g_E"])
    rows = np.zeros((cases.VIEWS, 257), bool)
    rows[1, [100, 200]] = True
    for key in ("E", "grad_normal"):
        assert np.array_equal(got[key][~rows], clean[key][~rows]), key      # every other row keeps its bits
        assert not np.isfinite(got[key][rows]).all(axis=-1).any(), key
    assert np.isnan(got["E"][1, 100]).all() and np.isnan(got["grad_normal"][1, 100]).all()
    t = oracle.irradiance_view(c["M"][1], n[1], c["g_E"][1])
    assert np.array_equal(np.isnan(got["grad_M"][1]), np.isnan(t["grad_M"]))
    assert np.isnan(got["grad_M"][1][:3]).all() and np.isnan(got["grad_M"][1][3, :3]).all()      # all that hold n
    assert np.isfinite(got["grad_M"][1][3, 3]).all()                        # h_3 h_3 = 1: the sum of the upstream alone
    assert np.array_equal(got["grad_M"][[0, 2]], clean["grad_M"][[0, 2]])   # the other views' sums keep their bits


def test_the_zero_normal_returns_m33_and_the_linear_terms_gradient():
    M = np.array(cases.irradiance(7)["M"][:1])                              # [1, 4, 4, 3], not symmetric
    got = run_irradiance(M, np.zeros((1, 1, 3), np.float32), np.ones((1, 1, 3), np.float32))
    assert np.array_equal(got["E"][0, 0], M[0, 3, 3])
    want = (M[0, :3, 3].astype(np.float64) + M[0, 3, :3]).sum(-1)
    check(got["grad_normal"][0, 0], want, np.abs(M[0, :3, 3]).astype(np.float64).sum(-1) + np.abs(M[0, 3, :3]).sum(-1))
    assert (got["grad_M"][0, :3] == 0).all() and (got["grad_M"][0, 3, :3] == 0).all() and (got["grad_M"][0, 3, 3] == 1).all()


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_the_one_pixel_probe_projects_to_exactly_zero_for_every_channel_count(C):
    env = np.full((2, 1, 1, C), 3.0, np.float32)
    env[1] = np.nan                                                         # its one pixel is outside: not read
    got = run_projection(env, np.ones((2, C, 9), np.float32))
    assert got["L"].shape == (2, C, 9) and (got["L"] == 0).all() and (got["grad_envmap"] == 0).all()


def test_two_channels_and_four_have_the_oracles_values():
    rng = np.random.RandomState(8)
    for C in (2, 4):
        env, g = cases.f32(rng.uniform(0, 2, (1, 9, 11, C))), cases.f32(rng.uniform(-1, 1, (1, C, 9)))
        got = run_projection(env, g)
        L, A = oracle.project(env[0])
        grad, A_g = oracle.project_grad(env[0].shape, g[0])
        check(got["L"][0], L, A, f"L, C = {C}")
        check(got["grad_envmap"][0], grad, A_g, f"grad_envmap, C = {C}")
        M, n, g_E = cases.f32(rng.uniform(-1, 1, (4, 4, C))), cases.f32(rng.standard_normal((1, 70, 3))), cases.f32(rng.uniform(-1, 1, (1, 70, C)))
        got, t = run_irradiance(M, n, g_E), oracle.irradiance_view(M, n[0], g_E[0])
        check(got["E"][0], t["E"], t["A_E"], f"E, C = {C}")
        check(got["grad_M"], t["grad_M"], t["A_M"], f"grad_M, C = {C}")
        check(got["grad_normal"][0], t["grad_normal"], t["A_normal"], f"grad_normal, C = {C}")


def test_a_normal_map_keeps_its_frame_and_equals_the_flat_call():
    from surf_renderer_amd import irradiance_batched
    c = cases.irradiance(7)                                                 # 64 normals = 4 x 16
    flat = run_irradiance(c["M"], c["normal"], c["g_E"])
    tM, tn = leaf(c["M"]), leaf(c["normal"].reshape(3, 4, 16, 3))
    E = irradiance_batched(tM, tn)
    assert E.shape == (3, 4, 16, 3) and E.dtype == torch.float32 and E.device.type == "cuda"
    (E * torch.tensor(c["g_E"].reshape(3, 4, 16, 3), device=DEV)).sum().backward()
    assert np.array_equal(E.detach().cpu().numpy().reshape(3, 64, 3), flat["E"])
    assert tn.grad.shape == tn.shape and np.array_equal(tn.grad.cpu().numpy().reshape(3, 64, 3), flat["grad_normal"])
    assert np.array_equal(tM.grad.cpu().numpy(), flat["grad_M"])


def test_gradients_come_back_in_the_leafs_own_dtype_layout_and_device():
    from surf_renderer_amd import irradiance_batched, radiance_SH9_batched
    c, p = cases.irradiance(7), cases.projection(1)
    want, want_p = run_irradiance(c["M"], c["normal"], c["g_E"]), run_projection(p["envmap"], p["g_L"])
    tM, tn = leaf(c["M"], torch.float64, "cpu"), leaf(c["normal"], torch.float64, "cpu")        # float64 on the CPU
    E = irradiance_batched(tM, tn)
    assert E.device.type == "cuda" and E.dtype == torch.float32
    (E * torch.tensor(np.array(c["g_E"]), device=DEV)).sum().backward()
    for t, key in ((tM, "grad_M"), (tn, "grad_normal")):
        assert t.grad.dtype == torch.float64 and t.grad.device.type == "cpu" and t.grad.shape == t.shape
    assert np.array_equal(tn.grad.numpy(), want["grad_normal"].astype(np.float64))
    assert np.array_equal(tM.grad.numpy().astype(np.float32), want["grad_M"])                   # fp64 sums, rounded there
    env = leaf(p["envmap"], torch.float64, "cpu")
    (radiance_SH9_batched(env) * torch.tensor(np.array(p["g_L"]), device=DEV)).sum().backward()
    assert env.grad.dtype == torch.float64 and env.grad.device.type == "cpu"
    assert np.array_equal(env.grad.numpy(), want_p["grad_envmap"].astype(np.float64))
    env = leaf(np.ascontiguousarray(p["envmap"].transpose(0, 3, 1, 2)))                         # channels first, on the GPU
    (radiance_SH9_batched(env.permute(0, 2, 3, 1)) * torch.tensor(np.array(p["g_L"]), device=DEV)).sum().backward()
    assert env.grad.shape == env.shape and np.array_equal(env.grad.cpu().numpy().transpose(0, 2, 3, 1), want_p["grad_envmap"])
    half = leaf(c["normal"], torch.float16)                                                     # computed on its float32 values
    irradiance_batched(np.array(c["M"]), half).sum().backward()
    assert half.grad.dtype == torch.float16


def test_the_single_item_calls_under_the_references_names(tmp_path):
    from surf_renderer_amd import irradiance, irradiance_polar, radiance_SH9
    # a probe file goes through load_lightprobe and uses the processed array
    raw = cases.lightprobe_bytes()
    path = tmp_path / "probe.float"
    path.write_bytes(raw)
    L = radiance_SH9(str(path))
    assert L.shape == (3, 9) and L.dtype == torch.float32 and L.device.type == "cuda"
    processed = oracle.load_lightprobe_bytes(raw)[1].astype(np.float32)
    check(L.cpu().numpy(), *oracle.project(processed), "probe file")
    # lists and ndarrays; a 2-D M gives [...], a 3-D M [..., C]
    c = cases.irradiance(7)
    M, n = c["M"][0], c["normal"][0].reshape(4, 16, 3)
    t = oracle.irradiance_view(M, c["normal"][0])
    E = irradiance(M, n.tolist())
    assert E.shape == (4, 16, 3)
    check(E.cpu().numpy().reshape(64, 3), t["E"], t["A_E"], "3-D M")
    E0 = irradiance(M[..., 0], n)
    assert E0.shape == (4, 16) and torch.equal(E0, E[..., 0])
    assert irradiance(M, n[0, 0]).shape == (3,) and torch.equal(irradiance(M, n[0, 0]), E[0, 0])
    # irradiance_polar: the directions are made in float64 and taken as float32
    theta, phi = np.linspace(0.1, 3.0, 7), np.linspace(-3.0, 3.0, 7)
    d = torch.stack((torch.cos(torch.tensor(phi)) * torch.sin(torch.tensor(theta)),
                     torch.sin(torch.tensor(phi)) * torch.sin(torch.tensor(theta)), torch.cos(torch.tensor(theta))), -1)
    t = oracle.irradiance_view(M, d.float().numpy())
    check(irradiance_polar(M, theta, phi).cpu().numpy(), t["E"], t["A_E"], "irradiance_polar")


@pytest.mark.parametrize("k", [0, 1], ids=cases.projection_tag)
def test_the_grid_functions_have_the_references_images(k):
    """irrad_Z hands the kernel M and the directions as float32: each factor of a term n_r M_rs n_s is rounded once, at
    most 3 * 2^-24 of the term, before the kernel's own 2^-40 A and the one store."""
    from surf_renderer_amd import irrad_Z, reconstruct_SH9
    z = fixture(cases.projection_tag(k))
    L = z["ref/L"][0]
    for dim in cases.GRID_DIMS:
        g = oracle.grid(*dim)
        n = np.stack((np.cos(g["phi"]) * np.sin(g["theta"]), np.sin(g["phi"]) * np.sin(g["theta"]), np.cos(g["theta"])), -1)
        A = oracle.irradiance_abs(oracle.zonal_abs(L), n)
        got = irrad_Z(L, dim)
        assert got.shape == dim + (3,) and got.dtype == torch.float32 and got.device.type == "cuda"
        want = z["ref/irrad_Z_%dx%d" % dim][0]
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        assert (err <= 2.0 ** -24 * np.abs(want) + (3 * 2.0 ** -24 + 2.0 ** -39) * A).all(), (dim, (err / A).max() * 2 ** 24)
        assert not g["inside"].all()                                        # unmasked: pixels with r > 1 are evaluated too
        rec = reconstruct_SH9(torch.tensor(L, device=DEV), dim)             # float64 torch on L's device
        assert rec.device.type == "cuda" and rec.dtype == torch.float64
        A = np.sum(np.abs(L)[None, None] * np.abs(g["Y"])[..., None, :] * np.abs(g["domega"])[..., None, None], -1)
        assert (np.abs(rec.cpu().numpy() - z["ref/reconstruct_%dx%d" % dim][0]) <= 2.0 ** -48 * A).all()


def test_radiance_sh9_of_the_recorded_probes_is_the_references_with_the_swapped_axes():
    from surf_renderer_amd import radiance_SH9
    c, T, z = cases.projection(1), projection_truth(1), fixture(cases.projection_tag(1))        # 12 x 20
    L = radiance_SH9(np.array(c["envmap"][0])).cpu().numpy()
    check(L, z["ref/L"][0], T[0]["A_L"], "12 x 20")
    # scaled the other way round the coefficients are others by far more than the bound
    other = oracle.project(np.ascontiguousarray(c["envmap"][0].transpose(1, 0, 2)).astype(np.float64))[0]
    assert np.abs(other - z["ref/L"][0]).max() > 1e-2
