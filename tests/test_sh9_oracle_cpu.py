"""tests/sh9_oracle.py, the restatement the GPU tests of the SH9 lighting are held to, against the reference's own values
recorded under tests/golden/sh_lighting (tools/gen_sh_lighting_golden.py): every entry within 64 * 2^-53 * A of the
reference's, A the entry's sum of |terms| -- a few roundings and libm calls per term plus the summation -- and the probe
loader bit for bit.  No GPU."""
import os

import numpy as np
import pytest

import sh9_cases as cases
import sh9_oracle as oracle
from conftest import GOLDEN_DIR

TOL = 64 * 2.0 ** -53
P_ALL, I_ALL = range(len(cases.PROJECTION)), range(len(cases.IRRADIANCE))


def fixture(tag):
    return dict(np.load(os.path.join(GOLDEN_DIR, "sh_lighting", "sh1_" + tag + ".npz")))


def close(got, want, A, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, where
    assert (np.abs(got - want) <= TOL * A).all(), (where, (np.abs(got - want) / np.where(A > 0, A, 1)).max())


@pytest.mark.parametrize("k", P_ALL, ids=cases.projection_tag)
def test_the_projection_and_the_zonal_matrix_are_the_references(k):
    c, z = cases.projection(k), fixture(cases.projection_tag(k))
    assert np.array_equal(z["in/envmap"], c["envmap"]) and z["in/envmap"].dtype == np.float32
    for b, env in enumerate(c["envmap"]):
        L, A = oracle.project(env)
        close(L, z["ref/L"][b], A, f"L, view {b}")
        # M of the REFERENCE's L: a product per entry, and one difference in M[3, 3]
        M = oracle.zonal_matrix(z["ref/L"][b])
        close(M, z["ref/M"][b], oracle.zonal_abs(z["ref/L"][b]), f"M, view {b}")


def test_the_one_pixel_probe_has_no_pixel_inside_and_projects_to_zero():
    k = cases.PROJECTION.index((1, 1, 3, 1))
    assert not oracle.grid(1, 1)["inside"].any()
    assert (fixture(cases.projection_tag(k))["ref/L"] == 0).all() and (oracle.project(cases.projection(k)["envmap"][0])[0] == 0).all()


@pytest.mark.parametrize("k", P_ALL, ids=cases.projection_tag)
def test_the_grid_functions_are_the_references(k):
    z = fixture(cases.projection_tag(k))
    for dim in cases.GRID_DIMS:
        g = oracle.grid(*dim)
        for b, L in enumerate(z["ref/L"]):
            n = np.stack((np.cos(g["phi"]) * np.sin(g["theta"]), np.sin(g["phi"]) * np.sin(g["theta"]), np.cos(g["theta"])), -1)
            A = oracle.irradiance_abs(oracle.zonal_abs(L), n)
            close(oracle.irrad_Z(L, dim), z["ref/irrad_Z_%dx%d" % dim][b], A, f"irrad_Z {dim}, view {b}")
            A = np.sum(np.abs(L)[None, None] * np.abs(g["Y"])[..., None, :] * np.abs(g["domega"])[..., None, None], -1)
            close(oracle.reconstruct(L, dim), z["ref/reconstruct_%dx%d" % dim][b], A, f"reconstruct {dim}, view {b}")


@pytest.mark.parametrize("k", I_ALL, ids=cases.irradiance_tag)
def test_the_irradiance_is_the_references(k):
    c, z = cases.irradiance(k), fixture(cases.irradiance_tag(k))
    for key in ("M", "normal", "L"):
        assert np.array_equal(z["in/" + key], c[key]) and z["in/" + key].dtype == np.float32
    for b in range(cases.VIEWS):
        r = oracle.irradiance_view(cases.view_M(c, b), c["normal"][b])
        close(r["E"], z["ref/E"][b], r["A_E"], f"E, view {b}")
    # the zero normal: E = M[3, 3]
    assert np.array_equal(z["ref/E"][-1, -1], cases.view_M(c, cases.VIEWS - 1)[3, 3].astype(np.float64))
    if "ref/M" in z:                                                   # the case's M is the reference's, rounded once
        assert np.array_equal(z["ref/M"].astype(np.float32), c["M"])


def test_the_closed_form_of_the_issue_is_the_quadratic_form():
    c = cases.irradiance(cases.IRRADIANCE.index((257, 4, "zonal", True)))
    L, n = c["L"][0].astype(np.float64), c["normal"][0].astype(np.float64)
    x, y, z = n.T[:, :, None]
    L00, L1m1, L10, L11, L2m2, L2m1, L20, L21, L22 = L.T
    E = (oracle.C4 * L00 - oracle.C5 * L20 + 2 * oracle.C2 * (L11 * x + L1m1 * y + L10 * z) + oracle.C1 * L22 * (x * x - y * y)
         + oracle.C3 * L20 * z * z + 2 * oracle.C1 * (L2m2 * x * y + L21 * x * z + L2m1 * y * z))
    M = oracle.zonal_matrix(L)
    close(oracle.irradiance(M, n), E, oracle.irradiance_abs(M, n), "closed form")


def test_the_gradients_of_the_restatement_are_its_formulas():
    """autograd's gradients against the formulas the kernels implement, written out"""
    c = cases.irradiance(cases.IRRADIANCE.index((64, 3, "random", True)))
    M, n, g = (c[k][1].astype(np.float64) for k in ("M", "normal", "g_E"))
    r = oracle.irradiance_view(M, n, g)
    h = np.concatenate([n, np.ones((len(n), 1))], 1)
    close(r["grad_M"], np.einsum("nc,nr,ns->rsc", g, h, h), r["A_M"], "grad_M")
    sym = M[:3, :3] + M[:3, :3].transpose(1, 0, 2)
    want = np.einsum("nc,rsc,ns->nr", g, sym, n) + g @ (M[:3, 3] + M[3, :3]).T
    close(r["grad_normal"], want, r["A_normal"], "grad_normal")
    p = cases.projection(0)
    grad, A = oracle.project_grad(p["envmap"][0].shape, p["g_L"][0])
    import torch
    gr = oracle.grid(16, 16)
    env = torch.tensor(p["envmap"][0].astype(np.float64), requires_grad=True)
    w = torch.tensor(np.where(gr["inside"][..., None], gr["Y"] * gr["domega"][..., None], 0.0))
    (torch.einsum("ijc,ijk->ck", env, w) * torch.tensor(p["g_L"][0].astype(np.float64))).sum().backward()
    close(env.grad.numpy(), grad, A, "grad_envmap")
    assert (grad[~gr["inside"]] == 0).all()


def test_a_nan_outside_the_disc_reaches_nothing_and_inside_it_poisons_its_channel_only():
    env = cases.projection(0)["envmap"][0].astype(np.float64)
    inside = oracle.grid(16, 16)["inside"]
    assert not inside[0, 0] and inside[8, 8]
    clean = oracle.project(env)[0]
    out = env.copy()
    out[0, 0, 1] = np.nan
    assert np.array_equal(oracle.project(out)[0], clean)               # the deliberate difference from the reference
    hit = env.copy()
    hit[5, 6, 1] = np.inf
    L = oracle.project(hit)[0]
    assert np.array_equal(L[[0, 2]], clean[[0, 2]]) and not np.isfinite(L[1]).any()


def test_load_lightprobe_is_the_references_bit_for_bit(tmp_path):
    from surf_renderer_amd.sh_lighting import load_lightprobe
    z = fixture("lightprobe")
    raw = cases.lightprobe_bytes()
    assert np.array_equal(z["in/bytes"], np.frombuffer(raw, np.uint8))
    path = tmp_path / "probe.float"
    path.write_bytes(raw)
    for k, kw in enumerate(cases.LIGHTPROBE_CALLS):
        for data, processed in (load_lightprobe(str(path), **kw), oracle.load_lightprobe_bytes(raw, **kw)):
            assert data.dtype == z["ref/data_%d" % k].dtype and processed.dtype == np.float64
            assert np.array_equal(data, z["ref/data_%d" % k]) and np.array_equal(processed, z["ref/processed_%d" % k])
    assert (z["ref/processed_0"] == 0).any() and z["ref/processed_0"].max() == 1.0      # the clamp and the range act
    assert np.array_equal(z["ref/data_0"][::-1], z["ref/data_1"])                       # the rows are flipped
    # endian='big' selects '<': on this little-endian file it is the default that reads the values as written
    assert np.array_equal(z["ref/data_1"], np.frombuffer(raw, "<f4").reshape(4, 4, 3))
