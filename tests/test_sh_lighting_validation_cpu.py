"""The SH9 lighting layer's interface without a GPU: every name is exported and resolves to the module's object, every
refusal is a ValueError that names the layer and the argument before anything reaches the GPU, a valid call gets as far
as the device, and the host-side functions (the harmonics, the zonal matrix, the loader) are the restatement's."""
import numpy as np
import pytest
import torch

import sh9_cases as cases
import sh9_oracle as oracle
import surf_renderer_amd
from surf_renderer_amd import sh_lighting as sh

NAMES = ("radiance_SH9", "radiance_SH9_batched", "RealSH9_ZonalMatrix", "irradiance", "irradiance_batched",
         "irradiance_polar", "irrad_Z", "reconstruct_SH9", "RealSH9_cart", "RealSH9_polar", "load_lightprobe")


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_the_names_are_exported():
    for name in NAMES:
        assert name in surf_renderer_amd.__all__ and getattr(surf_renderer_amd, name) is getattr(sh, name)
        assert name in dir(surf_renderer_amd)


@pytest.mark.parametrize("fn,envmap,shown", [
    ("radiance_SH9", None, "envmap is missing"), ("radiance_SH9", z(4, 4, 3, dtype=torch.int32), "envmap has dtype"),
    ("radiance_SH9", z(4, 4), r"envmap is \[4, 4\], expected \[H, W, C\]"),
    ("radiance_SH9", z(2, 4, 4, 3), r"expected \[H, W, C\]"),
    ("radiance_SH9_batched", z(4, 4, 3), r"envmap is \[4, 4, 3\], expected \[B, H, W, C\]"),
    ("radiance_SH9", z(4, 4, 0), "envmap has 0 channels"), ("radiance_SH9", z(4, 4, 5), "envmap has 5 channels, expected 1..4"),
    ("radiance_SH9_batched", z(0, 4, 4, 3), "0 views"), ("radiance_SH9_batched", torch.empty(65536, 1, 1, 1), "65536 views"),
    ("radiance_SH9", z(0, 4, 3), "envmap is 0 x 4"), ("radiance_SH9", z(4, 0, 3), "envmap is 4 x 0"),
    ("radiance_SH9", torch.empty(1).expand(4097, 4096, 1), r"envmap is 4097 x 4096, expected .*2\^24"),
])
def test_the_projection_refuses(fn, envmap, shown):
    with pytest.raises(ValueError, match=fn + ": .*" + shown):
        getattr(sh, fn)(envmap)


@pytest.mark.parametrize("M,normal,shown", [
    (None, z(2, 5, 3), "M is missing"), (z(4, 4, 3), None, "normal is missing"),
    (z(4, 4, 3, dtype=torch.int64), z(2, 5, 3), "M has dtype"), (z(4, 4, 3), np.zeros((2, 5, 3), np.int32), "normal has dtype"),
    (z(4, 4, 3), z(5, 3), r"normal is \[5, 3\], expected \[B, N, 3\] or \[B, H, W, 3\]"),
    (z(4, 4, 3), z(2, 5, 4), "normal is"), (z(4, 4, 3), z(2, 2, 2, 5, 3), "normal is"),
    (z(4, 4), z(2, 5, 3), r"M is \[4, 4\], expected \[4, 4, C\] or \[B, 4, 4, C\]"),
    (z(3, 4, 3), z(2, 5, 3), "M is"), (z(2, 4, 3, 3), z(2, 5, 3), "M is"),
    (z(3, 4, 4, 3), z(2, 5, 3), "normal has 2 views and M has 3"),
    (z(4, 4, 0), z(2, 5, 3), "M has 0 channels"), (z(4, 4, 5), z(2, 5, 3), "M has 5 channels"),
    (z(4, 4, 3), z(0, 5, 3), "0 views"), (z(4, 4, 3), torch.empty(1).expand(65536, 1, 3), "65536 views"),
    (z(4, 4, 3), z(2, 0, 3), "normal has 0 normals"), (z(4, 4, 3), torch.empty(1).expand(1, 4097, 4096, 3), "16781312 normals"),
])
def test_irradiance_batched_refuses(M, normal, shown):
    with pytest.raises(ValueError, match="irradiance_batched: .*" + shown):
        sh.irradiance_batched(M, normal)


def test_the_single_item_calls_refuse_under_their_own_names():
    with pytest.raises(ValueError, match=r"irradiance: M is \[2, 4, 4, 3\], expected \[4, 4\] or \[4, 4, C\]"):
        sh.irradiance(z(2, 4, 4, 3), z(5, 3))
    with pytest.raises(ValueError, match=r"irradiance: normal is \[5, 2\]"):
        sh.irradiance(z(4, 4), z(5, 2))
    with pytest.raises(ValueError, match="irradiance: M has 5 channels"):
        sh.irradiance(z(4, 4, 5), z(5, 3))
    with pytest.raises(ValueError, match=r"RealSH9_ZonalMatrix: L is \[3, 8\]"):
        sh.RealSH9_ZonalMatrix(z(3, 8))
    with pytest.raises(ValueError, match="RealSH9_ZonalMatrix: L has dtype"):
        sh.RealSH9_ZonalMatrix(z(3, 9, dtype=torch.int32))
    for fn in (sh.irrad_Z, sh.reconstruct_SH9):
        with pytest.raises(ValueError, match=fn.__name__ + ": dim is"):
            fn(z(3, 9), 7)
        with pytest.raises(ValueError, match=fn.__name__ + ": dim is 0 x 4"):
            fn(z(3, 9), (0, 4))
        with pytest.raises(ValueError, match=r"L is \[9\]"):
            fn(z(9), (4, 4))


def test_a_valid_call_gets_as_far_as_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for name, call in (("radiance_SH9", lambda: sh.radiance_SH9(np.zeros((4, 4, 3)))),
                       ("radiance_SH9_batched", lambda: sh.radiance_SH9_batched([[[[0.5]]]])),
                       ("irradiance_batched", lambda: sh.irradiance_batched(z(4, 4, 1), z(2, 3, 4, 3))),
                       ("irradiance", lambda: sh.irradiance(np.zeros((4, 4)), z(7, 3))),
                       ("irradiance", lambda: sh.irrad_Z(z(3, 9), (5, 8)))):
        with pytest.raises(RuntimeError, match=name + ": the hip backend needs a GPU"):
            call()


def test_the_harmonics_and_the_zonal_matrix_are_the_restatements():
    rng = np.random.RandomState(3)
    X, Y, Z = rng.standard_normal((3, 5, 7))
    got = sh.RealSH9_cart(X, torch.tensor(Y), Z.astype(np.float32))
    assert got.dtype == torch.float64 and got.shape == (5, 7, 9)
    assert np.array_equal(got.numpy(), oracle.real_sh9_cart(X, Y, Z.astype(np.float32).astype(np.float64)))
    g = oracle.grid(5, 8)
    # torch's sin and cos against numpy's: a few ulps of values that are at most 1.1
    assert np.abs(sh.RealSH9_polar(g["theta"], g["phi"]).numpy() - g["Y"]).max() <= 2.0 ** -48
    for k in (2, 5):                                         # a shared M's L [C, 9] and per-view [B, C, 9]
        L = np.array(cases.irradiance(k)["L"])
        M = sh.RealSH9_ZonalMatrix(L)
        assert M.dtype == torch.float64 and M.shape == (L.shape[:-2] + (4, 4, L.shape[-2]))
        per_view = lambda f: f(L) if L.ndim == 2 else np.stack([f(x) for x in L])             # noqa: E731
        want, A = per_view(lambda x: oracle.zonal_matrix(x.astype(np.float64))), per_view(oracle.zonal_abs)
        assert (np.abs(M.numpy() - want) <= 2.0 ** -52 * A).all()
        assert np.array_equal(M.numpy(), np.swapaxes(M.numpy(), -3, -2))
    # it is differentiable: the transposed map, with the literals
    L = torch.tensor(cases.irradiance(2)["L"].astype(np.float64), requires_grad=True)
    g_M = torch.tensor(rng.standard_normal((4, 4, L.shape[0])))
    (sh.RealSH9_ZonalMatrix(L) * g_M).sum().backward()
    tL = torch.tensor(L.detach().numpy(), requires_grad=True)
    (oracle.zonal_matrix(tL, torch) * g_M).sum().backward()
    assert np.abs(L.grad.numpy() - tL.grad.numpy()).max() <= 2.0 ** -50 * np.abs(g_M.numpy()).max()


def test_reconstruct_is_the_restatements_and_keeps_the_solid_angle():
    L = np.array(cases.irradiance(2)["L"])
    for dim in cases.GRID_DIMS:
        got = sh.reconstruct_SH9(L, dim)
        assert got.dtype == torch.float64 and got.shape == dim + (L.shape[0],)
        g = oracle.grid(*dim)
        A = np.sum(np.abs(L.astype(np.float64))[None, None] * np.abs(g["Y"])[..., None, :] * np.abs(g["domega"])[..., None, None], -1)
        assert (np.abs(got.numpy() - oracle.reconstruct(L, dim)) <= 2.0 ** -48 * A).all()     # torch's libm, the sum's order
        assert (np.abs(got.numpy()[~g["inside"]]) > 0).any()                                  # unmasked
