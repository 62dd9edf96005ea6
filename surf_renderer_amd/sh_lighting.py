"""Order-2 spherical-harmonic (SH9) environment lighting: the reference's diffrend/numpy/sph.py and its loader
diffrend/utils/lightprobe.py under their own names, so the swap is one import, plus a batched, differentiable form of the
two hot functions:

    # from diffrend.numpy.sph import radiance_SH9, RealSH9_ZonalMatrix, irradiance
    from surf_renderer_amd import radiance_SH9, RealSH9_ZonalMatrix, irradiance
    L = radiance_SH9(envmap)                        # [H, W, C] -> [C, 9]
    E = irradiance(RealSH9_ZonalMatrix(L), normal)  # [..., 3] -> [..., C]

    L = radiance_SH9_batched(envmaps)               # [B, H, W, C] -> [B, C, 9], differentiable in the envmaps
    E = irradiance_batched(RealSH9_ZonalMatrix(L), res['normal'])      # [B, H, W, 3] -> [B, H, W, C]

The kernels (surf_renderer_amd/csrc/srh_sh9.h) compute in fp64 on the float32 inputs and store each element once as
float32; no atomic, so values and gradients are identical from run to run and a batch equals its views.

The reference's quirks are kept: rows are scaled by W and columns by H (visible for H != W), the solid angle uses
numpy's normalised sinc -- sin(pi theta) / (pi theta), not sin(theta) / theta --, RealSH9_ZonalMatrix uses the decimal
literals c1 .. c5, irradiance takes any 4 x 4 M and does not normalise n, the two grid functions are unmasked and
reconstruct_SH9 keeps the solid angle, and load_lightprobe's endian='big' selects '<'.

One deliberate deviation: a pixel outside the probe's disc (r > 1) is NOT READ.  A NaN or Inf there reaches no
coefficient and gets a gradient of exactly 0, where the reference multiplies it by 0 and turns the channel's nine
coefficients into NaN.  Inside the disc values go through plain IEEE arithmetic.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Tuple

import numpy as np
import torch

from . import _lib
from ._layer import as_float_tensor, f32, fill_grads, gpu_device, grad_buffers, ptr, scratch, stream, upstreams

_C1, _C2, _C3, _C4, _C5 = 0.429043, 0.511664, 0.743125, 0.886227, 0.247708


def load_lightprobe(filename, dim=None, endian="big", datatype="f4", flipud=True, clip_lb_thresh=0, normalize=True):
    """The reference's loader (utils/lightprobe.py:4-33), numpy on the host: a raw file of `datatype` values -> (data,
    processed).  Without `dim` a square [w, w, 3] is guessed from the size.  endian='big' selects the dtype prefix '<'
    (the reference's inversion, kept).  The rows are flipped; processed = (data - lo) / (hi - lo) as float64, lo and hi
    the extremes of the values > clip_lb_thresh, clamped at 0 from below."""
    data = np.fromfile(filename, dtype=("<" if endian == "big" else ">") + datatype)
    if dim is None:
        w = int(np.sqrt(data.size / 3))
        dim = (w, w, 3)
    data = data.reshape(dim)
    if flipud:
        data = data[::-1, ...]
    d = data[data > clip_lb_thresh]
    processed = (data - d.min()).astype(np.float64)
    if normalize:
        processed /= (d.max() - d.min())
    processed[processed < 0] = 0
    return data, processed


def _f64(name: str, x, caller: str) -> torch.Tensor:
    return as_float_tensor(name, x, caller).to(torch.float64)


def RealSH9_cart(X, Y, Z) -> torch.Tensor:
    """The nine real harmonics of a direction, [..., 9] float64 in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1),
    (2,0), (2,1), (2,2); elementwise torch on the inputs' device."""
    X, Y, Z = (_f64(k, v, "RealSH9_cart") for k, v in (("X", X), ("Y", Y), ("Z", Z)))
    s1, s3, s5, s15 = (math.sqrt(k / math.pi) for k in (1, 3, 5, 15))
    return torch.stack((1 / 2. * s1 * torch.ones_like(X), 1 / 2. * s3 * Y, 1 / 2. * s3 * Z, 1 / 2. * s3 * X,
                        1 / 2. * s15 * X * Y, 1 / 2. * s15 * Y * Z, 1 / 4. * s5 * (3 * Z ** 2 - 1),
                        1 / 2. * s15 * X * Z, 1 / 4. * s15 * (X ** 2 - Y ** 2)), dim=-1)


def _direction(theta, phi, caller: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    theta, phi = _f64("theta", theta, caller), _f64("phi", phi, caller)
    return torch.cos(phi) * torch.sin(theta), torch.sin(phi) * torch.sin(theta), torch.cos(theta)


def RealSH9_polar(theta, phi) -> torch.Tensor:
    """RealSH9_cart of (cos phi sin theta, sin phi sin theta, cos theta)."""
    return RealSH9_cart(*_direction(theta, phi, "RealSH9_polar"))


def _grid(dim, caller: str):
    """theta, phi and the solid angle of the projection's pixel grid, [H, W] float64 on the host, unmasked."""
    try:
        H, W = (int(k) for k in dim)
    except (TypeError, ValueError):
        raise ValueError(f"{caller}: dim is {dim!r}, expected (H, W)") from None
    if H < 1 or W < 1 or H * W > _lib.SH9_MAX:
        raise ValueError(f"{caller}: dim is {H} x {W}, expected H, W >= 1 and H W <= 2^24")
    i, j = np.mgrid[0:H, 0:W]
    v = (W / 2.0 - i) / (W / 2.0)
    u = (j - H / 2.0) / (H / 2.0)
    theta = np.pi * np.sqrt(u ** 2 + v ** 2)
    domega = (2 * np.pi / W) * (2 * np.pi / H) * np.sinc(theta)
    return torch.from_numpy(theta), torch.from_numpy(np.arctan2(v, u)), torch.from_numpy(domega)


def _channels(name: str, what: str, n: int) -> None:
    if not 1 <= n <= _lib.SH9_MAX_CHANNELS:
        raise ValueError(f"{name}: {what} has {n} channels, expected 1..{_lib.SH9_MAX_CHANNELS}")


def _views(name: str, B: int) -> None:
    if not 1 <= B <= 65535:
        raise ValueError(f"{name}: {B} views, expected 1..65535")


class _ProjectFunction(torch.autograd.Function):
    """envmap [B, H, W, C] fp32 contiguous on the GPU -> L [B, C, 9] fp32."""

    @staticmethod
    def forward(ctx, params, envmap):
        lib = _lib.load()
        dev = envmap.device
        L = torch.empty((params.n_views, params.channels, 9), dtype=torch.float32, device=dev)
        ws = scratch(lib.srh_sh9_workspace_bytes(C.byref(params), _lib.SH9_WS_PROJECT), dev)
        _lib.check(lib.srh_sh9_project_fwd(C.byref(params), envmap.data_ptr(), ws.data_ptr(), ws.numel(), L.data_ptr(),
                                           stream(dev)))
        ctx.params, ctx.like = params, envmap
        ctx.set_materialize_grads(False)
        return L

    @staticmethod
    def backward(ctx, g_L):
        grads = grad_buffers((ctx.like,), ctx.needs_input_grad[1:2])
        ups = upstreams((g_L,))
        fill_grads(grads, ups, lambda: _lib.check(_lib.load().srh_sh9_project_bwd(
            C.byref(ctx.params), ups[0].data_ptr(), grads[0].data_ptr(), stream(ctx.like.device))))
        return (None, *grads)


def _project(name: str, envmap, batched: bool) -> torch.Tensor:
    envmap = as_float_tensor("envmap", envmap, name)
    rank, form = (4, "[B, H, W, C]") if batched else (3, "[H, W, C]")
    if envmap.dim() != rank:
        raise ValueError(f"{name}: envmap is {list(envmap.shape)}, expected {form}")
    B = envmap.shape[0] if batched else 1
    H, W, Cn = envmap.shape[-3:]
    _views(name, B)
    if H < 1 or W < 1 or H * W > _lib.SH9_MAX:
        raise ValueError(f"{name}: envmap is {H} x {W}, expected H, W >= 1 and H W <= 2^24")
    _channels(name, "envmap", Cn)
    dev = gpu_device(name, (envmap,))
    params = _lib.SrhSh9Params(n_views=B, height=H, width=W, n_points=0, channels=Cn, m_per_view=0)
    L = _ProjectFunction.apply(params, f32(envmap, dev).reshape(B, H, W, Cn))
    return L if batched else L[0]


def radiance_SH9(envmap) -> torch.Tensor:
    """The reference's call: envmap [H, W, C] (tensor on any device, ndarray or list; C in 1..4, H W <= 2^24), or the path
    of a probe file, which goes through load_lightprobe and uses the processed array -> L [C, 9] float32 on the GPU,
    differentiable in envmap.  A pixel outside the disc is not read (see the module's docstring)."""
    if isinstance(envmap, (str, os.PathLike)):
        envmap = np.ascontiguousarray(load_lightprobe(envmap)[1])
    return _project("radiance_SH9", envmap, False)


def radiance_SH9_batched(envmap) -> torch.Tensor:
    """radiance_SH9 for envmap [B, H, W, C]: L [B, C, 9], each view's bits those of radiance_SH9(envmap[b])."""
    return _project("radiance_SH9_batched", envmap, True)


def _zonal_map() -> torch.Tensor:
    """T [16, 9]: M.reshape(16) = T L, the reference's Eq. 12 with its literals."""
    T = torch.zeros((4, 4, 9), dtype=torch.float64)
    for (r, s), (k, w) in {(0, 0): (8, _C1), (0, 1): (4, _C1), (0, 2): (7, _C1), (0, 3): (3, _C2), (1, 1): (8, -_C1),
                           (1, 2): (5, _C1), (1, 3): (1, _C2), (2, 2): (6, _C3), (2, 3): (2, _C2)}.items():
        T[r, s, k] = T[s, r, k] = w
    T[3, 3, 0], T[3, 3, 6] = _C4, -_C5
    return T.reshape(16, 9)


def RealSH9_ZonalMatrix(L) -> torch.Tensor:
    """Eq. 12 of Ramamoorthi and Hanrahan with the reference's decimal literals: L [C, 9] -> M [4, 4, C], and
    [B, C, 9] -> [B, 4, 4, C].  A nine-to-sixteen linear map in torch ops, float64 on L's device, so autograd
    differentiates it and a chain L -> M -> irradiance_batched sums unrounded gradients."""
    name = "RealSH9_ZonalMatrix"
    L = as_float_tensor("L", L, name)
    if L.dim() not in (2, 3) or L.shape[-1] != 9:
        raise ValueError(f"{name}: L is {list(L.shape)}, expected [C, 9] or [B, C, 9]")
    M = L.to(torch.float64) @ _zonal_map().to(L.device).T                  # [..., C, 16]
    return M.reshape(*L.shape[:-1], 4, 4).movedim(-3, -1)


class _IrradianceFunction(torch.autograd.Function):
    """(M of any floating dtype and device, [B, 4, 4, C] or [4, 4, C]; normal [B, N, 3] fp32 contiguous on the GPU) ->
    E [B, N, C] fp32.  M is converted here, not by the caller, so that its gradient leaves the kernels' fp64 sums for
    M's own dtype in one rounding: a float64 M (RealSH9_ZonalMatrix's) hands its chain unrounded values."""

    @staticmethod
    def forward(ctx, params, M, normal):
        lib = _lib.load()
        dev = normal.device
        M32 = f32(M.detach(), dev)
        E = torch.empty((params.n_views, params.n_points, params.channels), dtype=torch.float32, device=dev)
        _lib.check(lib.srh_sh9_irradiance_fwd(C.byref(params), M32.data_ptr(), normal.data_ptr(), E.data_ptr(),
                                              stream(dev)))
        ctx.params, ctx.m_like = params, (M.dtype, M.device)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(M32, normal)
        return E

    @staticmethod
    def backward(ctx, g_E):
        M32, normal = ctx.saved_tensors
        need_M, need_n = ctx.needs_input_grad[1:3]
        dev = normal.device
        grad_M = torch.empty(M32.shape, dtype=torch.float64, device=dev) if need_M else None
        grad_n, = grad_buffers((normal,), (need_n,))
        ups = upstreams((g_E,))

        def launch():
            lib = _lib.load()
            ws = scratch(lib.srh_sh9_workspace_bytes(C.byref(ctx.params), _lib.SH9_WS_IRRADIANCE_BWD), dev) if need_M else None
            _lib.check(lib.srh_sh9_irradiance_bwd(C.byref(ctx.params), M32.data_ptr(), normal.data_ptr(),
                                                  ups[0].data_ptr(), ptr(grad_n), ptr(grad_M), ptr(ws),
                                                  0 if ws is None else ws.numel(), stream(dev)))

        fill_grads((grad_M, grad_n), ups, launch)
        if grad_M is not None:
            grad_M = grad_M.to(device=ctx.m_like[1], dtype=ctx.m_like[0])
        return None, grad_M, grad_n


def _irradiance_batched(name: str, M, normal) -> torch.Tensor:
    M, normal = as_float_tensor("M", M, name), as_float_tensor("normal", normal, name)
    if normal.dim() not in (3, 4) or normal.shape[-1] != 3:
        raise ValueError(f"{name}: normal is {list(normal.shape)}, expected [B, N, 3] or [B, H, W, 3]")
    if M.dim() not in (3, 4) or M.shape[-3:-1] != (4, 4):
        raise ValueError(f"{name}: M is {list(M.shape)}, expected [4, 4, C] or [B, 4, 4, C]")
    B, N, Cn = normal.shape[0], math.prod(normal.shape[1:-1]), M.shape[-1]
    _views(name, B)
    if M.dim() == 4 and M.shape[0] != B:
        raise ValueError(f"{name}: normal has {B} views and M has {M.shape[0]}")
    if not 1 <= N <= _lib.SH9_MAX:
        raise ValueError(f"{name}: normal has {N} normals per view, expected 1..2^24")
    _channels(name, "M", Cn)
    dev = gpu_device(name, (normal, M))
    params = _lib.SrhSh9Params(n_views=B, height=0, width=0, n_points=N, channels=Cn, m_per_view=int(M.dim() == 4))
    E = _IrradianceFunction.apply(params, M, f32(normal, dev).reshape(B, N, 3))
    return E.reshape(*normal.shape[:-1], Cn)


def irradiance_batched(M, normal) -> torch.Tensor:
    """E_c = [n, 1]^T M_c [n, 1] for B views in one call.  normal [B, N, 3] or [B, H, W, 3]; M [4, 4, C], shared by the
    views, or [B, 4, 4, C]; C in 1..4, N or H W in 1..2^24, any floating dtype and device.  Returns [B, N, C] or
    [B, H, W, C] float32 on the GPU, differentiable in normal and in M -- and so in L through RealSH9_ZonalMatrix;
    gradients come back in each leaf's own dtype, layout and device, a shared M's as the views' sums added in ascending
    view order.  Any M, symmetric or not; n is not normalised.  A non-finite normal poisons its own row of E and of
    normal's gradient, and the sums of M's gradient for its view."""
    return _irradiance_batched("irradiance_batched", M, normal)


def irradiance(M, normal) -> torch.Tensor:
    """The reference's call: M [4, 4] or [4, 4, C], normal [..., 3] -> [...] or [..., C] float32 on the GPU."""
    name = "irradiance"
    M, normal = as_float_tensor("M", M, name), as_float_tensor("normal", normal, name)
    if M.dim() not in (2, 3) or M.shape[:2] != (4, 4):
        raise ValueError(f"{name}: M is {list(M.shape)}, expected [4, 4] or [4, 4, C]")
    if normal.dim() < 1 or normal.shape[-1] != 3:
        raise ValueError(f"{name}: normal is {list(normal.shape)}, expected [..., 3]")
    E = _irradiance_batched(name, M if M.dim() == 3 else M[..., None], normal.reshape(1, -1, 3))
    E = E.reshape(*normal.shape[:-1], E.shape[-1])
    return E if M.dim() == 3 else E[..., 0]


def irradiance_polar(M, theta, phi) -> torch.Tensor:
    """irradiance of the directions (cos phi sin theta, sin phi sin theta, cos theta); theta and phi of one shape."""
    return irradiance(M, torch.stack(_direction(theta, phi, "irradiance_polar"), dim=-1))


def irrad_Z(L, dim) -> torch.Tensor:
    """The irradiance image of L [C, 9] over the projection's (H, W) pixel grid, unmasked: [H, W, C] float32."""
    theta, phi, _ = _grid(dim, "irrad_Z")
    L = as_float_tensor("L", L, "irrad_Z")
    if L.dim() != 2:
        raise ValueError(f"irrad_Z: L is {list(L.shape)}, expected [C, 9]")
    return irradiance_polar(RealSH9_ZonalMatrix(L), theta, phi)


def reconstruct_SH9(L, dim) -> torch.Tensor:
    """sum_k L[c][k] Y_k domega over the projection's (H, W) pixel grid, unmasked, the solid angle kept as the reference
    keeps it: [H, W, C] float64 on L's device."""
    name = "reconstruct_SH9"
    theta, phi, domega = _grid(dim, name)
    L = as_float_tensor("L", L, name)
    if L.dim() != 2 or L.shape[-1] != 9:
        raise ValueError(f"{name}: L is {list(L.shape)}, expected [C, 9]")
    Y = RealSH9_polar(theta, phi).to(L.device)
    return torch.sum(L.to(torch.float64)[None, None] * Y[..., None, :] * domega.to(L.device)[..., None, None], dim=-1)
