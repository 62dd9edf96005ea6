"""The seven geometric regularisers the reference's trainers put on every rendered splat view (diffrend/torch/GAN/
gan.py:601-640 and the three other callers of render_splats_along_ray), for a whole batch in one forward pass and one
backward launch.

    from surf_renderer_amd import render_splats_along_ray_batch, splat_regularizers, REGULARIZER_TERMS
    res = render_splats_along_ray_batch(scene, samples=K)
    terms = splat_regularizers(res, z_min, z_max, z_scale=2.0, unit_normal_scale=10.0)
    loss = sum(w[k] * terms[k].sum() for k in w)

Forward and backward are HIP kernels (srh_regularizers_fwd / srh_regularizers_bwd, surf_renderer_amd/csrc/
srh_regularizers.h): fp64 arithmetic, fp32 results, no atomics, so values and gradients are identical from run to run.
Differentiable in pos, normal, image and depth.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping

import torch

from . import _lib
from ._layer import as_float_tensor, fill_grads, f32, gpu_device, grad_buffers, ptr, scratch, stream, upstreams

REGULARIZER_TERMS = ("z", "unit_normal", "normal_consistency", "spatial", "spatial_var", "image_depth_consistency",
                     "away_from_camera")
_INPUTS = ("pos", "normal", "image", "depth")


class _RegFunction(torch.autograd.Function):
    """(pos, normal, image, depth), fp32 contiguous with the leading view axis -> terms [B, 7]."""

    @staticmethod
    def forward(ctx, params, pos, normal, image, depth):
        lib = _lib.load()
        B, dev = params.n_views, pos.device
        ws = scratch(lib.srh_regularizers_workspace_bytes(B, params.width, params.height), dev)
        terms = torch.empty((B, _lib.REG_TERMS), dtype=torch.float32, device=dev)
        stats = torch.empty((B, _lib.REG_STATS), dtype=torch.float64, device=dev)
        _lib.check(lib.srh_regularizers_fwd(C.byref(params), pos.data_ptr(), normal.data_ptr(), image.data_ptr(),
                                            depth.data_ptr(), ws.data_ptr(), ws.numel(), terms.data_ptr(),
                                            stats.data_ptr(), stream(dev)))
        ctx.params = params
        ctx.save_for_backward(pos, normal, image, depth, stats)
        return terms

    @staticmethod
    def backward(ctx, g_terms):
        pos, normal, image, depth, stats = ctx.saved_tensors
        grads = grad_buffers((pos, normal, image, depth), ctx.needs_input_grad[1:])
        ups = upstreams((g_terms,))

        def launch():
            _lib.check(_lib.load().srh_regularizers_bwd(
                C.byref(ctx.params), pos.data_ptr(), normal.data_ptr(), image.data_ptr(), depth.data_ptr(),
                stats.data_ptr(), ups[0].data_ptr(), *[ptr(g) for g in grads], stream(pos.device)))

        fill_grads(grads, ups, launch)
        return (None, *grads)


def _validate(res: Mapping, z_min: float, z_max: float):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError); returns
    the four inputs as tensors and whether they carry the view axis."""
    t = {k: as_float_tensor(f"res['{k}']", res[k] if k in res else None, "splat_regularizers") for k in _INPUTS}
    shape = tuple(t["image"].shape)
    if len(shape) not in (3, 4) or shape[-1] != 3:
        raise ValueError(f"splat_regularizers: res['image'] is {list(shape)}, expected [B, H, W, 3] or [H, W, 3]")
    for k in ("pos", "normal"):
        if tuple(t[k].shape) != shape:
            raise ValueError(f"splat_regularizers: res['{k}'] is {list(t[k].shape)}, res['image'] is {list(shape)}")
    if tuple(t["depth"].shape) != shape[:-1]:
        raise ValueError(f"splat_regularizers: res['depth'] is {list(t['depth'].shape)}, expected {list(shape[:-1])}")
    H, W = shape[-3], shape[-2]
    if H < 2 or W < 2:
        raise ValueError(f"splat_regularizers: a {H} x {W} grid cannot be reflection-padded (at least 2 x 2)")
    if len(shape) == 4 and shape[0] < 1:
        raise ValueError("splat_regularizers: an empty batch")
    if not float(z_min) <= float(z_max):
        raise ValueError(f"splat_regularizers: z_min = {z_min} > z_max = {z_max}")
    return t, len(shape) == 4


def splat_regularizers(res: Mapping, z_min: float, z_max: float, z_scale: float = 2.0,
                       unit_normal_scale: float = 10.0) -> Dict[str, torch.Tensor]:
    """The trainers' seven regularisers of rendered splat views.  `res`: any mapping with 'pos', 'normal', 'image'
    [B, H, W, 3] and 'depth' [B, H, W] -- what render_splats_along_ray_batch and render_views(aux=True) return -- or
    without the leading B for one view.  Returns {name: float32 tensor [B] (0-dim for one view)} for the names in
    REGULARIZER_TERMS, differentiable in the four inputs; `away_from_camera` is a sum over the pixels, `spatial_var`
    1 / (variance + 1e-4), the others means.  z_scale is the trainers' 2 (test_optimization.py: 10),
    unit_normal_scale their 10."""
    t, batched = _validate(res, z_min, z_max)
    dev = gpu_device("splat_regularizers", t.values())
    x = [f32(t[k], dev) for k in _INPUTS]
    if not batched:
        x = [v.unsqueeze(0) for v in x]
    B, H, W = x[3].shape
    params = _lib.SrhRegularizerParams(n_views=B, width=W, height=H, z_min=float(z_min), z_max=float(z_max),
                                       z_scale=float(z_scale), unit_normal_scale=float(unit_normal_scale))
    terms = _RegFunction.apply(params, *x)
    return {name: (terms[:, k] if batched else terms[0, k]) for k, name in enumerate(REGULARIZER_TERMS)}
