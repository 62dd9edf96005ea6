"""The reference's hard scatter-mean projection (diffrend/torch/projection_layer.py:88-106) under its own name, so the
swap is one import:

    # from diffrend.torch.projection_layer import projection_renderer
    from surf_renderer_amd import projection_renderer
    rgb_out, mask = projection_renderer(surfels, rgb, camera)

Every surfel lands on the pixel nearest to its projection, and a pixel gets the mean of the values that land on it.
NOTE the mask's sense: it is a bool tensor that is True WHERE NO SURFEL LANDED, as in the reference -- the opposite of
the soft coverage masks of projection_renderer_differentiable_fast, projection_reverse_renderer and
projection_renderer_differentiable.  The reference scatters with float atomics; here the forward is a gather
(surf_renderer_amd/csrc/srh_hard_projection.h): fp64 sums in ascending surfel index, fp32 results, every element
written once, so values and gradients are identical from run to run.  Differentiable in rgb only: the pixel a surfel
lands on is piecewise constant, so surfels get no gradient (None), as autograd through the reference leaves it.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Tuple

import torch

from . import _lib
from ._camera import camera_frame, camera_views
from ._layer import as_float_tensor, fill_grads, gpu_device, stream, upstreams
from ._projection import check_channels, flat, sorted_order, upload_view

_NAME = "projection_renderer"


class _HardFunction(torch.autograd.Function):
    """(surfels [B, N, 3], rgb [B, N, D]), fp32 contiguous -> out [B, N, D], mask [B, N] bool, count [B, N] int32."""

    @staticmethod
    def forward(ctx, params, view, surfels, rgb):
        lib = _lib.load()
        B, N, D = rgb.shape
        dev = rgb.device
        keys = torch.empty((B, N), dtype=torch.int32, device=dev)
        _lib.check(lib.srh_hard_projection_keys(C.byref(params), view.data_ptr(), surfels.data_ptr(), keys.data_ptr(),
                                                stream(dev)))
        order = sorted_order(keys)
        out = torch.empty_like(rgb)
        mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
        count = torch.empty((B, N), dtype=torch.int32, device=dev)
        _lib.check(lib.srh_hard_projection_fwd(C.byref(params), rgb.data_ptr(), keys.data_ptr(), order.data_ptr(),
                                               out.data_ptr(), mask.data_ptr(), count.data_ptr(), stream(dev)))
        mask = mask.view(torch.bool)
        ctx.params = params
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(mask, count)
        ctx.save_for_backward(keys, count)
        return out, mask, count

    @staticmethod
    def backward(ctx, g_out, g_mask, g_count):
        keys, count = ctx.saved_tensors
        # rgb itself is not kept: its gradient has the shape of out, [B, N, D] fp32
        grads = [torch.empty((*keys.shape, ctx.params.channels), dtype=torch.float32, device=keys.device)
                 if ctx.needs_input_grad[3] else None]
        ups = upstreams((g_out,))

        def launch():
            _lib.check(_lib.load().srh_hard_projection_bwd(C.byref(ctx.params), keys.data_ptr(), count.data_ptr(),
                                                           ups[0].data_ptr(), grads[0].data_ptr(), stream(keys.device)))

        fill_grads(grads, ups, launch)
        return (None, None, None, *grads)


def _validate(surfels, rgb, camera: Mapping):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError)."""
    surfels, rgb = as_float_tensor("surfels", surfels, _NAME), as_float_tensor("rgb", rgb, _NAME)
    W, H = camera_frame(_NAME, camera)
    if surfels.dim() != 3 or surfels.shape[-1] != 3:
        raise ValueError(f"{_NAME}: surfels is {list(surfels.shape)}, expected [B, N, 3]")
    B, N = surfels.shape[:2]
    if B < 1:
        raise ValueError(f"{_NAME}: an empty batch")
    if N != W * H:
        raise ValueError(f"{_NAME}: {N} surfels per view, expected W x H = {W} x {H} = {W * H} (one per pixel of the "
                         "frame, as the reference's scatter needs)")
    D = rgb.shape[-1] if rgb.dim() else 0
    if tuple(rgb.shape) not in ((B, N, D), (B, H, W, D)):
        raise ValueError(f"{_NAME}: rgb is {list(rgb.shape)}, expected [{B}, {N}, D] or [{B}, {H}, {W}, D]")
    check_channels(_NAME, rgb)
    fovy, focal, view = camera_views(_NAME, camera, B)
    return surfels, rgb, (B, H, W, D), view, fovy, focal


def projection_renderer(surfels, rgb, camera: Mapping) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's call.  surfels [B, N, 3] in world coordinates with N = W H; rgb [B, N, D] or [B, H, W, D], D in
    1..4; camera: eye / at / up [B, 3] or [B, 4] and one shared viewport, fovy and focal_length.  Returns (rgb_out,
    mask), both in rgb's layout on the GPU: rgb_out float32, the mean of the values that land on each pixel (0 where
    none does), differentiable in rgb; mask bool, True where NO surfel landed, not differentiable."""
    surfels, rgb, (B, H, W, D), view, fovy, focal = _validate(surfels, rgb, camera)
    dev = gpu_device(_NAME, (surfels, rgb))
    pos, val = flat((surfels.detach(), rgb), B, H * W, dev)
    params = _lib.SrhHardProjectionParams(n_views=B, width=W, height=H, channels=D, fovy=fovy, focal_length=focal)
    out, mask, _ = _HardFunction.apply(params, upload_view(view, dev), pos, val)
    return out.reshape(rgb.shape), mask[..., None].expand(B, H * W, D).reshape(rgb.shape)
