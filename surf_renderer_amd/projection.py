"""The reference's surfel re-projection layer (diffrend/torch/projection_layer.py:170-278) under its own name, so the
swap is one import:

    # from diffrend.torch.projection_layer import projection_renderer_differentiable_fast
    from surf_renderer_amd import projection_renderer_differentiable_fast
    out, proj_out = projection_renderer_differentiable_fast(surfels, rgb, camera, rotated_image=None, blur_size=0.15)

A view's surfels (W H world-space points with a D-channel value each) are projected into another camera, spread
bilinearly over four pixels with weighted-blended order-independent transparency, blurred with a Gaussian and
optionally merged with a second image through the soft coverage mask.  Forward and backward are HIP kernels
(surf_renderer_amd/csrc/srh_projection.h), restated as gathers: fp64 arithmetic, fp32 results, no float atomics, so
values and gradients are identical from run to run.  Differentiable in surfels, rgb and rotated_image, and with
camera_grad=True in the camera's eye, at and up.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Mapping, Tuple

import numpy as np
import torch

from . import _layer, _lib
from ._camera import camera_views, check_camera_grad
from ._camera import view_matrices  # noqa: F401  (view_matrices stays importable from here)
from ._layer import fill_grads, gpu_device, grad_buffers, ptr, scratch, stream, upstreams, view_grad_buffers
from ._projection import flat, shaped_like, sorted_order, upload_view, validate_surfels

_NAME = "projection_renderer_differentiable_fast"


def as_float_tensor(name: str, x: Any, caller: str = _NAME) -> torch.Tensor:
    return _layer.as_float_tensor(name, x, caller)


class _ProjFunction(torch.autograd.Function):
    """(surfels [B, N, 3], rgb [B, N, D], rotated [B, N, D] or None), fp32 contiguous -> out, mask, image1, depth."""

    @staticmethod
    def forward(ctx, params, view, want_depth, surfels, rgb, rotated):
        lib = _lib.load()
        B, N, D = rgb.shape
        dev = rgb.device
        ws = scratch(lib.srh_projection_workspace_bytes(C.byref(params), _lib.PROJ_WS_FWD), dev)
        keys = torch.empty((B, N), dtype=torch.int32, device=dev)
        _lib.check(lib.srh_projection_keys(C.byref(params), view.data_ptr(), surfels.data_ptr(), ws.data_ptr(),
                                           ws.numel(), keys.data_ptr(), stream(dev)))
        order = sorted_order(keys)
        # without a backward to come the kernels keep nothing
        saved = None
        if ctx.needs_input_grad[1] or any(ctx.needs_input_grad[3:]):
            saved = scratch(lib.srh_projection_workspace_bytes(C.byref(params), _lib.PROJ_WS_SAVED), dev)
        out, image1 = torch.empty_like(rgb), torch.empty_like(rgb)
        mask = torch.empty((B, N), dtype=torch.float32, device=dev)
        depth = torch.empty_like(mask) if want_depth else None
        _lib.check(lib.srh_projection_fwd(C.byref(params), rgb.data_ptr(), ptr(rotated), keys.data_ptr(),
                                          order.data_ptr(), ws.data_ptr(), ws.numel(), ptr(saved),
                                          0 if saved is None else saved.numel(), out.data_ptr(), mask.data_ptr(),
                                          image1.data_ptr(), ptr(depth), stream(dev)))
        ctx.params = params
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(view, surfels, rgb, rotated, saved)
        return out, mask, image1, depth

    @staticmethod
    def backward(ctx, g_out, g_mask, g_image1, g_depth):
        view, surfels, rgb, rotated, saved = ctx.saved_tensors
        grads = grad_buffers((surfels, rgb, rotated), ctx.needs_input_grad[3:])
        ups = upstreams((g_out, g_mask, g_image1, g_depth))
        vgrads, vws = view_grad_buffers(_lib.load(), (view,), ctx.needs_input_grad[1:2], ctx.params.width,
                                        ctx.params.height)

        def launch():
            lib = _lib.load()
            ws = scratch(lib.srh_projection_workspace_bytes(C.byref(ctx.params), _lib.PROJ_WS_BWD), rgb.device)
            args = (C.byref(ctx.params), view.data_ptr(), surfels.data_ptr(), rgb.data_ptr(), ptr(rotated),
                    saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(), *[ptr(u) for u in ups],
                    *[ptr(g) for g in grads])
            if vws is None:
                _lib.check(lib.srh_projection_bwd(*args, stream(rgb.device)))
            else:
                _lib.check(lib.srh_projection_bwd_view(*args, vgrads[0].data_ptr(), vws.data_ptr(), vws.numel(),
                                                       stream(rgb.device)))

        fill_grads(grads + vgrads, ups, launch)
        return (None, *vgrads, None, *grads)


def blur_taps(blur_size: float, height: int) -> Tuple[int, np.ndarray]:
    """(half-width, taps[|d|]) of the reference's blur: sigma = blur_size * H / 6, half = floor(3 sigma), normalised."""
    sigma = blur_size * height / 6
    half = int(math.floor(sigma * 3))
    k = np.exp(-np.arange(-half, half + 1, dtype=np.float64) ** 2 / (2 * sigma ** 2))
    return half, (k / k.sum())[half:]


def _validate(surfels, rgb, camera: Mapping, rotated_image, blur_size, camera_grad=False):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError).  Returns the
    tensors, (B, H, W, D), the per-view matrices [B, 3, 4] float64 on the host, and the blur's half-width and taps."""
    surfels, rgb, rotated_image, (B, H, W, D), blur_size = validate_surfels(
        _NAME, surfels, rgb, camera, rotated_image, blur_size,
        "one per pixel of the frame, as the reference's scatter needs", camera_grad)
    if math.floor(blur_size * H / 6 * 3) > _lib.PROJ_MAX_BLUR_HALF:
        raise ValueError(f"{_NAME}: blur_size = {blur_size} at H = {H} gives a blur half-width of "
                         f"{math.floor(blur_size * H / 6 * 3)}, at most {_lib.PROJ_MAX_BLUR_HALF}")
    half, taps = blur_taps(blur_size, H)
    fovy, focal, view = camera_views(_NAME, camera, B, camera_grad=camera_grad)
    return surfels, rgb, rotated_image, (B, H, W, D), view, half, taps, fovy, focal


def projection_renderer_differentiable_fast(surfels, rgb, camera: Mapping, rotated_image=None, blur_size: float = 0.15,
                                            use_depth: bool = True, use_center_dist: bool = True,
                                            compute_new_depth: bool = False, blur_rotated_image: bool = True,
                                            detach_mask: bool = False, detach_mask2: bool = False,
                                            detach_depth_merge: bool = False, *,
                                            camera_grad: bool = False) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The reference's call.  surfels [B, N, 3] in world coordinates with N = W H; rgb [B, N, D] or [B, H, W, D], D in
    1..4; rotated_image like rgb or None; camera: eye / at / up [B, 3] or [B, 4] and one shared viewport, fovy and
    focal_length.  Returns (out, {'mask': [..., 1], 'image1': like rgb, and with compute_new_depth 'depth': [..., 1]}),
    float32 on the GPU, differentiable in surfels, rgb and rotated_image through every output.  camera_grad=True lets
    camera['eye'], ['at'] and ['up'] require grad (they are refused otherwise) and gives them their gradient, in their own
    shape, dtype and device; values and the other gradients are bit for bit those of the same call with the camera
    detached."""
    surfels, rgb, rotated_image, (B, H, W, D), view, half, taps, fovy, focal = _validate(
        surfels, rgb, camera, rotated_image, blur_size, check_camera_grad(_NAME, camera_grad))
    dev = gpu_device(_NAME, (surfels, rgb, rotated_image))
    x = flat((surfels, rgb, rotated_image), B, H * W, dev)
    flags = (_lib.PROJ_USE_DEPTH * bool(use_depth) | _lib.PROJ_USE_CENTER_DIST * bool(use_center_dist)
             | _lib.PROJ_BLUR_ROTATED * bool(blur_rotated_image) | _lib.PROJ_DETACH_MASK * bool(detach_mask)
             | _lib.PROJ_DETACH_MASK2 * bool(detach_mask2) | _lib.PROJ_DETACH_DEPTH_MERGE * bool(detach_depth_merge))
    params = _lib.SrhProjectionParams(n_views=B, width=W, height=H, channels=D, flags=flags, blur_half=half, fovy=fovy,
                                      focal_length=focal)
    params.taps[:half + 1] = taps.tolist()
    out, mask, image1, depth = _ProjFunction.apply(params, upload_view(view, dev), bool(compute_new_depth), *x)
    return out.reshape(rgb.shape), shaped_like(rgb.shape, mask, image1, depth)
