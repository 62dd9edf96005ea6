"""The reference's dense Gaussian re-projection (diffrend/torch/projection_layer.py:108-152) under its own name, so the
swap is one import:

    # from diffrend.torch.projection_layer import projection_renderer_differentiable
    from surf_renderer_amd import projection_renderer_differentiable
    out, mask = projection_renderer_differentiable(surfels, rgb, camera, rotated_image=None, blur_size=0.15)

A view's surfels (W H world-space points with a D-channel value each) are projected into another camera, and EVERY
surfel contributes to EVERY pixel with the weight exp(-d^2 / (2 sigma^2)), d the distance between the surfel's pixel
coordinate and the pixel's centre -- surfels outside the frame and behind the camera included.  There is no cell
choice, no floor and no drop at the frame's edge: the layer is smooth in the surfel positions everywhere except Z = 0.
The reference materialises the weights as a [B, W H, N] tensor; here forward and backward are HIP kernels
(surf_renderer_amd/csrc/srh_dense_projection.h) that form the separable weight tile by tile and need memory linear in
B W H: fp64 arithmetic, fp32 results, no atomics, so values and gradients are identical from run to run.
Differentiable in surfels, rgb and rotated_image.  projection_renderer_differentiable_camera is the same layer with the
keyword-only camera_grad of the fast layer: with camera_grad=True it is differentiable in the camera's eye, at and up
too, and since every surfel reaches every pixel that gradient does not vanish when the surfels land outside the frame.
The function under the reference's name keeps the reference's signature and treats the camera as data.

Two things follow the reference to the letter, and one cannot:
  - sigma = blur_size * rgb.shape[-2] / 6: the WIDTH for rgb [B, H, W, D] and the SURFEL COUNT for rgb [B, N, D].  An
    accident of the reference's indexing, but it is the function under this name; the two layouts of one image give
    different results.
  - mask is the plain sum of the weights: not normalised, and well above 1 wherever surfels are dense.
  - with a rotated image the reference's line `sum(...) + rotated_image * (1 - mask)` multiplies [B, N, D] by [B, N] and
    raises for every frame of more than one pixel.  Here the mask is broadcast over the channels, the line's evident
    meaning: out = S + rotated_image * (1 - mask)[..., None].
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Tuple

import torch

from . import _lib
from ._camera import camera_views, check_camera_grad
from ._layer import fill_grads, gpu_device, grad_buffers, ptr, scratch, stream, upstreams, view_grad_buffers
from ._projection import flat, shaped_like, upload_view, validate_surfels

_NAME = "projection_renderer_differentiable"
_NAME_CAMERA = "projection_renderer_differentiable_camera"


class _DenseProjFunction(torch.autograd.Function):
    """(surfels [B, N, 3], rgb [B, N, D], rotated [B, N, D] or None), fp32 contiguous -> out [B, N, D], mask [B, N]; view
    [B, 12] fp64 gets a gradient when it requires one."""

    @staticmethod
    def forward(ctx, params, view, surfels, rgb, rotated):
        lib = _lib.load()
        B, N, D = rgb.shape
        dev = rgb.device
        ws = scratch(lib.srh_dense_projection_workspace_bytes(C.byref(params), _lib.DPROJ_WS_FWD), dev)
        # without a backward to come the kernels keep nothing
        saved = None
        if any(ctx.needs_input_grad[1:]):
            saved = scratch(lib.srh_dense_projection_workspace_bytes(C.byref(params), _lib.DPROJ_WS_SAVED), dev)
        out = torch.empty_like(rgb)
        mask = torch.empty((B, N), dtype=torch.float32, device=dev)
        _lib.check(lib.srh_dense_projection_fwd(C.byref(params), view.data_ptr(), surfels.data_ptr(), rgb.data_ptr(),
                                                ptr(rotated), ws.data_ptr(), ws.numel(), ptr(saved),
                                                0 if saved is None else saved.numel(), out.data_ptr(), mask.data_ptr(),
                                                stream(dev)))
        ctx.params = params
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(view, surfels, rgb, rotated, saved)
        return out, mask

    @staticmethod
    def backward(ctx, g_out, g_mask):
        view, surfels, rgb, rotated, saved = ctx.saved_tensors
        grads = grad_buffers((surfels, rgb, rotated), ctx.needs_input_grad[2:])
        ups = upstreams((g_out, g_mask))
        lib = _lib.load()
        # the surfel kernel runs one wave per workgroup: the partials have this layer's own size
        vgrads, vws = view_grad_buffers(
            lib, (view,), ctx.needs_input_grad[1:2], ctx.params.width, ctx.params.height,
            lambda: lib.srh_dense_projection_workspace_bytes(C.byref(ctx.params), _lib.DPROJ_WS_VIEW))

        def launch():
            ws = scratch(lib.srh_dense_projection_workspace_bytes(C.byref(ctx.params), _lib.DPROJ_WS_BWD), rgb.device)
            args = (C.byref(ctx.params), view.data_ptr(), surfels.data_ptr(), rgb.data_ptr(), ptr(rotated),
                    saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(), *[ptr(u) for u in ups],
                    *[ptr(g) for g in grads])
            if vws is None:
                _lib.check(lib.srh_dense_projection_bwd(*args, stream(rgb.device)))
            else:
                _lib.check(lib.srh_dense_projection_bwd_view(*args, vgrads[0].data_ptr(), vws.data_ptr(), vws.numel(),
                                                             stream(rgb.device)))

        fill_grads(grads + vgrads, ups, launch)
        return (None, *vgrads, *grads)


def _validate(name, surfels, rgb, camera: Mapping, rotated_image, blur_size, camera_grad=None):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError, prefixed
    `name`).  camera_grad: None = the function called has no such keyword.  Returns the tensors, (B, H, W, D), sigma, and
    the camera's fovy, focal length and per-view matrices [B, 3, 4] float64."""
    surfels, rgb, rotated_image, (B, H, W, D), blur_size = validate_surfels(
        name, surfels, rgb, camera, rotated_image, blur_size,
        "one per pixel of the frame: the result is shaped like rgb", camera_grad)
    sigma = blur_size * rgb.shape[-2] / 6          # the reference's rgb.size(-2): W for [B, H, W, D], N for [B, N, D]
    fovy, focal, view = camera_views(name, camera, B, camera_grad=bool(camera_grad))
    return surfels, rgb, rotated_image, (B, H, W, D), sigma, fovy, focal, view


def _project(name, surfels, rgb, camera: Mapping, rotated_image, blur_size, camera_grad=None):
    surfels, rgb, rotated_image, (B, H, W, D), sigma, fovy, focal, view = _validate(
        name, surfels, rgb, camera, rotated_image, blur_size, camera_grad)
    dev = gpu_device(name, (surfels, rgb, rotated_image))
    x = flat((surfels, rgb, rotated_image), B, H * W, dev)
    params = _lib.SrhDenseProjectionParams(n_views=B, width=W, height=H, channels=D,
                                           has_rotated=int(rotated_image is not None), sigma=sigma, fovy=fovy,
                                           focal_length=focal)
    out, mask = _DenseProjFunction.apply(params, upload_view(view, dev), *x)
    return out.reshape(rgb.shape), shaped_like(rgb.shape, mask)["mask"]


def projection_renderer_differentiable(surfels, rgb, camera: Mapping, rotated_image=None,
                                       blur_size: float = 0.15) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's call.  surfels [B, N, 3] in world coordinates with N = W H; rgb [B, N, D] or [B, H, W, D], D in
    1..4; rotated_image like rgb or None; camera: eye / at / up [B, 3] or [B, 4] and one shared viewport, fovy and
    focal_length.  Returns (out like rgb, mask [*rgb.shape[:-1], 1]), float32 on the GPU, differentiable in surfels, rgb
    and rotated_image through both.  The camera is data here: for its gradient call
    projection_renderer_differentiable_camera.

    sigma = blur_size * rgb.shape[-2] / 6 as in the reference: W for [B, H, W, D] input, N for [B, N, D] input.  With
    rotated_image, out = S + rotated_image * (1 - mask) with the mask broadcast over the channels (the reference raises
    there unless B = N = 1); without, out = S / (mask + 1e-10).  See the module docstring."""
    return _project(_NAME, surfels, rgb, camera, rotated_image, blur_size)


def projection_renderer_differentiable_camera(surfels, rgb, camera: Mapping, rotated_image=None, blur_size: float = 0.15,
                                              *, camera_grad: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """projection_renderer_differentiable with the keyword-only camera_grad of projection_renderer_differentiable_fast, so
    that the two can be switched with one flag.  camera_grad=True lets camera['eye'], ['at'] and ['up'] require grad (they
    are refused otherwise) and gives them their gradient, in their own shape, dtype and device; values and the other
    gradients are bit for bit those of projection_renderer_differentiable on the detached camera.  Every surfel
    contributes, so the gradient does not vanish when all of them project outside the frame."""
    return _project(_NAME_CAMERA, surfels, rgb, camera, rotated_image, blur_size,
                    check_camera_grad(_NAME_CAMERA, camera_grad))
