"""The front end of the reference's novel-view and depth-optimisation loops (diffrend/torch/projection_layer.py:749-750,
:788-789, :846-879): a depth map lifted to one world-space surfel per pixel,

    # pos_wc = cam_to_world_batched(z_to_pcl_CC_batched(-depth, camera), None, camera)['pos']
    from surf_renderer_amd import depth_to_surfels
    pos_wc = depth_to_surfels(depth, camera)

as [B, N, 3] -- three columns, not the reference's homogeneous four (whose last is exactly 1), so the result feeds
projection_renderer_differentiable_fast, projection_reverse_renderer, projection_renderer_differentiable and
projection_renderer directly.  Forward and backward are HIP kernels (surf_renderer_amd/csrc/srh_surfels.h): fp64
arithmetic, one fp32 store per element, one lane per pixel, no atomics.  Differentiable in depth, and with
camera_grad=True in the camera's eye, at and up (world frame).

One difference by design: the pixel grid is z_to_pcl_CC's (numpy's linspace, rounded once to float32), the one
render_splats_along_ray uses, where the batched reference function builds it with torch.linspace in float32; the two
differ by at most 4 * 2^-24 of the frame's half extent.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import torch

from . import _lib
from ._camera import camera_frame, camera_views, check_camera_grad
from ._layer import (as_float_tensor, f32, fill_grads, gpu_device, grad_buffers, ptr, stream, upstreams,
                     view_grad_buffers)
from ._projection import upload_view

_NAME = "depth_to_surfels"


class _SurfelsFunction(torch.autograd.Function):
    """depth [B, N] fp32 contiguous -> [B, N, 3]; view [B, 12] fp64 gets a gradient when it requires one."""

    @staticmethod
    def forward(ctx, params, view, depth):
        lib = _lib.load()
        out = torch.empty((*depth.shape, 3), dtype=torch.float32, device=depth.device)
        _lib.check(lib.srh_depth_to_surfels_fwd(C.byref(params), view.data_ptr(), depth.data_ptr(), out.data_ptr(),
                                                stream(depth.device)))
        ctx.params = params
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(view, depth)
        return out

    @staticmethod
    def backward(ctx, g_out):
        view, depth = ctx.saved_tensors
        grads = grad_buffers((depth,), ctx.needs_input_grad[2:])
        ups = upstreams((g_out,))
        vgrads, vws = view_grad_buffers(_lib.load(), (view,), ctx.needs_input_grad[1:2], ctx.params.width,
                                        ctx.params.height)

        def launch():
            lib, p, st = _lib.load(), C.byref(ctx.params), stream(depth.device)
            if vws is None:
                _lib.check(lib.srh_depth_to_surfels_bwd(p, view.data_ptr(), depth.data_ptr(), ups[0].data_ptr(),
                                                        grads[0].data_ptr(), st))
            else:
                _lib.check(lib.srh_depth_to_surfels_bwd_view(p, view.data_ptr(), depth.data_ptr(), ups[0].data_ptr(),
                                                             ptr(grads[0]), vgrads[0].data_ptr(), vws.data_ptr(),
                                                             vws.numel(), st))

        fill_grads(grads + vgrads, ups, launch)
        return (None, *vgrads, *grads)


def _validate(depth, camera: Mapping, frame, camera_grad=False):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError)."""
    depth = as_float_tensor("depth", depth, _NAME)
    if frame not in _lib.SURFELS_FRAME:
        raise ValueError(f"{_NAME}: frame = {frame!r}, expected 'world' or 'camera'")
    W, H = camera_frame(_NAME, camera, camera_grad=check_camera_grad(_NAME, camera_grad))
    if depth.dim() < 2 or depth.shape[0] < 1:
        raise ValueError(f"{_NAME}: depth is {list(depth.shape)}, expected [B, N], [B, H, W] or [B, H, W, 1] with B >= 1")
    B = depth.shape[0]
    if tuple(depth.shape) not in ((B, H * W), (B, H, W), (B, H, W, 1)):
        raise ValueError(f"{_NAME}: depth is {list(depth.shape)}, expected [{B}, W x H = {W} x {H} = {W * H}], "
                         f"[{B}, {H}, {W}] or [{B}, {H}, {W}, 1] (one depth per pixel of the frame)")
    # the camera frame does not read eye / at / up: its view table stays detached and the camera gets no gradient
    fovy, focal, view = camera_views(_NAME, camera, B, to_world=True, camera_grad=camera_grad and frame == "world")
    return depth, (B, H, W), view, fovy, focal


def depth_to_surfels(depth, camera: Mapping, frame: str = "world", *, camera_grad: bool = False) -> torch.Tensor:
    """depth [B, N], [B, H, W] or [B, H, W, 1] with N = W H of camera['viewport'], row by row from the top-left pixel,
    positive in front of the camera (the `depth` the projection layers return, the reference's -z; a depth <= 0 is
    clamped to 0: the point is the eye and its gradient exactly 0); camera: eye / at / up [B, 3] or [B, 4] and one shared
    viewport, fovy and focal_length.  Returns the surfels [B, N, 3], float32 on the GPU, in world coordinates or with
    frame='camera' in the camera's; differentiable in depth.  camera_grad=True lets camera['eye'], ['at'] and ['up']
    require grad (they are refused otherwise) and gives them their gradient, in their own shape, dtype and device; values
    and the gradient of depth are bit for bit those of the same call with the camera detached.  frame='camera' does not
    depend on them, so they get none there."""
    depth, (B, H, W), view, fovy, focal = _validate(depth, camera, frame, camera_grad)
    dev = gpu_device(_NAME, (depth,))
    params = _lib.SrhSurfelsParams(n_views=B, width=W, height=H, frame=_lib.SURFELS_FRAME[frame], fovy=fovy,
                                   focal_length=focal)
    return _SurfelsFunction.apply(params, upload_view(view, dev), f32(depth, dev).reshape(B, H * W))
