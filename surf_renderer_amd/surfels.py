"""The front end of the reference's novel-view and depth-optimisation loops (diffrend/torch/projection_layer.py:749-750,
:788-789, :846-879): a depth map lifted to one world-space surfel per pixel,

    # pos_wc = cam_to_world_batched(z_to_pcl_CC_batched(-depth, camera), None, camera)['pos']
    from surf_renderer_amd import depth_to_surfels
    pos_wc = depth_to_surfels(depth, camera)

as [B, N, 3] -- three columns, not the reference's homogeneous four (whose last is exactly 1), so the result feeds
projection_renderer_differentiable_fast, projection_reverse_renderer, projection_renderer_differentiable and
projection_renderer directly.  Forward and backward are HIP kernels (surf_renderer_amd/csrc/srh_surfels.h): fp64
arithmetic, one fp32 store per element, one lane per pixel, no atomics.  Differentiable in depth; the camera is not.

One difference by design: the pixel grid is z_to_pcl_CC's (numpy's linspace, rounded once to float32), the one
render_splats_along_ray uses, where the batched reference function builds it with torch.linspace in float32; the two
differ by at most 4 * 2^-24 of the frame's half extent.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import torch

from . import _lib
from ._camera import camera_frame, camera_views
from ._layer import as_float_tensor, f32, fill_grads, gpu_device, grad_buffers, stream, upstreams
from ._projection import upload_view

_NAME = "depth_to_surfels"


class _SurfelsFunction(torch.autograd.Function):
    """depth [B, N] fp32 contiguous -> [B, N, 3]."""

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

        def launch():
            _lib.check(_lib.load().srh_depth_to_surfels_bwd(C.byref(ctx.params), view.data_ptr(), depth.data_ptr(),
                                                            ups[0].data_ptr(), grads[0].data_ptr(),
                                                            stream(depth.device)))

        fill_grads(grads, ups, launch)
        return (None, None, *grads)


def _validate(depth, camera: Mapping, frame):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError)."""
    depth = as_float_tensor("depth", depth, _NAME)
    if frame not in _lib.SURFELS_FRAME:
        raise ValueError(f"{_NAME}: frame = {frame!r}, expected 'world' or 'camera'")
    W, H = camera_frame(_NAME, camera)
    if depth.dim() < 2 or depth.shape[0] < 1:
        raise ValueError(f"{_NAME}: depth is {list(depth.shape)}, expected [B, N], [B, H, W] or [B, H, W, 1] with B >= 1")
    B = depth.shape[0]
    if tuple(depth.shape) not in ((B, H * W), (B, H, W), (B, H, W, 1)):
        raise ValueError(f"{_NAME}: depth is {list(depth.shape)}, expected [{B}, W x H = {W} x {H} = {W * H}], "
                         f"[{B}, {H}, {W}] or [{B}, {H}, {W}, 1] (one depth per pixel of the frame)")
    fovy, focal, view = camera_views(_NAME, camera, B, to_world=True)
    return depth, (B, H, W), view, fovy, focal


def depth_to_surfels(depth, camera: Mapping, frame: str = "world") -> torch.Tensor:
    """depth [B, N], [B, H, W] or [B, H, W, 1] with N = W H of camera['viewport'], row by row from the top-left pixel,
    positive in front of the camera (the `depth` the projection layers return, the reference's -z; a depth <= 0 is
    clamped to 0: the point is the eye and its gradient exactly 0); camera: eye / at / up [B, 3] or [B, 4] and one shared
    viewport, fovy and focal_length.  Returns the surfels [B, N, 3], float32 on the GPU, in world coordinates or with
    frame='camera' in the camera's; differentiable in depth."""
    depth, (B, H, W), view, fovy, focal = _validate(depth, camera, frame)
    dev = gpu_device(_NAME, (depth,))
    params = _lib.SrhSurfelsParams(n_views=B, width=W, height=H, frame=_lib.SURFELS_FRAME[frame], fovy=fovy,
                                   focal_length=focal)
    return _SurfelsFunction.apply(params, upload_view(view, dev), f32(depth, dev).reshape(B, H * W))
