"""The reference's backward-warp ("pull") re-projection (diffrend/torch/projection_layer.py:281-333) under its own name,
so the swap is one import:

    # from diffrend.torch.projection_layer import projection_reverse_renderer
    from surf_renderer_amd import projection_reverse_renderer
    out, proj_out = projection_reverse_renderer(rgb, in_pos_wc, out_pos_wc, camera1, camera2, rotated_image=None)

The surfels of the target view (out_pos_wc) are projected into the source camera (camera1), and the source image rgb
is sampled there bilinearly.  Pixels that leave the frame, or that a nearer surface of the source view (in_pos_wc, seen
by camera2) hides, are masked out, and rotated_image fills the holes.  Forward and backward are HIP kernels
(surf_renderer_amd/csrc/srh_reverse_projection.h): fp64 arithmetic, fp32 results, no float atomics, so values and
gradients are identical from run to run.  Differentiable in rgb, rotated_image, out_pos_wc (through the sample
coordinates) and in_pos_wc (through the values of the new depth), and with camera_grad=True in both cameras' eye, at
and up; the mask is not differentiable.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Mapping, Tuple

import torch

from . import _lib
from ._camera import camera_frame, camera_views, check_camera_grad
from ._layer import (as_float_tensor, fill_grads, gpu_device, grad_buffers, ptr, scratch, stream, upstreams,
                     view_grad_buffers)
from ._projection import check_channels, flat, rotated_like, shaped_like, sorted_order, upload_view

_NAME = "projection_reverse_renderer"


class _ReverseFunction(torch.autograd.Function):
    """(rgb [B, N, D], in_pos, out_pos [B, N, 3], rotated [B, N, D] or None), fp32 contiguous -> out (None without a
    rotated image: the result is image1), mask, image1, depth."""

    @staticmethod
    def forward(ctx, params, view1, view2, keep, want_depth, rgb, in_pos, out_pos, rotated):
        lib = _lib.load()
        B, N, D = rgb.shape
        dev = rgb.device
        ws = scratch(lib.srh_reverse_projection_workspace_bytes(C.byref(params), _lib.RPROJ_WS_FWD), dev)
        image1 = torch.empty_like(rgb)
        out = torch.empty_like(rgb) if rotated is not None else None
        mask = torch.empty((B, N), dtype=torch.float32, device=dev)
        depth = torch.empty_like(mask) if want_depth else None
        _lib.check(lib.srh_reverse_projection_fwd(
            C.byref(params), view1.data_ptr(), view2.data_ptr(), rgb.data_ptr(), in_pos.data_ptr(), out_pos.data_ptr(),
            ptr(rotated), ptr(keep), ws.data_ptr(), ws.numel(), ptr(out), mask.data_ptr(), image1.data_ptr(),
            ptr(depth), stream(dev)))
        ctx.params = params
        ctx.set_materialize_grads(False)
        # the kernels keep nothing of their own: the backward reads the inputs and the mask
        if any(ctx.needs_input_grad[1:3]) or any(ctx.needs_input_grad[5:]):
            ctx.save_for_backward(view1, view2, rgb, in_pos, out_pos, mask)
        return out, mask, image1, depth

    @staticmethod
    def backward(ctx, g_out, g_mask, g_image1, g_depth):
        view1, view2, rgb, in_pos, out_pos, mask = ctx.saved_tensors
        grads = grad_buffers((rgb, in_pos, out_pos, rgb), ctx.needs_input_grad[5:])
        ups = upstreams((g_out, g_image1, g_depth))
        vgrads, vws = view_grad_buffers(_lib.load(), (view1, view2), ctx.needs_input_grad[1:3], ctx.params.width,
                                        ctx.params.height)

        def launch():
            lib = _lib.load()
            st = stream(rgb.device)
            keys = order = ws = None
            if grads[0] is not None or grads[1] is not None or vgrads[1] is not None:
                # grad rgb, grad in_pos and grad view2 gather over the pixels that sampled each texel: key, order, walk
                ws = scratch(lib.srh_reverse_projection_workspace_bytes(C.byref(ctx.params), _lib.RPROJ_WS_BWD),
                             rgb.device)
                keys = torch.empty(mask.shape, dtype=torch.int32, device=rgb.device)
                _lib.check(lib.srh_reverse_projection_keys(C.byref(ctx.params), view1.data_ptr(), out_pos.data_ptr(),
                                                           ws.data_ptr(), ws.numel(), keys.data_ptr(), st))
                order = sorted_order(keys)
            args = (C.byref(ctx.params), view1.data_ptr(), view2.data_ptr(), rgb.data_ptr(), in_pos.data_ptr(),
                    out_pos.data_ptr(), mask.data_ptr(), ptr(keys), ptr(order), ptr(ws), 0 if ws is None else ws.numel(),
                    *[ptr(u) for u in ups], *[ptr(g) for g in grads])
            if vws is None:
                _lib.check(lib.srh_reverse_projection_bwd(*args, st))
            else:
                _lib.check(lib.srh_reverse_projection_bwd_view(*args, *[ptr(g) for g in vgrads], vws.data_ptr(),
                                                               vws.numel(), st))

        fill_grads(grads + vgrads, ups, launch)
        return (None, *vgrads, None, None, *grads)


def _validate(rgb, in_pos_wc, out_pos_wc, camera1: Mapping, camera2: Mapping, rotated_image, depth_epsilon,
              mask_dropout, camera_grad=False):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError)."""
    rgb = as_float_tensor("rgb", rgb, _NAME)
    pos = {k: as_float_tensor(k, v, _NAME) for k, v in (("in_pos_wc", in_pos_wc), ("out_pos_wc", out_pos_wc))}
    if rgb.dim() != 4:
        raise ValueError(f"{_NAME}: rgb is {list(rgb.shape)}, expected [B, H, W, D]")
    B, H, W, D = rgb.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{_NAME}: rgb is {list(rgb.shape)}: an empty batch or frame")
    check_channels(_NAME, rgb)
    for k, t in pos.items():
        if tuple(t.shape) != (B, H * W, 3):
            raise ValueError(f"{_NAME}: {k} is {list(t.shape)}, expected [{B}, H W = {H * W}, 3]")
    rotated_image = rotated_like(_NAME, rotated_image, rgb)
    cams = []
    for label, camera in (("camera1", camera1), ("camera2", camera2)):
        if camera_frame(_NAME, camera, label, camera_grad) != (W, H):
            raise ValueError(f"{_NAME}: {label}['viewport'] is not the {W} x {H} (W x H) frame of rgb")
        cams.append(camera_views(_NAME, camera, B, label, camera_grad=camera_grad))
    depth_epsilon, mask_dropout = float(depth_epsilon), float(mask_dropout)
    if not math.isfinite(depth_epsilon):
        raise ValueError(f"{_NAME}: depth_epsilon = {depth_epsilon}, expected finite")
    if not 0 <= mask_dropout < 1:
        raise ValueError(f"{_NAME}: mask_dropout = {mask_dropout}, expected 0 <= mask_dropout < 1")
    return rgb, pos["in_pos_wc"], pos["out_pos_wc"], rotated_image, cams, depth_epsilon, mask_dropout


def projection_reverse_renderer(rgb, in_pos_wc, out_pos_wc, camera1: Mapping, camera2: Mapping, rotated_image=None,
                                compute_new_depth: bool = False, depth_epsilon: float = 1e-1, mask_dropout: float = 0,
                                *, camera_grad: bool = False) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The reference's call.  rgb [B, H, W, D], D in 1..4: the source view; in_pos_wc, out_pos_wc [B, H W, 3]: the world
    positions of the source and of the target view's pixels; camera1 the source camera, camera2 the target camera (eye /
    at / up [B, 3] or [B, 4], a viewport of W x H, fovy and focal_length each); rotated_image like rgb or None.  With
    mask_dropout > 0 the mask is multiplied by F.dropout(ones, mask_dropout, training=True), drawn with torch on the
    GPU, so it follows torch.manual_seed.  Returns (out, {'mask': [B, H, W, 1], 'image1': like rgb, and with
    compute_new_depth 'depth': [B, H, W, 1]}), float32 on the GPU; without a rotated image out is image1.
    camera_grad=True lets eye, at and up of both cameras require grad (they are refused otherwise) and gives them their
    gradient, in their own shape, dtype and device: camera1 through the sample coordinates, camera2 through the values of
    the new depth (zero without compute_new_depth); values and the other gradients are bit for bit those of the same call
    with the cameras detached."""
    rgb, in_pos, out_pos, rotated_image, cams, depth_epsilon, mask_dropout = _validate(
        rgb, in_pos_wc, out_pos_wc, camera1, camera2, rotated_image, depth_epsilon, mask_dropout,
        check_camera_grad(_NAME, camera_grad))
    dev = gpu_device(_NAME, (rgb, in_pos, out_pos, rotated_image))
    B, H, W, D = rgb.shape
    x = flat((rgb, in_pos, out_pos, rotated_image), B, H * W, dev)
    (fovy1, focal1, view1), (fovy2, focal2, view2) = cams
    params = _lib.SrhReverseProjectionParams(n_views=B, width=W, height=H, channels=D, fovy1=fovy1, focal_length1=focal1,
                                             fovy2=fovy2, focal_length2=focal2, depth_epsilon=depth_epsilon)
    keep = None
    if mask_dropout > 0:
        keep = torch.nn.functional.dropout(torch.ones((B, H * W), dtype=torch.float32, device=dev), mask_dropout,
                                           training=True)
    out, mask, image1, depth = _ReverseFunction.apply(params, upload_view(view1, dev), upload_view(view2, dev), keep,
                                                      bool(compute_new_depth), *x)
    proj_out = shaped_like(rgb.shape, mask, image1, depth)
    return (proj_out["image1"] if out is None else out.reshape(rgb.shape)), proj_out
