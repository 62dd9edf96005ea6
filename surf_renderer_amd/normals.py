"""The reference's constrained plane fit (diffrend/torch/utils.py:886-968) under its own names: a grid of camera-space
points to one unit normal per point with nz > 0, the link between depth_to_surfels and what wants normals,

    # normal = estimate_surface_normals_plane_fit_batched(pos)
    from surf_renderer_amd import depth_to_surfels, estimate_surface_normals_plane_fit_batched
    pos = depth_to_surfels(depth, camera, frame="camera")                   # [B, N, 3]
    normal = estimate_surface_normals_plane_fit_batched(pos, camera)        # [B, N, 3]

Forward and backward are HIP kernels (surf_renderer_amd/csrc/srh_normals.h): fp64 arithmetic, one fp32 store per
element, one lane per point, no atomics, the gradient to all three components of every point.  Differentiable in pos.
frame='world' returns R n with R the camera's lookat basis, the value of the reference's
cam_to_world_batched(None, normal, camera)['normal'], and with camera_grad=True it is differentiable in the camera's eye,
at and up through R, as that reference call is.

Of the reference's dispatcher estimate_surface_normals only method='plane' exists: 'quadric' is None there, and
'avg_normal' (find_average_normal) normalises a sum of cross products that cancels on border pixels, so that its own
float32 and float64 results disagree by thousands of times any tolerance a kernel could be held to.
"""
from __future__ import annotations

from typing import Mapping, Optional

import numpy as np
import torch

from . import _lib
from ._camera import (VIEW_KEYS, _host, camera_entries, camera_vectors, camera_viewport, check_camera_grad,
                      differentiable_vectors, inverse_view_matrices)
from ._layer import (as_float_tensor, f32, fill_grads, gpu_device, grad_buffers, ptr, scratch, stream, upstreams,
                     view_grad_buffers)

_NAME = "estimate_surface_normals_plane_fit_batched"
FRAMES = ("camera", "world")


class _NormalsFunction(torch.autograd.Function):
    """pos [B, H, W, 3] fp32 contiguous, rot [B, 9] fp64 or None -> [B, H, W, 3]; rot gets a gradient when it requires
    one."""

    @staticmethod
    def forward(ctx, rot, pos):
        lib = _lib.load()
        B, H, W = pos.shape[:3]
        out = torch.empty_like(pos)
        _lib.check(lib.srh_normals_fwd(B, W, H, ptr(rot), pos.data_ptr(), out.data_ptr(), stream(pos.device)))
        ctx.rot = None if rot is None else rot.detach()
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(pos)
        return out

    @staticmethod
    def backward(ctx, g_out):
        pos, = ctx.saved_tensors
        B, H, W = pos.shape[:3]
        grads = grad_buffers((pos,), ctx.needs_input_grad[1:])
        ups = upstreams((g_out,))
        lib = _lib.load()
        vgrads, vws = view_grad_buffers(lib, (ctx.rot,), ctx.needs_input_grad[:1], W, H)

        def launch():
            n_bytes = lib.srh_normals_workspace_bytes(B, W, H) if grads[0] is not None else 0
            ws = scratch(n_bytes, pos.device) if n_bytes else None
            args = (B, W, H, ptr(ctx.rot), pos.data_ptr(), ups[0].data_ptr(), ptr(ws), n_bytes, ptr(grads[0]))
            if vws is None:
                _lib.check(lib.srh_normals_bwd(*args, stream(pos.device)))
            else:
                _lib.check(lib.srh_normals_bwd_view(*args, vgrads[0].data_ptr(), vws.data_ptr(), vws.numel(),
                                                    stream(pos.device)))

        fill_grads(grads + vgrads, ups, launch)
        # srh_normals_bwd_view writes [B, 12]: the 3 x 3 gradient row-major, then three zeros
        return (None if vgrads[0] is None else vgrads[0][:, :9], *grads)


def _rotation(name: str, camera: Mapping, B: int, camera_grad: bool = False) -> torch.Tensor:
    """The lookat basis R = [x y z] of every view as [B, 9] float64 on the host; eye / at / up per view ([B, 3] or
    [B, 4]) or shared ([3] or [4]).  With `camera_grad` attached to those of them that require grad (a shared one is
    expanded over the views, so it gets the sum -- widened to float64 on the host BEFORE the expansion, so that the
    views' gradients are added in float64 and the leaf's dtype rounds the sum once, not every view's term)."""
    shared = {k: _host(camera[k]) for k in VIEW_KEYS}
    shared = {k: (np.broadcast_to(v, (B, v.shape[0])) if v.ndim == 1 else v) for k, v in shared.items()}
    cam = camera_vectors(name, shared, B)
    if camera_grad:
        per_view = {k: (camera[k].to(device="cpu", dtype=torch.float64)[None].expand(B, -1)
                        if isinstance(camera[k], torch.Tensor) and camera[k].dim() == 1 else camera[k]) for k in VIEW_KEYS}
        cam = differentiable_vectors(per_view, cam)
    return inverse_view_matrices(cam["eye"], cam["at"], cam["up"])[:, :, :3].reshape(B, 9).contiguous()


def _validate(name: str, pos, camera: Optional[Mapping], frame, camera_grad=None):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError).  Returns
    (pos, (B, H, W), the rotations [B, 9] float64 on the host or None)."""
    pos = as_float_tensor("pos", pos, name)
    if frame not in FRAMES:
        raise ValueError(f"{name}: frame = {frame!r}, expected 'camera' or 'world'")
    if camera is not None:
        camera_entries(name, camera, VIEW_KEYS if frame == "world" else (), camera_grad=camera_grad)
    elif frame == "world":
        raise ValueError(f"{name}: frame = 'world' needs a camera (eye, at, up)")
    if pos.dim() not in (3, 4) or pos.shape[-1] != 3 or pos.shape[0] < 1:
        raise ValueError(f"{name}: pos is {list(pos.shape)}, expected [B, H, W, 3] or [B, N, 3] with B >= 1")
    B = pos.shape[0]
    if pos.dim() == 3:
        if camera is None:
            raise ValueError(f"{name}: pos is [B, N, 3] = {list(pos.shape)}: camera['viewport'] must give the grid W x H")
        camera_entries(name, camera, ("viewport",), camera_grad=camera_grad)
        W, H = camera_viewport(name, camera)
        if pos.shape[1] != W * H:
            raise ValueError(f"{name}: pos is {list(pos.shape)}, expected [{B}, W x H = {W} x {H} = {W * H}, 3] "
                             "(one point per pixel of the frame)")
    else:
        H, W = pos.shape[1:3]
    if H < 2 or W < 2:
        raise ValueError(f"{name}: pos is a grid of H x W = {H} x {W}, but the reflected 3 x 3 stencil needs H >= 2 "
                         "and W >= 2")
    return pos, (B, H, W), (_rotation(name, camera, B, bool(camera_grad)) if frame == "world" else None)


def _fit(name: str, pos, camera: Optional[Mapping], frame, camera_grad=None) -> torch.Tensor:
    pos, (B, H, W), rot = _validate(name, pos, camera, frame, camera_grad)
    dev = gpu_device(name, (pos,))
    out = _NormalsFunction.apply(None if rot is None else rot.to(dev), f32(pos, dev).reshape(B, H, W, 3))
    return out.reshape(pos.shape)


def estimate_surface_normals_plane_fit_batched(pos, camera: Optional[Mapping] = None, frame: str = "camera", *,
                                               camera_grad: bool = False) -> torch.Tensor:
    """pos [B, H, W, 3], or [B, N, 3] with N = W H of camera['viewport'] (what depth_to_surfels returns), row by row:
    camera-space points, H, W >= 2.  Returns the unit normals of the constrained plane fit over the reflected 3 x 3
    stencil in pos's shape, float32 on the GPU, nz > 0; with frame='world' rotated by the lookat basis of camera's eye /
    at / up ([B, 3] or [B, 4] per view, or [3] / [4] shared).  Differentiable in pos.  camera_grad=True lets camera['eye'],
    ['at'] and ['up'] require grad (they are refused otherwise) and gives them their gradient through that rotation, in
    their own shape, dtype and device (a shared one gets the sum over the views); values and the gradient of pos are
    bit for bit those of the same call with the camera detached.  frame='camera' does not read them, so they get none
    there."""
    return _fit(_NAME, pos, camera, frame, check_camera_grad(_NAME, camera_grad))


def estimate_surface_normals_plane_fit(pos, kernel_size=None) -> torch.Tensor:
    """pos [H, W, 3] -> normals [H, W, 3]: the batched layer with B = 1.  kernel_size is accepted and ignored, as in the
    reference."""
    name = "estimate_surface_normals_plane_fit"
    pos = as_float_tensor("pos", pos, name)
    if pos.dim() != 3 or pos.shape[-1] != 3:
        raise ValueError(f"{name}: pos is {list(pos.shape)}, expected [H, W, 3]")
    return _fit(name, pos[None], None, "camera")[0]


def estimate_surface_normals(pos, kernel_size=None, method: str = "plane") -> torch.Tensor:
    """The reference's dispatcher; only method='plane' is built (see the module's text)."""
    if method != "plane":
        raise ValueError(f"estimate_surface_normals: method = {method!r}, expected 'plane' ('quadric' is None in the "
                         "reference and 'avg_normal' is deliberately not built)")
    return estimate_surface_normals_plane_fit(pos, kernel_size)
