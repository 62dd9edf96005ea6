"""The reference's frame transforms and point projection under their own names (diffrend/torch/utils.py:539-647,
diffrend/torch/projection_layer.py:19-85), so the swap is one import:

    # from diffrend.torch.utils import cam_to_world, cam_to_world_batched, world_to_cam, world_to_cam_batched
    # from diffrend.torch.projection_layer import project_surfels, project_image_coordinates
    from surf_renderer_amd import (cam_to_world, cam_to_world_batched, world_to_cam, world_to_cam_batched,
                                   project_surfels, project_image_coordinates)
    res_wc = cam_to_world_batched(res['pos'], res['normal'], camera)

Points and normals of any count N (not tied to a viewport) between the world and a camera's frame, and world points
to the camera's image plane and pixel coordinates.  Forward and backward are HIP kernels
(surf_renderer_amd/csrc/srh_frames.h): fp64 arithmetic, one fp32 store per element, one lane per point, no atomics, so
values and gradients are identical from run to run and a batch equals its views.  Differentiable in the points and
normals, and with camera_grad=True in the camera's eye, at and up.

One difference by design: project_image_coordinates returns px_idx as int64, where the reference returns a float
tensor that every caller passes through .long().
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._camera import (VIEW_KEYS, camera_entries, camera_frame, camera_vectors, camera_views, check_camera_grad,
                      differentiable_vectors, inverse_view_matrices, view_matrices)
from ._layer import (as_float_tensor, f32, fill_grads, gpu_device, grad_buffers, ptr, stream, upstreams,
                     view_grad_buffers_for_points)
from ._projection import upload_view

MAX_VIEWS = 65535
MAX_POINTS = 1 << 24


class _FrameFunction(torch.autograd.Function):
    """(pos [B, n_pos, 3|4], normal [B, n_normal, 3|4]) fp32 contiguous, either None -> (out_pos [B, n_pos, 4],
    out_normal [B, n_normal, 3]); the tables [B, 12] fp64 get a gradient where they require one."""

    @staticmethod
    def forward(ctx, params, view_pos, view_normal, pos, normal):
        lib = _lib.load()
        dev = (pos if pos is not None else normal).device
        out_pos = None if pos is None else torch.empty((*pos.shape[:2], 4), dtype=torch.float32, device=dev)
        out_normal = None if normal is None else torch.empty((*normal.shape[:2], 3), dtype=torch.float32, device=dev)
        _lib.check(lib.srh_frame_transform_fwd(C.byref(params), ptr(view_pos), ptr(view_normal), ptr(pos), ptr(normal),
                                               ptr(out_pos), ptr(out_normal), stream(dev)))
        ctx.params = params
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(view_pos, view_normal, pos, normal)
        return out_pos, out_normal

    @staticmethod
    def backward(ctx, g_pos, g_normal):
        view_pos, view_normal, pos, normal = ctx.saved_tensors
        p = ctx.params
        dev = (pos if pos is not None else normal).device
        grads = grad_buffers((pos, normal), ctx.needs_input_grad[3:5])
        ups = upstreams((g_pos, g_normal))
        vgrads, vws = view_grad_buffers_for_points(_lib.load(), (view_pos, view_normal), ctx.needs_input_grad[1:3],
                                                   max(p.n_pos, p.n_normal), tables=2)

        def launch():
            lib, st = _lib.load(), stream(dev)
            # an output the loss does not read has a zero upstream gradient
            up = [u if u is not None or t is None else torch.zeros((*t.shape[:2], c), dtype=torch.float32, device=dev)
                  for u, t, c in zip(ups, (pos, normal), (4, 3))]
            if vws is None:
                # a half whose gradient nobody wants is left out of the launch
                q = _lib.SrhFrameParams(n_views=p.n_views, n_pos=p.n_pos if grads[0] is not None else 0,
                                        n_normal=p.n_normal if grads[1] is not None else 0, pos_cols=p.pos_cols,
                                        normal_cols=p.normal_cols)
                _lib.check(lib.srh_frame_transform_bwd(C.byref(q), ptr(view_pos), ptr(view_normal), ptr(up[0]),
                                                       ptr(up[1]), ptr(grads[0]), ptr(grads[1]), st))
            else:
                _lib.check(lib.srh_frame_transform_bwd_view(C.byref(p), ptr(view_pos), ptr(view_normal), ptr(pos),
                                                            ptr(normal), ptr(up[0]), ptr(up[1]), ptr(grads[0]),
                                                            ptr(grads[1]), ptr(vgrads[0]), ptr(vgrads[1]),
                                                            vws.data_ptr(), vws.numel(), st))

        fill_grads(grads + vgrads, ups, launch)
        return (None, *vgrads, *grads)


class _ProjectFunction(torch.autograd.Function):
    """surfels [B, N, 3|4] fp32 contiguous -> plane [B, N, 3] (`coords` False) or px_coord [B, N, 3] and px_idx [B, N]
    int32 (`coords` True); view [B, 12] fp64 gets a gradient when it requires one."""

    @staticmethod
    def forward(ctx, params, coords, view, surfels):
        lib = _lib.load()
        B, N = surfels.shape[:2]
        dev = surfels.device
        out = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        idx = torch.empty((B, N), dtype=torch.int32, device=dev) if coords else None
        _lib.check(lib.srh_project_coordinates_fwd(C.byref(params), view.data_ptr(), surfels.data_ptr(),
                                                   None if coords else out.data_ptr(),
                                                   out.data_ptr() if coords else None, ptr(idx), stream(dev)))
        ctx.params, ctx.coords = params, coords
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(view, surfels)
        if idx is not None:
            ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, g_out, g_idx):
        view, surfels = ctx.saved_tensors
        p = ctx.params
        grads = grad_buffers((surfels,), ctx.needs_input_grad[3:])
        ups = upstreams((g_out,))
        vgrads, vws = view_grad_buffers_for_points(_lib.load(), (view,), ctx.needs_input_grad[2:3], p.n_points)

        def launch():
            lib, st = _lib.load(), stream(surfels.device)
            g_plane, g_coord = (None, ups[0].data_ptr()) if ctx.coords else (ups[0].data_ptr(), None)
            if vws is None:
                _lib.check(lib.srh_project_coordinates_bwd(C.byref(p), view.data_ptr(), surfels.data_ptr(), g_plane,
                                                           g_coord, grads[0].data_ptr(), st))
            else:
                _lib.check(lib.srh_project_coordinates_bwd_view(C.byref(p), view.data_ptr(), surfels.data_ptr(), g_plane,
                                                                g_coord, ptr(grads[0]), vgrads[0].data_ptr(),
                                                                vws.data_ptr(), vws.numel(), st))

        fill_grads(grads + vgrads, ups, launch)
        return (None, None, *vgrads, *grads)


def _points(name: str, what: str, x) -> Optional[torch.Tensor]:
    """A [B, N, 3 | 4] point set within the kernels' ranges (ValueError), or None."""
    if x is None:
        return None
    t = as_float_tensor(what, x, name)
    if t.dim() != 3 or t.shape[-1] not in (3, 4):
        raise ValueError(f"{name}: {what} is {list(t.shape)}, expected [B, N, 3] or [B, N, 4]")
    B, N = t.shape[:2]
    if not 1 <= B <= MAX_VIEWS:
        raise ValueError(f"{name}: {what} has {B} views, expected 1..{MAX_VIEWS}")
    if not 1 <= N <= MAX_POINTS:
        raise ValueError(f"{name}: {what} has {N} points per view, expected 1..2^24")
    return t


def _transform(name: str, to_world: bool, pos, normal, camera: Mapping, camera_grad) -> Dict[str, Optional[torch.Tensor]]:
    """Both directions: everything the kernels index by is checked on the host before anything reaches the GPU
    (ValueError), then one launch for both inputs."""
    camera_grad = check_camera_grad(name, camera_grad)
    camera_entries(name, camera, VIEW_KEYS, camera_grad=camera_grad)
    pos, normal = _points(name, "pos", pos), _points(name, "normal", normal)
    if pos is None and normal is None:
        raise ValueError(f"{name}: pos and normal are both None")
    B = (pos if pos is not None else normal).shape[0]
    if pos is not None and normal is not None and normal.shape[0] != B:
        raise ValueError(f"{name}: pos has {B} views, normal has {normal.shape[0]}")
    cam = camera_vectors(name, camera, B)
    if camera_grad:
        cam = differentiable_vectors(camera, cam)
    # the reference pairs each direction's position matrix with the other direction's 3 x 3 for the normals
    tables = (inverse_view_matrices, view_matrices) if to_world else (view_matrices, inverse_view_matrices)
    dev = gpu_device(name, (pos, normal))
    view_pos = None if pos is None else upload_view(tables[0](cam["eye"], cam["at"], cam["up"]), dev)
    view_normal = None if normal is None else upload_view(tables[1](cam["eye"], cam["at"], cam["up"]), dev)
    params = _lib.SrhFrameParams(n_views=B, n_pos=0 if pos is None else pos.shape[1],
                                 n_normal=0 if normal is None else normal.shape[1],
                                 pos_cols=3 if pos is None else pos.shape[2],
                                 normal_cols=3 if normal is None else normal.shape[2])
    out_pos, out_normal = _FrameFunction.apply(params, view_pos, view_normal, None if pos is None else f32(pos, dev),
                                               None if normal is None else f32(normal, dev))
    return {"pos": out_pos, "normal": out_normal}


def _one_view(name: str, pos, normal, camera: Mapping):
    """The unbatched forms' arguments as a batch of one: [N, 3 | 4] points and [3] or [4] camera vectors."""
    def lift(what, x, rank):
        if x is None:
            return None
        t = x if isinstance(x, torch.Tensor) else np.asarray(x)
        if t.ndim != rank:
            shape = "[N, 3] or [N, 4]" if rank == 2 else "[3] or [4]"
            raise ValueError(f"{name}: {what} is {list(t.shape)}, expected {shape}")
        return t[None]
    camera = {k: (lift(f"camera['{k}']", v, 1) if k in VIEW_KEYS else v) for k, v in camera.items()}
    return lift("pos", pos, 2), lift("normal", normal, 2), camera


def _first(res: Dict[str, Optional[torch.Tensor]]) -> Dict[str, Optional[torch.Tensor]]:
    return {k: None if v is None else v[0] for k, v in res.items()}


def world_to_cam_batched(pos, normal, camera: Mapping, *, camera_grad: bool = False):
    """pos [B, N, 3] or [B, N, 4] and normal [B, N', 3] or [B, N', 4] (its first three columns are read) in world
    coordinates, either None; camera: eye / at / up [B, 3] or [B, 4].  Returns {'pos': [B, N, 4], 'normal': [B, N', 3]}
    in the camera's frame, float32 on the GPU, None for a None input: pos = lookat [p, w] with w = 1 for three columns
    and column 3 = w; normal = n^T (lookat_inv's 3 x 3), not normalised.  Differentiable in pos (all columns) and
    normal.  camera_grad=True lets camera['eye'], ['at'] and ['up'] require grad (they are refused otherwise) and
    gives them their gradient, in their own shape, dtype and device; values and the other gradients are bit for bit
    those of the same call with the camera detached."""
    return _transform("world_to_cam_batched", False, pos, normal, camera, camera_grad)


def cam_to_world_batched(pos, normal, camera: Mapping, *, camera_grad: bool = False):
    """world_to_cam_batched's inverse direction: pos = [x y z | eye] [p, w], normal = n^T (lookat's 3 x 3)."""
    return _transform("cam_to_world_batched", True, pos, normal, camera, camera_grad)


def world_to_cam(pos, normal, camera: Mapping, *, camera_grad: bool = False):
    """world_to_cam_batched for one view: pos [N, 3 | 4], normal [N', 3 | 4], camera eye / at / up [3] or [4]; the
    results come without the leading B."""
    name = "world_to_cam"
    return _first(_transform(name, False, *_one_view(name, pos, normal, camera), camera_grad))


def cam_to_world(pos, normal, camera: Mapping, *, camera_grad: bool = False):
    """cam_to_world_batched for one view, as world_to_cam."""
    name = "cam_to_world"
    return _first(_transform(name, True, *_one_view(name, pos, normal, camera), camera_grad))


def _project(name: str, coords: bool, surfels, camera: Mapping, camera_grad):
    camera_grad = check_camera_grad(name, camera_grad)
    W, H = camera_frame(name, camera, camera_grad=camera_grad)
    if W * H > MAX_POINTS:
        raise ValueError(f"{name}: camera['viewport']: {W} x {H} pixels, expected at most 2^24")
    surfels = _points(name, "surfels", surfels)
    if surfels is None:
        raise ValueError(f"{name}: surfels is missing")
    B, N, cols = surfels.shape
    fovy, focal, view = camera_views(name, camera, B, camera_grad=camera_grad)
    dev = gpu_device(name, (surfels,))
    params = _lib.SrhProjectCoordsParams(n_views=B, n_points=N, cols=cols, width=W, height=H, fovy=fovy,
                                         focal_length=focal)
    return _ProjectFunction.apply(params, coords, upload_view(view, dev), f32(surfels, dev))


def project_surfels(surfel_pos_WC, camera: Mapping, *, camera_grad: bool = False) -> torch.Tensor:
    """surfel_pos_WC [B, N, 3] or [B, N, 4] in world coordinates, N free; camera: eye / at / up [B, 3] or [B, 4] and
    one shared viewport, fovy and focal_length.  Returns [B, N, 3], float32 on the GPU: (f X / Z, f Y / Z, -Z) of the
    camera-space point, a Z of exactly 0 divided by 1 (and x, y then have exactly zero gradient with respect to Z).
    Differentiable in the surfels, and with camera_grad=True in camera['eye'], ['at'] and ['up'] as in
    world_to_cam_batched."""
    return _project("project_surfels", False, surfel_pos_WC, camera, camera_grad)[0]


def project_image_coordinates(surfels, camera: Mapping, *, camera_grad: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """project_surfels taken on to pixels.  Returns (px_idx [B, N] int64, px_coord [B, N, 3] float32), both on the GPU:
    px_coord = (x (-(W - 1) / w) + W / 2, y ((H - 1) / h) + H / 2, -Z) with the frame h = 2 f tan(fovy / 2), w = h W / H;
    px_idx = round(px_coord_y - 1/2) W + round(px_coord_x - 1/2), ties to even, and W H (the dump slot) for a surfel
    outside the frame, NaN or beyond an int -- the key projection_renderer bins by, bit for bit.  px_coord is
    differentiable as project_surfels' result is; px_idx carries no gradient."""
    px_coord, px_idx = _project("project_image_coordinates", True, surfels, camera, camera_grad)
    return px_idx.to(torch.int64), px_coord
