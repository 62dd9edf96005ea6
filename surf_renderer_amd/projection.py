"""The reference's surfel re-projection layer (diffrend/torch/projection_layer.py:170-278) under its own name, so the
swap is one import:

    # from diffrend.torch.projection_layer import projection_renderer_differentiable_fast
    from surf_renderer_amd import projection_renderer_differentiable_fast
    out, proj_out = projection_renderer_differentiable_fast(surfels, rgb, camera, rotated_image=None, blur_size=0.15)

A view's surfels (W H world-space points with a D-channel value each) are projected into another camera, spread
bilinearly over four pixels with weighted-blended order-independent transparency, blurred with a Gaussian and
optionally merged with a second image through the soft coverage mask.  Forward and backward are HIP kernels
(surf_renderer_amd/csrc/srh_projection.h), restated as gathers: fp64 arithmetic, fp32 results, no float atomics, so
values and gradients are identical from run to run.  Differentiable in surfels, rgb and rotated_image; the camera is
not differentiable.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib

_NAME = "projection_renderer_differentiable_fast"


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class _ProjFunction(torch.autograd.Function):
    """(surfels [B, N, 3], rgb [B, N, D], rotated [B, N, D] or None), fp32 contiguous -> out, mask, image1, depth."""

    @staticmethod
    def forward(ctx, params, view, want_depth, surfels, rgb, rotated):
        lib = _lib.load()
        B, N, D = rgb.shape
        dev = rgb.device
        stream = torch.cuda.current_stream(dev).cuda_stream

        def scratch(which):
            return torch.empty((lib.srh_projection_workspace_bytes(C.byref(params), which),), dtype=torch.uint8,
                               device=dev)

        ws = scratch(_lib.PROJ_WS_FWD)
        keys = torch.empty((B, N), dtype=torch.int32, device=dev)
        _lib.check(lib.srh_projection_keys(C.byref(params), view.data_ptr(), surfels.data_ptr(), ws.data_ptr(),
                                           ws.numel(), keys.data_ptr(), stream))
        # the one step left to torch: a stable sort fixes the order inside every cell's list, and with it every sum
        order = torch.sort(keys, dim=1, stable=True).indices.to(torch.int32)
        # without a backward to come the kernels keep nothing
        saved = scratch(_lib.PROJ_WS_SAVED) if any(ctx.needs_input_grad[3:]) else None
        out, image1 = torch.empty_like(rgb), torch.empty_like(rgb)
        mask = torch.empty((B, N), dtype=torch.float32, device=dev)
        depth = torch.empty_like(mask) if want_depth else None
        _lib.check(lib.srh_projection_fwd(C.byref(params), rgb.data_ptr(), _ptr(rotated), keys.data_ptr(),
                                          order.data_ptr(), ws.data_ptr(), ws.numel(), _ptr(saved),
                                          0 if saved is None else saved.numel(), out.data_ptr(), mask.data_ptr(),
                                          image1.data_ptr(), _ptr(depth), stream))
        ctx.params = params
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(view, surfels, rgb, rotated, saved)
        return out, mask, image1, depth

    @staticmethod
    def backward(ctx, g_out, g_mask, g_image1, g_depth):
        view, surfels, rgb, rotated, saved = ctx.saved_tensors
        # an input that does not require grad gets no buffer, and the kernels skip the work only it would need
        grads = [torch.empty_like(t) if t is not None and ctx.needs_input_grad[3 + k] else None
                 for k, t in enumerate((surfels, rgb, rotated))]
        ups = [None if g is None else g.to(torch.float32).contiguous() for g in (g_out, g_mask, g_image1, g_depth)]
        if any(g is not None for g in grads):
            if all(u is None for u in ups):
                for g in grads:
                    if g is not None:
                        g.zero_()
            else:
                lib = _lib.load()
                ws = torch.empty((lib.srh_projection_workspace_bytes(C.byref(ctx.params), _lib.PROJ_WS_BWD),),
                                 dtype=torch.uint8, device=rgb.device)
                _lib.check(lib.srh_projection_bwd(
                    C.byref(ctx.params), view.data_ptr(), surfels.data_ptr(), rgb.data_ptr(), _ptr(rotated),
                    saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(), *[_ptr(u) for u in ups],
                    *[_ptr(g) for g in grads], torch.cuda.current_stream(rgb.device).cuda_stream))
        return (None, None, None, *grads)


def _normalize(u: torch.Tensor) -> torch.Tensor:
    """diffrend.torch.utils.normalize: u / nz(sqrt(sum(u^2 + 1e-10)))."""
    d = torch.sqrt(torch.sum(u * u + 1e-10, dim=-1, keepdim=True))
    return u / torch.where(d.abs() > 0, d, torch.ones_like(d))


def view_matrices(eye: torch.Tensor, at: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """The reference's lookat(eye, at, up) (torch/utils.py:376-427) of [B, 3] float64 triples: the inverse of
    [x y z eye; 0 0 0 1], whose first three rows [B, 3, 4] take a world point to camera coordinates."""
    z = _normalize(eye - at)
    x = _normalize(torch.cross(_normalize(up), z, dim=-1))
    y = torch.cross(z, x, dim=-1)
    inv = torch.zeros((eye.shape[0], 4, 4), dtype=torch.float64)
    inv[:, :3, :3] = torch.stack((x, y, z), dim=-1)
    inv[:, :3, 3] = eye
    inv[:, 3, 3] = 1.0
    return torch.linalg.inv(inv)[:, :3, :]


def blur_taps(blur_size: float, height: int) -> Tuple[int, np.ndarray]:
    """(half-width, taps[|d|]) of the reference's blur: sigma = blur_size * H / 6, half = floor(3 sigma), normalised."""
    sigma = blur_size * height / 6
    half = int(math.floor(sigma * 3))
    k = np.exp(-np.arange(-half, half + 1, dtype=np.float64) ** 2 / (2 * sigma ** 2))
    return half, (k / k.sum())[half:]


def as_float_tensor(name: str, x: Any, caller: str = _NAME) -> torch.Tensor:
    if x is None:
        raise ValueError(f"{caller}: {name} is missing")
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if not t.is_floating_point():
        raise ValueError(f"{caller}: {name} has dtype {t.dtype}, expected a floating-point type")
    return t


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def camera_frame(name: str, camera: Mapping, label: str = "camera") -> Tuple[int, int]:
    """The first half of the camera checks (ValueError, prefixed `name`, the camera called `label`): every entry is
    there, none requires grad, and the viewport is a frame.  Returns (W, H)."""
    for k in ("eye", "at", "up", "viewport", "fovy", "focal_length"):
        if k not in camera or camera[k] is None:
            raise ValueError(f"{name}: {label}['{k}'] is missing")
    for k, v in camera.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise ValueError(f"{name}: {label}['{k}'] requires grad, but the camera is not differentiable on this "
                             "path (detach it)")
    vp = _host(camera["viewport"]).reshape(-1)
    if vp.size != 4:
        raise ValueError(f"{name}: {label}['viewport']: expected 4 values, got {vp.size}")
    W, H = int(vp[2] - vp[0]), int(vp[3] - vp[1])
    if W < 1 or H < 1:
        raise ValueError(f"{name}: {label}['viewport']: empty {W} x {H} frame")
    return W, H


def camera_views(name: str, camera: Mapping, B: int, label: str = "camera") -> Tuple[float, float, torch.Tensor]:
    """The second half, once the batch size is known: fovy and focal_length in range, eye / at / up finite [B, 3] or
    [B, 4] under the reference's w conventions and not degenerate.  Returns (fovy, focal_length, the per-view matrices
    [B, 3, 4] float64 on the host)."""
    fovy, focal = float(_host(camera["fovy"]).reshape(-1)[0]), float(_host(camera["focal_length"]).reshape(-1)[0])
    if not 0 < fovy < math.pi:
        raise ValueError(f"{name}: {label}['fovy'] = {fovy}, expected 0 < fovy < pi")
    if not (math.isfinite(focal) and focal > 0):
        raise ValueError(f"{name}: {label}['focal_length'] = {focal}, expected positive and finite")
    cam = {}
    for k in ("eye", "at", "up"):
        v = np.asarray(_host(camera[k]), dtype=np.float64)
        if v.ndim != 2 or v.shape[0] != B or v.shape[1] not in (3, 4) or not np.all(np.isfinite(v)):
            raise ValueError(f"{name}: {label}['{k}'] is {list(v.shape)}, expected finite [{B}, 3] or [{B}, 4]")
        if v.shape[1] == 4:          # lookat_rot_inv's conventions; world_to_cam_batched then drops w
            if k == "up" and np.any(v[:, 3] != 0):
                raise ValueError(f"{name}: {label}['up'] is a direction: w must be 0")
            if k != "up" and np.any(v[:, 3] == 0):
                raise ValueError(f"{name}: {label}['{k}'] is a point: w must not be 0")
        cam[k] = torch.from_numpy(np.ascontiguousarray(v[:, :3]))
    if torch.any(torch.all(cam["eye"] == cam["at"], dim=-1)):
        raise ValueError(f"{name}: {label}['eye'] == {label}['at']")
    if torch.any(torch.linalg.cross(cam["up"], cam["eye"] - cam["at"]).abs().amax(-1) == 0):
        raise ValueError(f"{name}: {label}['up'] is zero or parallel to eye - at")
    return fovy, focal, view_matrices(cam["eye"], cam["at"], cam["up"])


def _validate(surfels, rgb, camera: Mapping, rotated_image, blur_size):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError).  Returns the
    tensors, (B, H, W, D), the per-view matrices [B, 3, 4] float64 on the host, and the blur's half-width and taps."""
    surfels, rgb = as_float_tensor("surfels", surfels), as_float_tensor("rgb", rgb)
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
    if not 1 <= D <= _lib.PROJ_MAX_CHANNELS:
        raise ValueError(f"{_NAME}: rgb has {D} channels, expected 1..{_lib.PROJ_MAX_CHANNELS}")
    if rotated_image is not None:
        rotated_image = as_float_tensor("rotated_image", rotated_image)
        if tuple(rotated_image.shape) != tuple(rgb.shape):
            raise ValueError(f"{_NAME}: rotated_image is {list(rotated_image.shape)}, rgb is {list(rgb.shape)}")
    blur_size = float(blur_size)
    if not (math.isfinite(blur_size) and blur_size > 0):
        raise ValueError(f"{_NAME}: blur_size = {blur_size}, expected positive and finite")
    if math.floor(blur_size * H / 6 * 3) > _lib.PROJ_MAX_BLUR_HALF:
        raise ValueError(f"{_NAME}: blur_size = {blur_size} at H = {H} gives a blur half-width of "
                         f"{math.floor(blur_size * H / 6 * 3)}, at most {_lib.PROJ_MAX_BLUR_HALF}")
    half, taps = blur_taps(blur_size, H)
    fovy, focal, view = camera_views(_NAME, camera, B)
    return surfels, rgb, rotated_image, (B, H, W, D), view, half, taps, fovy, focal


def projection_renderer_differentiable_fast(surfels, rgb, camera: Mapping, rotated_image=None, blur_size: float = 0.15,
                                            use_depth: bool = True, use_center_dist: bool = True,
                                            compute_new_depth: bool = False, blur_rotated_image: bool = True,
                                            detach_mask: bool = False, detach_mask2: bool = False,
                                            detach_depth_merge: bool = False) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The reference's call.  surfels [B, N, 3] in world coordinates with N = W H; rgb [B, N, D] or [B, H, W, D], D in
    1..4; rotated_image like rgb or None; camera: eye / at / up [B, 3] or [B, 4] and one shared viewport, fovy and
    focal_length.  Returns (out, {'mask': [..., 1], 'image1': like rgb, and with compute_new_depth 'depth': [..., 1]}),
    float32 on the GPU, differentiable in surfels, rgb and rotated_image through every output."""
    surfels, rgb, rotated_image, (B, H, W, D), view, half, taps, fovy, focal = _validate(
        surfels, rgb, camera, rotated_image, blur_size)
    if not torch.cuda.is_available():
        raise RuntimeError(f"{_NAME}: the hip backend needs a GPU")
    leaves = [t for t in (surfels, rgb, rotated_image) if t is not None]
    dev = next((t.device for t in leaves if t.device.type == "cuda"), torch.device("cuda"))
    # autograd carries the gradient back through these conversions to the leaf's own dtype, layout and device
    x = [None if t is None else t.to(device=dev, dtype=torch.float32).reshape(B, H * W, -1).contiguous()
         for t in (surfels, rgb, rotated_image)]
    flags = (_lib.PROJ_USE_DEPTH * bool(use_depth) | _lib.PROJ_USE_CENTER_DIST * bool(use_center_dist)
             | _lib.PROJ_BLUR_ROTATED * bool(blur_rotated_image) | _lib.PROJ_DETACH_MASK * bool(detach_mask)
             | _lib.PROJ_DETACH_MASK2 * bool(detach_mask2) | _lib.PROJ_DETACH_DEPTH_MERGE * bool(detach_depth_merge))
    params = _lib.SrhProjectionParams(n_views=B, width=W, height=H, channels=D, flags=flags, blur_half=half, fovy=fovy,
                                      focal_length=focal)
    params.taps[:half + 1] = taps.tolist()
    out, mask, image1, depth = _ProjFunction.apply(params, view.reshape(B, 12).contiguous().to(dev),
                                                   bool(compute_new_depth), *x)
    proj_out = {"mask": mask.reshape(*rgb.shape[:-1], 1), "image1": image1.reshape(rgb.shape)}
    if compute_new_depth:
        proj_out["depth"] = depth.reshape(*rgb.shape[:-1], 1)
    return out.reshape(rgb.shape), proj_out
