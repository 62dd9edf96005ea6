"""What the three re-projection layers (projection, dense_projection, reverse_projection) share on the host beyond
_layer.py and _camera.py: the checks of the surfel and image arguments, the flattening to [B, N, .], the view upload,
the sort between the key and the gather kernels, and the reshapes of the results."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Mapping, Optional

import torch

from . import _lib
from ._camera import camera_frame
from ._layer import as_float_tensor, f32


def check_channels(name: str, rgb: torch.Tensor) -> None:
    D = rgb.shape[-1] if rgb.dim() else 0
    if not 1 <= D <= _lib.PROJ_MAX_CHANNELS:
        raise ValueError(f"{name}: rgb has {D} channels, expected 1..{_lib.PROJ_MAX_CHANNELS}")


def rotated_like(name: str, rotated_image, rgb: torch.Tensor) -> Optional[torch.Tensor]:
    if rotated_image is None:
        return None
    rotated_image = as_float_tensor("rotated_image", rotated_image, name)
    if tuple(rotated_image.shape) != tuple(rgb.shape):
        raise ValueError(f"{name}: rotated_image is {list(rotated_image.shape)}, rgb is {list(rgb.shape)}")
    return rotated_image


def validate_surfels(name: str, surfels, rgb, camera: Mapping, rotated_image, blur_size, why: str,
                     camera_grad: Optional[bool] = None):
    """The checks of (surfels, rgb, camera's frame, rotated_image, blur_size) of the layer `name` (ValueError), before
    anything reaches the GPU; `why` ends the message for N != W H.  The caller goes on with its own blur and with
    camera_views.  `camera_grad` is given by the layer that has the keyword (camera_frame).  Returns the tensors,
    (B, H, W, D) and blur_size as a float."""
    surfels, rgb = as_float_tensor("surfels", surfels, name), as_float_tensor("rgb", rgb, name)
    W, H = camera_frame(name, camera, camera_grad=camera_grad)
    if surfels.dim() != 3 or surfels.shape[-1] != 3:
        raise ValueError(f"{name}: surfels is {list(surfels.shape)}, expected [B, N, 3]")
    B, N = surfels.shape[:2]
    if B < 1:
        raise ValueError(f"{name}: an empty batch")
    if N != W * H:
        raise ValueError(f"{name}: {N} surfels per view, expected W x H = {W} x {H} = {W * H} ({why})")
    D = rgb.shape[-1] if rgb.dim() else 0
    if tuple(rgb.shape) not in ((B, N, D), (B, H, W, D)):
        raise ValueError(f"{name}: rgb is {list(rgb.shape)}, expected [{B}, {N}, D] or [{B}, {H}, {W}, D]")
    check_channels(name, rgb)
    rotated_image = rotated_like(name, rotated_image, rgb)
    blur_size = float(blur_size)
    if not (math.isfinite(blur_size) and blur_size > 0):
        raise ValueError(f"{name}: blur_size = {blur_size}, expected positive and finite")
    return surfels, rgb, rotated_image, (B, H, W, D), blur_size


def flat(tensors: Iterable[Optional[torch.Tensor]], B: int, N: int, device) -> List[Optional[torch.Tensor]]:
    """Each tensor as the kernels read it: float32, contiguous, [B, N, .] on `device`."""
    return [None if t is None else f32(t, device).reshape(B, N, -1) for t in tensors]


def upload_view(view: torch.Tensor, device) -> torch.Tensor:
    """camera_views' [B, 3, 4] float64 matrices as the kernels' [B, 12] table."""
    return view.reshape(view.shape[0], 12).contiguous().to(device)


def sorted_order(keys: torch.Tensor) -> torch.Tensor:
    """The one step left to torch between a layer's key kernel and its gather: a stable sort fixes the order inside
    every cell's list, and with it every sum."""
    return torch.sort(keys, dim=1, stable=True).indices.to(torch.int32)


def shaped_like(shape, mask, image1=None, depth=None) -> Dict[str, torch.Tensor]:
    """The kernels' flat results in the layout of an image of `shape` [..., D]: mask and depth [..., 1], image1 [..., D];
    an entry for each one given."""
    out = {"mask": mask.reshape(*shape[:-1], 1)}
    if image1 is not None:
        out["image1"] = image1.reshape(shape)
    if depth is not None:
        out["depth"] = depth.reshape(*shape[:-1], 1)
    return out
