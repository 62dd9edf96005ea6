"""The camera of the re-projection layers (projection, dense_projection, reverse_projection): the host-side checks of a
camera dict and the reference's lookat as per-view world-to-camera matrices."""
from __future__ import annotations

import math
from typing import Mapping, Optional, Tuple

import numpy as np
import torch


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


def inverse_view_matrices(eye: torch.Tensor, at: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """The first three rows [B, 3, 4] of the reference's lookat_inv(eye, at, up) (torch/utils.py:385-427) of [B, 3]
    float64 triples: [x y z | eye], which takes a camera-space point to world coordinates."""
    z = _normalize(eye - at)
    x = _normalize(torch.cross(_normalize(up), z, dim=-1))
    y = torch.cross(z, x, dim=-1)
    return torch.cat((torch.stack((x, y, z), dim=-1), eye[..., None]), dim=-1)


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


VIEW_KEYS = ("eye", "at", "up")      # what a layer with `camera_grad` differentiates in


def check_camera_grad(name: str, camera_grad) -> bool:
    if not isinstance(camera_grad, bool):
        raise ValueError(f"{name}: camera_grad = {camera_grad!r}, expected True or False")
    return camera_grad


def camera_frame(name: str, camera: Mapping, label: str = "camera",
                 camera_grad: Optional[bool] = None) -> Tuple[int, int]:
    """The first half of the camera checks (ValueError, prefixed `name`, the camera called `label`): every entry is
    there, none requires grad, and the viewport is a frame.  Returns (W, H).  `camera_grad` is given by the layers that
    have the keyword: True lets eye / at / up require grad."""
    camera_entries(name, camera, ("eye", "at", "up", "viewport", "fovy", "focal_length"), label, camera_grad)
    return camera_viewport(name, camera, label)


def camera_entries(name: str, camera: Mapping, keys, label: str = "camera", camera_grad: Optional[bool] = None) -> None:
    """Every entry among `keys` is there and no entry requires grad (ValueError) -- with `camera_grad` no entry but
    eye / at / up: fovy, focal_length and the viewport get no gradient anywhere, so one that asks for it is refused."""
    for k in keys:
        if k not in camera or camera[k] is None:
            raise ValueError(f"{name}: {label}['{k}'] is missing")
    # camera_grad: None = the layer has no such keyword (the hint does not offer it), False / True = the caller's value
    for k, v in camera.items():
        if isinstance(v, torch.Tensor) and v.requires_grad and not (camera_grad and k in VIEW_KEYS):
            hint = "detach it" if camera_grad is None or k not in VIEW_KEYS else "detach it, or pass camera_grad=True"
            raise ValueError(f"{name}: {label}['{k}'] requires grad, but the camera is not differentiable on this "
                             f"path ({hint})")


def camera_viewport(name: str, camera: Mapping, label: str = "camera") -> Tuple[int, int]:
    """(W, H) of the camera's viewport, which must be a frame (ValueError)."""
    vp = _host(camera["viewport"]).reshape(-1)
    if vp.size != 4:
        raise ValueError(f"{name}: {label}['viewport']: expected 4 values, got {vp.size}")
    W, H = int(vp[2] - vp[0]), int(vp[3] - vp[1])
    if W < 1 or H < 1:
        raise ValueError(f"{name}: {label}['viewport']: empty {W} x {H} frame")
    return W, H


def camera_views(name: str, camera: Mapping, B: int, label: str = "camera", to_world: bool = False,
                 camera_grad: bool = False) -> Tuple[float, float, torch.Tensor]:
    """The second half, once the batch size is known: fovy and focal_length in range, eye / at / up finite [B, 3] or
    [B, 4] under the reference's w conventions and not degenerate.  Returns (fovy, focal_length, the per-view matrices
    [B, 3, 4] float64 on the host): world to camera, or with `to_world` camera to world.  With `camera_grad` the
    matrices are attached to those of eye / at / up that require grad (differentiable_vectors)."""
    fovy, focal = float(_host(camera["fovy"]).reshape(-1)[0]), float(_host(camera["focal_length"]).reshape(-1)[0])
    if not 0 < fovy < math.pi:
        raise ValueError(f"{name}: {label}['fovy'] = {fovy}, expected 0 < fovy < pi")
    if not (math.isfinite(focal) and focal > 0):
        raise ValueError(f"{name}: {label}['focal_length'] = {focal}, expected positive and finite")
    cam = camera_vectors(name, camera, B, label)
    if camera_grad:
        cam = differentiable_vectors(camera, cam)
    return fovy, focal, (inverse_view_matrices if to_world else view_matrices)(cam["eye"], cam["at"], cam["up"])


def differentiable_vectors(camera: Mapping, checked: Mapping[str, torch.Tensor]) -> Mapping[str, torch.Tensor]:
    """camera_vectors' result with every entry whose tensor requires grad replaced by that tensor's own float64 host
    copy, which autograd carries back to the leaf's dtype, device and shape.  The values, and with them the bits of the
    matrices, are camera_vectors': a float32 converts to float64 exactly either way.  The w column is dropped as
    world_to_cam_batched and cam_to_world_batched drop it, before lookat, so it gets a zero gradient."""
    return {k: (camera[k].to(device="cpu", dtype=torch.float64)[:, :3]
                if isinstance(camera[k], torch.Tensor) and camera[k].requires_grad else v) for k, v in checked.items()}


def camera_vectors(name: str, camera: Mapping, B: int, label: str = "camera") -> Mapping[str, torch.Tensor]:
    """eye / at / up as [B, 3] float64 on the host: finite [B, 3] or [B, 4] under the reference's w conventions and not
    degenerate (ValueError)."""
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
    return cam
