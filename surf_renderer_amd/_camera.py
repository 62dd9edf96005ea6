"""The camera of the re-projection layers (projection, dense_projection, reverse_projection): the host-side checks of a
camera dict and the reference's lookat as per-view world-to-camera matrices."""
from __future__ import annotations

import math
from typing import Mapping, Tuple

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


def camera_frame(name: str, camera: Mapping, label: str = "camera") -> Tuple[int, int]:
    """The first half of the camera checks (ValueError, prefixed `name`, the camera called `label`): every entry is
    there, none requires grad, and the viewport is a frame.  Returns (W, H)."""
    camera_entries(name, camera, ("eye", "at", "up", "viewport", "fovy", "focal_length"), label)
    return camera_viewport(name, camera, label)


def camera_entries(name: str, camera: Mapping, keys, label: str = "camera") -> None:
    """Every entry among `keys` is there and no entry requires grad (ValueError)."""
    for k in keys:
        if k not in camera or camera[k] is None:
            raise ValueError(f"{name}: {label}['{k}'] is missing")
    for k, v in camera.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise ValueError(f"{name}: {label}['{k}'] requires grad, but the camera is not differentiable on this "
                             "path (detach it)")


def camera_viewport(name: str, camera: Mapping, label: str = "camera") -> Tuple[int, int]:
    """(W, H) of the camera's viewport, which must be a frame (ValueError)."""
    vp = _host(camera["viewport"]).reshape(-1)
    if vp.size != 4:
        raise ValueError(f"{name}: {label}['viewport']: expected 4 values, got {vp.size}")
    W, H = int(vp[2] - vp[0]), int(vp[3] - vp[1])
    if W < 1 or H < 1:
        raise ValueError(f"{name}: {label}['viewport']: empty {W} x {H} frame")
    return W, H


def camera_views(name: str, camera: Mapping, B: int, label: str = "camera",
                 to_world: bool = False) -> Tuple[float, float, torch.Tensor]:
    """The second half, once the batch size is known: fovy and focal_length in range, eye / at / up finite [B, 3] or
    [B, 4] under the reference's w conventions and not degenerate.  Returns (fovy, focal_length, the per-view matrices
    [B, 3, 4] float64 on the host): world to camera, or with `to_world` camera to world."""
    fovy, focal = float(_host(camera["fovy"]).reshape(-1)[0]), float(_host(camera["focal_length"]).reshape(-1)[0])
    if not 0 < fovy < math.pi:
        raise ValueError(f"{name}: {label}['fovy'] = {fovy}, expected 0 < fovy < pi")
    if not (math.isfinite(focal) and focal > 0):
        raise ValueError(f"{name}: {label}['focal_length'] = {focal}, expected positive and finite")
    cam = camera_vectors(name, camera, B, label)
    return fovy, focal, (inverse_view_matrices if to_world else view_matrices)(cam["eye"], cam["at"], cam["up"])


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
