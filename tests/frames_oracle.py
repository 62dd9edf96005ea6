"""fp64 restatement of the reference's frame transforms and point projection -- world_to_cam[_batched],
cam_to_world[_batched] (diffrend/torch/utils.py:539-647), project_surfels and project_image_coordinates
(diffrend/torch/projection_layer.py:19-85) -- in torch on the CPU, with the camera's eye, at and up as possible autograd
leaves, so that autograd supplies the gradient oracle, the camera's included.  Test infrastructure:
tests/test_frames_oracle_cpu.py pins it to the reference's own float64 and float32 results
(tests/golden/frames/fr1_*.npz), tests/test_hip_frames.py compares the kernels with it.

lookat, nonzero_divide and the camera leaves are projection_oracle's and camera_chain_oracle's, by import.  A camera
entry may be an array or a tensor, [B, 3] or [B, 4]; the w column is dropped before lookat.  `dtype` and `device` follow
the inputs: tools/bench_frames.py times this composition in float32 on the GPU."""
from typing import Dict, Mapping, Optional

import numpy as np
import torch

import camera_chain_oracle as cco
import projection_oracle as po

CAMERA_KEYS = cco.CAMERA_KEYS


def homogeneous(p):
    """[..., 3] -> [..., 4] with w = 1; [..., 4] as it is."""
    return p if p.shape[-1] == 4 else torch.cat((p, torch.ones_like(p[..., :1])), dim=-1)


def _tables(camera: Mapping, like):
    """(world-to-camera [B, 3, 4], camera-to-world [B, 3, 4]) in the dtype and on the device of `like`."""
    dt, dev = like.dtype, like.device
    R, eye = cco.camera_to_world(camera, dt)
    return cco.world_to_camera(camera, dt)[:, :3].to(dev), torch.cat((R, eye[..., None]), dim=-1).to(dev)


def _apply(pos, normal, m_pos, m_normal) -> Dict[str, Optional[torch.Tensor]]:
    """pos -> [M p | w] (four columns), normal -> n^T A with A the 3 x 3 of the OTHER direction's matrix."""
    out = {"pos": None, "normal": None}
    if pos is not None:
        h = homogeneous(pos)
        out["pos"] = torch.cat((h @ m_pos.transpose(-1, -2), h[..., 3:]), dim=-1)
    if normal is not None:
        out["normal"] = normal[..., :3] @ m_normal[..., :3, :3]
    return out


def world_to_cam_batched(pos, normal, camera: Mapping):
    like = pos if pos is not None else normal
    w2c, c2w = _tables(camera, like)
    return _apply(pos, normal, w2c, c2w)


def cam_to_world_batched(pos, normal, camera: Mapping):
    like = pos if pos is not None else normal
    w2c, c2w = _tables(camera, like)
    return _apply(pos, normal, c2w, w2c)


TRANSFORMS = {"to_cam": world_to_cam_batched, "to_world": cam_to_world_batched}


def project_surfels(surfels, camera: Mapping):
    cc = world_to_cam_batched(surfels, None, camera)["pos"]
    f = float(camera["focal_length"])
    return torch.stack((f * po.nonzero_divide(cc[..., 0], cc[..., 2]), f * po.nonzero_divide(cc[..., 1], cc[..., 2]),
                        -cc[..., 2]), dim=-1)


def frame_scales(camera: Mapping):
    """((sx, sy), (W / 2, H / 2)) of px_coord = plane * scale + half."""
    W, H = po.frame(camera)
    f, fovy = float(camera["focal_length"]), float(camera["fovy"])
    h = np.tan(fovy / 2) * 2 * f
    w = h * (float(W) / float(H))
    return (-(W - 1) / w, (H - 1) / h), (W / 2.0, H / 2.0)


def project_image_coordinates(surfels, camera: Mapping):
    """(px_idx [B, N] int64 with W H the dump slot, px_coord [B, N, 3])."""
    W, H = po.frame(camera)
    plane = project_surfels(surfels, camera)
    (sx, sy), (hx, hy) = frame_scales(camera)
    px = torch.stack((plane[..., 0] * sx + hx, plane[..., 1] * sy + hy, plane[..., 2]), dim=-1)
    r = torch.round(px[..., :2].detach() - 0.5)                 # ties to even
    inside = (r[..., 0] >= 0) & (r[..., 0] <= W - 1) & (r[..., 1] >= 0) & (r[..., 1] <= H - 1)   # false for NaN
    safe = torch.where(inside[..., None], r, torch.zeros_like(r)).long()
    idx = torch.where(inside, safe[..., 1] * W + safe[..., 0], torch.full_like(safe[..., 0], W * H))
    return idx, px


def transform_gradients(direction, inputs, camera: Mapping, upstream, camera_wrt=CAMERA_KEYS):
    """({'pos', 'normal'} of those given, {input: gradient}, {entry: gradient}) of TRANSFORMS[direction]."""
    def fn(x, c):
        res = TRANSFORMS[direction](x.get("pos"), x.get("normal"), c["camera"])
        return {k: v for k, v in res.items() if v is not None}
    vals, grads, cams = cco.autograd(fn, inputs, ("pos", "normal"), {"camera": camera}, upstream, ("pos", "normal"),
                                     camera_wrt)
    return vals, grads, cams["camera"]


def project_gradients(coords: bool, surfels, camera: Mapping, upstream, camera_wrt=CAMERA_KEYS):
    """project_surfels ({'plane'}) or with `coords` project_image_coordinates ({'px_coord', 'px_idx'})."""
    def fn(x, c):
        if not coords:
            return {"plane": project_surfels(x["surfels"], c["camera"])}
        idx, px = project_image_coordinates(x["surfels"], c["camera"])
        return {"px_coord": px, "px_idx": idx}
    vals, grads, cams = cco.autograd(fn, {"surfels": surfels}, ("surfels",), {"camera": camera}, upstream, ("surfels",),
                                     camera_wrt)
    return vals, grads, cams["camera"]
