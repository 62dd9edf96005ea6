"""fp64 restatement of the depth lift, depth_to_surfels: the reference's cam_to_world_batched(z_to_pcl_CC_batched(-depth,
camera), None, camera)['pos'] (diffrend/torch/renderer.py:510-534, torch/utils.py:622-647 with lookat_inv), in torch on
the CPU, so that autograd supplies the gradient oracle.  Test infrastructure: tests/test_surfels_oracle_cpu.py pins it
to the reference's own results (tests/golden/surfels/sf1_*.npz), tests/test_hip_surfels.py compares the kernels with it.

    d = max(depth, 0);  h = 2 tan(fovy / 2) f,  w = h W / H
    P_cc = (d x_j / f, d y_i / f, -d)  for pixel q = i W + j
    P_wc = [x y z] P_cc + eye,  z = unit(eye - at), x = unit(unit(up) x z), y = z x x

`grid` chooses the pixel grid (x_j, y_i), both float32-valued:
    "numpy"   fp32(np.linspace(-1, 1, W) * (w / 2)), fp32(np.linspace(1, -1, H) * (h / 2)) -- z_to_pcl_CC's, the kernels'
    "torch"   torch.linspace(-1, 1, W) * w / 2, torch.linspace(1, -1, H) * h / 2, all in float32 -- the batched reference
              function's
They differ by at most GRID_BOUND = 4 * 2^-24 of the half extent: the torch grid's three float32 roundings (the step,
the product i * step, the sum with the start point; the later * w / 2 is counted with the one rounding of the numpy
grid).  `dtype` and `device` exist for tools/bench_depth_reprojection.py, which times this composition in float32 on the
GPU."""
from typing import Mapping

import numpy as np
import torch

import projection_oracle as po

INPUTS = ("depth",)
OUTPUTS = ("pos",)
GRID_BOUND = 4 * 2.0 ** -24


def frame_extent(camera: Mapping):
    """(w / 2, h / 2) of the pinhole frame at the focal distance."""
    W, H = po.frame(camera)
    h = np.tan(float(camera["fovy"]) / 2) * 2 * float(camera["focal_length"])
    return h * (W / H) / 2, h / 2


def pixel_grid(camera: Mapping, grid="numpy"):
    """(x [W], y [H]) as float64 arrays of float32 values."""
    W, H = po.frame(camera)
    half_w, half_h = frame_extent(camera)
    if grid == "numpy":
        x, y = np.linspace(-1, 1, W) * half_w, np.linspace(1, -1, H) * half_h
        return x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    assert grid == "torch", grid
    x = torch.linspace(-1, 1, W, dtype=torch.float32) * (2 * half_w) / 2
    y = torch.linspace(1, -1, H, dtype=torch.float32) * (2 * half_h) / 2
    return x.numpy().astype(np.float64), y.numpy().astype(np.float64)


def camera_to_world(camera: Mapping, dtype=torch.float64):
    """[B, 3, 3] rotation (columns x, y, z) and [B, 3] eye."""
    eye, at, up = (torch.as_tensor(np.asarray(camera[k], dtype=np.float64)[..., :3]).to(dtype) for k in ("eye", "at", "up"))
    z = po._normalize(eye - at)
    x = po._normalize(torch.cross(po._normalize(up), z, dim=-1))
    y = torch.cross(z, x, dim=-1)
    return torch.stack((x, y, z), dim=-1), eye


def lift(depth, camera: Mapping, frame="world", grid="numpy"):
    """depth [B, N] (or [B, H, W], [B, H, W, 1]) -> [B, N, 3] in depth's dtype, on its device."""
    W, H = po.frame(camera)
    B = depth.shape[0]
    dt, dev = depth.dtype, depth.device
    f = float(camera["focal_length"])
    gx, gy = pixel_grid(camera, grid)
    x = torch.as_tensor(np.tile(gx, H)).to(dt).to(dev)
    y = torch.as_tensor(np.repeat(gy, W)).to(dt).to(dev)
    d = torch.relu(depth.reshape(B, H * W))
    pos = torch.stack((d * x / f, d * y / f, -d), dim=-1)
    if frame == "camera":
        return pos
    assert frame == "world", frame
    R, eye = camera_to_world(camera, dt)
    return pos @ R.to(dev).transpose(-1, -2) + eye.to(dev)[:, None]


def _c2w_table(eye, at, up):
    z = po._normalize(eye - at)
    x = po._normalize(torch.cross(po._normalize(up), z, dim=-1))
    y = torch.cross(z, x, dim=-1)
    return torch.cat((torch.stack((x, y, z), dim=-1), eye[..., None]), dim=-1)


def magnitudes(inputs, camera: Mapping, upstream, frame="world", grid="numpy"):
    """The sums of the absolute values of the terms of every entry `gradients` returns, and of the camera gradients of
    camera_chain_oracle.lift_gradients (tests/entry_checks.py's A), numpy fp64: ({'pos'}, {'depth'}, {eye, at, up}).
        P_cc           a product and a quotient, no sum: |P_cc|
        P_wc[r]        sum_c |R[r][c]| |P_cc[c]| + |eye_r|
        g_depth        the three-term dot product sum_c A_G[c] |dir_c| with dir = (x_j / f, y_i / f, -1) and, in the
                       world frame, G = R^T g itself a sum, A_G[c] = sum_r |R[r][c]| |g_r|; 0 where depth <= 0
        camera         entry_checks.camera_magnitudes of d loss / d[R | eye]: columns 0-2 sum over the pixels of
                       |g_r| |P_cc[c]|, column 3 sum of |g_r|; zeros in the camera frame, which reads no camera"""
    W, H = po.frame(camera)
    depth = np.asarray(inputs["depth"], np.float64)
    B = depth.shape[0]
    f = float(camera["focal_length"])
    gx, gy = pixel_grid(camera, grid)
    dirs = np.abs(np.stack((np.tile(gx, H) / f, np.repeat(gy, W) / f, -np.ones(H * W)), -1))          # [N, 3]
    d = np.maximum(depth.reshape(B, H * W), 0.0)
    with np.errstate(invalid="ignore"):                      # an infinite depth on the optical axis: inf * 0
        P_cc = d[..., None] * dirs
    g = np.abs(np.asarray(upstream["pos"], np.float64)).reshape(B, H * W, 3)
    cam = {k: np.zeros(np.asarray(camera[k]).shape) for k in ("eye", "at", "up")}
    if frame == "camera":
        A_pos, A_G = P_cc, g
    else:
        R, eye = (t.numpy() for t in camera_to_world(camera))
        A_pos = np.einsum("brc,bnc->bnr", np.abs(R), P_cc) + np.abs(eye)[:, None]
        A_G = np.einsum("brc,bnr->bnc", np.abs(R), g)
        A_M = np.concatenate((np.einsum("bnr,bnc->brc", g, P_cc), g.sum(1)[..., None]), -1)
        import entry_checks
        cam = entry_checks.camera_magnitudes([(_c2w_table, A_M)], camera)
    A_depth = np.where(depth.reshape(B, H * W) <= 0, 0.0, np.einsum("bnc,nc->bn", A_G, dirs))       # a NaN depth is not <= 0
    return {"pos": A_pos}, {"depth": A_depth.reshape(depth.shape)}, cam


def gradients(inputs, camera: Mapping, upstream, frame="world", grid="numpy", wrt=INPUTS):
    """({'pos': [B, N, 3]}, {'depth': like the input}) in fp64 for loss = sum(pos * upstream['pos'])."""
    return po.autograd(lambda x: {"pos": lift(x["depth"], camera, frame, grid)}, inputs, INPUTS, upstream, wrt)
