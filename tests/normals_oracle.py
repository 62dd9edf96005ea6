"""fp64 restatement of the plane-fit layer, estimate_surface_normals_plane_fit_batched (diffrend/torch/utils.py:926-963,
with grad_spatial2d_batched's reflected 3 x 3 differences and normalize's eps), in torch on the CPU, so that autograd
supplies the gradient oracle.  Test infrastructure: tests/test_normals_oracle_cpu.py pins it to the reference's own
results (tests/golden/normals/nm1_*.npz) and to tests/splat_oracle.plane_fit_normals, tests/test_hip_normals.py compares
the kernels with it.

    u_k = (P_k - P_c) / sqrt(sum((P_k - P_c)^2 + 1e-10))       the 8 neighbours of the reflected stencil, dy-major
    a = sum ux^2, b = sum ux uy, d = sum uy^2, r = -(sum ux uz, sum uy uz)
    (nx, ny) = adj([[a, b], [b, d]]) r / (a d - b^2 + 1e-12),  n = unit(nx, ny, 1)
    frame = 'world': R n with [x y z] = R the camera's lookat basis (cam_to_world_batched(None, n, camera)['normal'])

`dtype` and `device` follow pos: tools/bench_normals.py times this composition in float32 on the GPU."""
from typing import Mapping, Optional

import numpy as np
import torch

import projection_oracle as po
import surfels_oracle as so

INPUTS = ("pos",)
OUTPUTS = ("normal",)


def _unit(v):
    return v / torch.sqrt(torch.sum(v * v + 1e-10, dim=-1, keepdim=True))


def reflect_index(n: int, device="cpu"):
    """The indices of a reflected pad of one sample at either end of an axis of n >= 2 samples: 1, 0 .. n - 1, n - 2."""
    i = torch.arange(-1, n + 1, device=device).abs()
    return torch.where(i > n - 1, 2 * (n - 1) - i, i)


def neighbour_units(pos):
    """[B, H, W, 3] -> u [8, B, H, W, 3]."""
    H, W = pos.shape[1:3]
    padded = pos[:, reflect_index(H, pos.device)][:, :, reflect_index(W, pos.device)]
    return _unit(torch.stack([padded[:, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] - pos
                              for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], dim=0))


def moments(pos):
    """(a, b, d, r0, r1, a d - b^2 + 1e-12), each [B, H, W]."""
    u = neighbour_units(pos)
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    a, b, d = torch.sum(ux * ux, 0), torch.sum(ux * uy, 0), torch.sum(uy * uy, 0)
    r0, r1 = -torch.sum(ux * uz, 0), -torch.sum(uy * uz, 0)
    return a, b, d, r0, r1, a * d - b * b + 1e-12


def rotation(camera: Mapping, B: int, dtype=torch.float64):
    """[B, 3, 3], columns x, y, z; eye / at / up per view or shared."""
    cam = {k: np.asarray(camera[k], dtype=np.float64) for k in ("eye", "at", "up")}
    cam = {k: (np.tile(v, (B, 1)) if v.ndim == 1 else v) for k, v in cam.items()}
    return so.camera_to_world(cam, dtype)[0]


def plane_fit(pos, camera: Optional[Mapping] = None, frame="camera"):
    """pos [B, H, W, 3] (or [B, N, 3] with the camera's viewport) -> normals in pos's shape, dtype and device."""
    shape = pos.shape
    if pos.dim() == 3:
        W, H = po.frame(camera)
        pos = pos.reshape(shape[0], H, W, 3)
    a, b, d, r0, r1, det = moments(pos)
    nx = (d * r0 - b * r1) / det
    ny = (a * r1 - b * r0) / det
    n = _unit(torch.stack((nx, ny, torch.ones_like(nx)), dim=-1))
    if frame == "world":
        R = rotation(camera, shape[0], pos.dtype).to(pos.device)
        n = (n.reshape(shape[0], -1, 3) @ R.transpose(-1, -2))
    else:
        assert frame == "camera", frame
    return n.reshape(shape)


def gradients(inputs, camera: Optional[Mapping], upstream, frame="camera", wrt=INPUTS):
    """({'normal': like pos}, {'pos': like pos}) in fp64 for loss = sum(normal * upstream['normal'])."""
    return po.autograd(lambda x: {"normal": plane_fit(x["pos"], camera, frame)}, inputs, INPUTS, upstream, wrt)


def turned_gradients(inputs, camera: Optional[Mapping], upstream, frame="camera", shape=None):
    """`gradients` evaluated on the map turned by 180 degrees and turned back: the turn maps the reflected stencil onto
    itself, so this is the same function with every sum over the neighbours run in the reverse order.  `shape` (B, H, W)
    is needed for points given as [B, N, 3].  Where the two evaluations differ, the difference is the restatement's own
    fp64 rounding, amplified by the cancelling determinant (tests/entry_checks.ill_conditioned)."""
    pos = np.asarray(inputs["pos"])
    B, H, W = shape if shape is not None else pos.shape[:3]

    def turn(a):
        return np.ascontiguousarray(np.asarray(a).reshape(B, H, W, 3)[:, ::-1, ::-1])

    cam = None if camera is None else dict(camera, viewport=[0, 0, W, H])
    v, g = gradients({"pos": turn(pos)}, cam, {k: turn(u) for k, u in upstream.items()}, frame)
    return {k: turn(a).reshape(pos.shape) for k, a in v.items()}, {k: turn(a).reshape(pos.shape) for k, a in g.items()}


def camera_magnitudes(inputs, camera: Mapping, upstream, shape, carried: float):
    """{eye, at, up: A} of the world frame's camera gradients (tests/entry_checks.py).  out = R n, so d loss / dR[r][c] is
    the fp64 sum over the pixels of g_r n_c with n the camera-frame normal, and entry_checks.camera_magnitudes chains
    A_R[r][c] = sum |g_r| (|n_c| + carried) to eye / at / up through lookat_inv's Jacobian.  `carried` is what the
    forward's own floor is in units of the standing 2^-40: n is known to NORMALS_C64 max|n| = NORMALS_C64 and not to
    2^-53 of its terms, and every derived A carries that.  A camera shared by the views ([3] vectors) gets the sum."""
    import entry_checks
    B, H, W = shape
    pos = torch.as_tensor(np.asarray(inputs["pos"], np.float64)).reshape(B, H, W, 3)
    n = plane_fit(pos).abs().numpy().reshape(B, H * W, 3)
    g = np.abs(np.asarray(upstream["normal"], np.float64)).reshape(B, H * W, 3)
    A_M = np.zeros((B, 3, 4))
    A_M[..., :3] = np.einsum("bqr,bqc->brc", g, n + carried)
    shared = np.asarray(camera["eye"]).ndim == 1
    cam = {k: (np.tile(np.asarray(camera[k], np.float64)[:3], (B, 1)) if shared else np.asarray(camera[k], np.float64))
           for k in ("eye", "at", "up")}
    A = entry_checks.camera_magnitudes([(so._c2w_table, A_M)], cam)
    return {k: (a.sum(0) if shared else a) for k, a in A.items()}
