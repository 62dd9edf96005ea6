"""fp64 torch restatement of the seven geometric regularisers the reference's trainers put on every rendered splat
view (diffrend/torch/GAN/gan.py:601-640; diffrend/torch/utils.py:731-851: grad_spatial2d, spatial_3x3,
depth_rgb_gradient_consistency, normal_consistency_cost with norm = 1, unit_norm2_L2loss, away_from_camera_penalty, and
the z-range penalty and position-variance term the trainers write inline).

One view: pos, normal, image (H, W, 3) and depth (H, W); N = H W; d_k(x) = x[neighbour k] - x[centre] over the 3 x 3
stencil without its centre (dy-major), reflected at the borders:
    z                        mean (s relu(z_min - |p_z|))^2 + (s relu(|p_z| - z_max))^2
    unit_normal              mean (c (|n| - 1))^2
    normal_consistency       mean over the 8 N pairs of |u_k . n|,  u_k = d_k(pos) / sqrt(|d_k|^2 + 3e-10)
    spatial                  mean over the 8 N pairs of sum_c |d_k(pos)_c|
    spatial_var              1 / (var p_x + var p_y + var p_z + 1e-4), unbiased variances
    image_depth_consistency  mean over the 8 N pairs of | |d_k(mean_c image)| - |d_k(depth)| |
    away_from_camera         SUM of relu(-n . c),  c = -p / sqrt(|p|^2 + 3e-10)
Any leading axes are batch axes: every term then has their shape.  Written in this project's own terms; pinned to the
reference by tests/test_regularizer_oracle_cpu.py (tests/golden/regularizers/r1_*.npz, tools/gen_regularizer_golden.py).
The dtype and device are the inputs': fp64 on the CPU in the tests, fp32 on the GPU as tools/bench_regularizers.py's
baseline."""
from typing import Dict, Optional

import numpy as np
import torch

from splat_oracle import _unit

TERMS = ("z", "unit_normal", "normal_consistency", "spatial", "spatial_var", "image_depth_consistency",
         "away_from_camera")
INPUTS = ("pos", "normal", "image", "depth")


def _reflected(n: int, device) -> torch.Tensor:
    i = torch.arange(-1, n + 1, device=device).abs()
    return torch.where(i > n - 1, 2 * (n - 1) - i, i)


def neighbour_differences(x: torch.Tensor) -> torch.Tensor:
    """(..., H, W, C) -> (8, ..., H, W, C): x[neighbour k] - x[centre], dy-major, reflection at the borders."""
    H, W = x.shape[-3], x.shape[-2]
    xp = x.index_select(-3, _reflected(H, x.device)).index_select(-2, _reflected(W, x.device))
    return torch.stack([xp[..., 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx, :] - x
                        for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], dim=0)


def terms(pos, normal, image, depth, z_min: float, z_max: float, z_scale: float = 2.0,
          unit_normal_scale: float = 10.0) -> Dict[str, torch.Tensor]:
    """The seven terms of (..., H, W, 3) pos / normal / image and (..., H, W) depth, each of shape (...)."""
    az = pos[..., 2].abs()
    z = ((z_scale * torch.relu(z_min - az)) ** 2 + (z_scale * torch.relu(az - z_max)) ** 2).mean(dim=(-2, -1))
    unit = ((unit_normal_scale * (torch.sqrt(torch.sum(normal * normal, dim=-1)) - 1)) ** 2).mean(dim=(-2, -1))
    d = neighbour_differences(pos)
    cons = torch.sum(_unit(d) * normal, dim=-1).abs().mean(dim=(0, -2, -1))
    spatial = d.abs().sum(dim=-1).mean(dim=(0, -2, -1))
    flat = pos.reshape(*pos.shape[:-3], -1, 3)
    var = 1.0 / (flat.var(dim=-2, unbiased=True).sum(dim=-1) + 1e-4)
    da = neighbour_differences(image.mean(dim=-1, keepdim=True))
    db = neighbour_differences(depth[..., None])
    idc = (da.abs() - db.abs()).abs().mean(dim=(0, -3, -2, -1))
    away = torch.relu(-torch.sum(normal * -_unit(pos), dim=-1)).sum(dim=(-2, -1))
    return dict(zip(TERMS, (z, unit, cons, spatial, var, idc, away)))


def decision_margin(pos, normal, image, depth, z_min: float, z_max: float, flat: Optional[np.ndarray] = None,
                    skip=()) -> float:
    """The smallest |q| over the quantities q whose sign or clamp a gradient depends on: |a| - |b| of the image /
    depth pair, n . c, u_k . n, |p_z| - z_min, |p_z| - z_max and the components of d_k(pos).  `flat` (H, W) bool marks
    deliberately degenerate pixels: there, and in pairs that touch them, a q that is EXACTLY 0 is the convention under
    test (sign(0) = 0, relu' (0) = 0) and is left out; every other q counts.  One view, fp64 tensors."""
    H, W = depth.shape
    flat = torch.zeros((H, W), dtype=torch.bool) if flat is None else torch.as_tensor(flat)
    pair_flat = flat[None] | _neighbour_values(flat.to(torch.float64)).ne(0)      # centre or neighbour is flat
    d = neighbour_differences(pos)
    az = pos[..., 2].abs()
    qs = {"pair": (neighbour_differences(image.mean(dim=-1, keepdim=True)).abs()
                   - neighbour_differences(depth[..., None]).abs())[..., 0],
          "away": torch.sum(normal * -_unit(pos), dim=-1),
          "consistency": torch.sum(_unit(d) * normal, dim=-1),
          "z_min": az - z_min, "z_max": az - z_max,
          "d": d}
    worst = np.inf
    for k, q in qs.items():
        if k in skip:
            continue
        allowed = pair_flat if q.dim() >= 3 and q.shape[0] == 8 else flat
        if q.dim() == 4:
            allowed = allowed[..., None].expand_as(q)
        keep = ~(allowed & q.eq(0))
        if bool(keep.any()):
            worst = min(worst, float(q[keep].abs().min()))
    return worst


def _neighbour_values(x: torch.Tensor) -> torch.Tensor:
    """(H, W) -> (8, H, W): the neighbours' own values."""
    return neighbour_differences(x[..., None])[..., 0] + x[None]


def gradients(inputs: Dict[str, np.ndarray], weights: np.ndarray, z_min: float, z_max: float, z_scale: float = 2.0,
              unit_normal_scale: float = 10.0, wrt=INPUTS):
    """({term: value}, {input: d loss / d input}) in fp64 for loss = sum_k sum_views weights[..., k] terms[k]; `weights`
    is (7,) or (B, 7) in TERMS order."""
    leaves = {k: torch.tensor(np.asarray(inputs[k], dtype=np.float64), requires_grad=k in wrt) for k in INPUTS}
    out = terms(leaves["pos"], leaves["normal"], leaves["image"], leaves["depth"], z_min, z_max, z_scale,
                unit_normal_scale)
    w = torch.as_tensor(np.asarray(weights, dtype=np.float64))
    loss = sum(torch.sum(w[..., k] * out[name]) for k, name in enumerate(TERMS))
    loss.backward()
    return ({k: v.detach().numpy() for k, v in out.items()},
            {k: leaves[k].grad.numpy() if leaves[k].grad is not None else np.zeros(leaves[k].shape) for k in wrt})
