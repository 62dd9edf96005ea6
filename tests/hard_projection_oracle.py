"""fp64 restatement of the reference's hard scatter-mean projection, projection_renderer (diffrend/torch/
projection_layer.py:88-106 with project_image_coordinates :45-85 and scatter_mean_dim0 torch/utils.py:146-175), in torch
on the CPU, so that autograd supplies the gradient oracle.  Test infrastructure: tests/test_hard_projection_oracle_cpu.py
pins it to the reference's own results (tests/golden/hard_projection/hp1_*.npz), tests/test_hip_hard_projection.py
compares the kernels with it.

    pixel coordinate (px, py) of a surfel: projection_oracle.pixel_coordinates (Z = 0 divided by 1, a surfel behind the
    camera projected like any other)
    pixel = round(px - 1/2, py - 1/2), ties to even; index = y W + x, or N (dropped) outside the frame, for a NaN, or
    beyond an int64
    out[q] = sum of the values with index q / their count, 0 where the count is 0;  mask[q] = count[q] == 0

It keeps the reference's formulation -- scatter-adds of values and of ones -- and not the kernels' gather.  `dtype` and
`device` follow the inputs: tools/bench_depth_reprojection.py times this composition in float32 on the GPU."""
from typing import Mapping

import numpy as np
import torch

import projection_oracle as po

INPUTS = ("surfels", "rgb")
OUTPUTS = ("out",)


def pixel_index(surfels, camera: Mapping):
    """[B, N] int64: each surfel's pixel index, N for a dropped surfel; and the pixel coordinates [B, N, 3]."""
    W, H = po.frame(camera)
    px = po.pixel_coordinates(surfels, camera)
    r = torch.round(px[..., :2] - 0.5)
    inside = (r[..., 0] >= 0) & (r[..., 0] <= W - 1) & (r[..., 1] >= 0) & (r[..., 1] <= H - 1)      # NaN fails
    r = torch.where(inside[..., None], r, torch.zeros_like(r)).long()
    return torch.where(inside, r[..., 1] * W + r[..., 0], torch.full_like(r[..., 0], W * H)), px


def project(surfels, rgb, camera: Mapping):
    """{'out': like rgb, 'mask': bool like rgb (True where no surfel landed), 'count': [B, N] int64, 'index': [B, N]}."""
    B, N = surfels.shape[:2]
    idx, _ = pixel_index(surfels.detach(), camera)
    x = rgb.reshape(B, N, -1)
    D = x.shape[-1]
    total = torch.zeros((B, N + 1, D), dtype=x.dtype, device=x.device).scatter_add(1, idx[..., None].expand(B, N, D), x)
    count = torch.zeros((B, N + 1), dtype=x.dtype, device=x.device).scatter_add(1, idx, torch.ones_like(x[..., 0]))
    total, count = total[:, :-1], count[:, :-1]
    out = total / torch.where(count > 0, count, torch.ones_like(count))[..., None]
    return {"out": out.reshape(rgb.shape), "mask": (count == 0)[..., None].expand(B, N, D).reshape(rgb.shape),
            "count": count.long(), "index": idx}


def kink_margin(surfels, camera: Mapping) -> float:
    """How far a case is from its nearest kink, fp64: the smallest of the distance of any pixel-coordinate component from
    an integer (where round(. - 1/2) ties) over 1e-4, and |Z| over 1e-3.  A case is clear when the result is >= 1."""
    px = po.pixel_coordinates(torch.as_tensor(np.asarray(surfels, dtype=np.float64)), camera)
    uv = px[..., :2]
    return min(float((uv - torch.round(uv)).abs().min()) / 1e-4, float(px[..., 2].abs().min()) / 1e-3)


def magnitudes(inputs, camera: Mapping, upstream):
    """The sums of the absolute values of the terms of every entry `gradients` returns (tests/entry_checks.py's A), numpy
    fp64: ({'out': (sum of |v| over the pixel's surfels) / count, 0 for an empty pixel}, {'rgb': |g_out| of the surfel's
    pixel / count -- one term --, 0 for a dropped surfel}).  The index is the oracle's own."""
    surfels = torch.as_tensor(np.asarray(inputs["surfels"], dtype=np.float64))
    rgb = np.abs(np.asarray(inputs["rgb"], np.float64))
    B, N = surfels.shape[:2]
    idx = pixel_index(surfels, camera)[0].numpy()
    x, g = rgb.reshape(B, N, -1), np.abs(np.asarray(upstream["out"], np.float64)).reshape(B, N, -1)
    total, count = np.zeros((B, N + 1, x.shape[-1])), np.zeros((B, N + 1))
    for b in range(B):
        np.add.at(total[b], idx[b], x[b])
        np.add.at(count[b], idx[b], 1.0)
    count[:, N] = 1.0
    safe = np.where(count > 0, count, 1.0)
    g_rgb = np.concatenate((g, np.zeros((B, 1, g.shape[-1]))), 1)[np.arange(B)[:, None], idx] / safe[np.arange(B)[:, None], idx, None]
    return {"out": (total / safe[..., None])[:, :N].reshape(rgb.shape)}, {"rgb": g_rgb.reshape(rgb.shape)}


def gradients(inputs, camera: Mapping, upstream, wrt=("rgb",)):
    """({'out', 'mask', 'count', 'index'}, {'rgb': like the input}) in fp64 for loss = sum(out * upstream['out'])."""
    return po.autograd(lambda x: project(x["surfels"], x["rgb"], camera), inputs, INPUTS, upstream, wrt)
