"""fp64 restatement of the reference's backward-warp re-projection, projection_reverse_renderer (diffrend/torch/
projection_layer.py:281-333 with project_image_coordinates :45-85), in torch on the CPU, so that autograd supplies the
gradient oracle.  Test infrastructure: tests/test_reverse_projection_oracle_cpu.py pins it to the reference's own
float32 results (tests/golden/reverse_projection/rp1_*.npz), tests/test_hip_reverse_projection.py compares the kernels
with it.

It keeps the reference's formulation -- four F.grid_sample calls on NCHW tensors with normalised coordinates, bilinear,
zero padding, align_corners=False (the defaults of the torch the reference's results were recorded under, spelled out)
-- and not the kernels' per-texel gather, so the two are independent statements of the same function.  `dtype` and
`device` follow the inputs: tools/bench_reverse_projection.py times this composition in float32 on the GPU."""
from typing import Dict, Mapping

import numpy as np
import torch
import torch.nn.functional as F

from projection_oracle import autograd, frame, pixel_coordinates

OUTPUTS = ("out", "mask", "image1", "depth")
INPUTS = ("rgb", "in_pos_wc", "out_pos_wc", "rotated_image")
ALIGN_CORNERS = False


def sample(image, px):
    """image [B, H, W, C] sampled at the pixel coordinates px [B, H, W, 2] -> [B, H, W, C], as the reference does it."""
    B, H, W, _ = image.shape
    grid = px / torch.tensor([W, H], dtype=px.dtype, device=px.device) * 2 - 1
    return F.grid_sample(image.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros",
                         align_corners=ALIGN_CORNERS).permute(0, 2, 3, 1)


def depths(in_pos_wc, out_pos_wc, camera1: Mapping, camera2: Mapping):
    """(c1, c2, d, d_out): the two projections [B, H, W, 3], the depth in camera 1 and the twice-resampled one."""
    W, H = frame(camera1)
    assert frame(camera2) == (W, H)
    B = out_pos_wc.shape[0]
    c1 = pixel_coordinates(out_pos_wc, camera1).reshape(B, H, W, 3)
    c2 = pixel_coordinates(in_pos_wc, camera2).reshape(B, H, W, 3)
    d = c1[..., 2:]
    d_in = sample(d, c2[..., :2])
    return c1, c2, d, sample(d_in, c1[..., :2])


def project(rgb, in_pos_wc, out_pos_wc, camera1: Mapping, camera2: Mapping, rotated_image=None,
            compute_new_depth=False, depth_epsilon=1e-1, keep=None) -> Dict[str, torch.Tensor]:
    """{'out', 'mask', 'image1'[, 'depth']} as [B, H, W, .] tensors of the inputs' dtype.  `keep` [B, H, W, 1] stands
    for the dropout plane F.dropout(ones, p, training=True) the mask is multiplied by."""
    B, H, W, _ = rgb.shape
    c1, c2, d, d_out = depths(in_pos_wc, out_pos_wc, camera1, camera2)
    image1 = sample(rgb, c1[..., :2])
    outside = (c1[..., 1] < 0.5) | (c1[..., 0] < 0.5) | (c1[..., 1] >= H - 0.5) | (c1[..., 0] >= W - 0.5)
    mask = (1 - outside[..., None].to(rgb.dtype)) * (d <= d_out + depth_epsilon).to(rgb.dtype)
    if keep is not None:
        mask = mask * keep
    res = {"out": image1 if rotated_image is None else mask * image1 + (1 - mask) * rotated_image, "mask": mask,
           "image1": image1}
    if compute_new_depth:
        res["depth"] = sample(c2[..., 2:], c1[..., :2])
    return res


def decision_margin(in_pos_wc, out_pos_wc, camera1: Mapping, camera2: Mapping, depth_epsilon=1e-1) -> float:
    """How far a case is from its nearest decision, fp64: the smallest of
      - the distance of any component of `pixel coordinate - 0.5` of either projection from an integer (the bilinear
        cell, the frame, the 0.5-pixel mask bounds), over 1e-4;
      - |Z| of either projection, over 1e-3;
      - |d - d_out - depth_epsilon|, over 1e-4.
    A case is clear when the result is >= 1.  An axis of one pixel is left out of the first: its scale (W - 1) / w is
    exactly 0, so the coordinate is exactly W / 2 in every precision and every formulation (the 1x1 case)."""
    W, H = frame(camera1)
    t = [torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in (in_pos_wc, out_pos_wc)]
    c1, c2, d, d_out = depths(t[0], t[1], camera1, camera2)
    worst = [float((d - d_out - depth_epsilon).abs().min()) / 1e-4]
    for c in (c1, c2):
        worst.append(float(c[..., 2].abs().min()) / 1e-3)
        for axis, size in ((0, W), (1, H)):
            if size > 1:
                uv = c[..., axis] - 0.5
                worst.append(float((uv - torch.round(uv)).abs().min()) / 1e-4)
    return min(worst)


def gradients(inputs, camera1: Mapping, camera2: Mapping, upstream, wrt=INPUTS, **flags):
    """projection_oracle.autograd() of project(): outputs as [B, H, W, .].  The mask is a comparison: a loss on it alone
    depends on nothing."""
    if flags.get("keep") is not None:
        flags = dict(flags, keep=torch.as_tensor(np.asarray(flags["keep"], dtype=np.float64)))
    return autograd(lambda x: project(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], camera1, camera2,
                                      x.get("rotated_image"), **flags), inputs, INPUTS, upstream, wrt)
