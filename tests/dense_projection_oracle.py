"""fp64 restatement of the reference's dense Gaussian re-projection, projection_renderer_differentiable (diffrend/torch/
projection_layer.py:108-152 with project_image_coordinates :45-85), in torch on the CPU, so that autograd supplies the
gradient oracle.  Test infrastructure: tests/test_dense_projection_oracle_cpu.py pins it to the reference's own results
(tests/golden/dense_projection/dp1_*.npz), tests/test_hip_dense_projection.py compares the kernels with it.

It keeps the reference's DENSE formulation -- the full [B, P, N] weight and one matrix product -- and not the kernels'
separable tiles, so the two are independent statements of the same function; `project_separable` is the other form, for
the CPU test that the two agree.  The projection is tests/projection_oracle.py's pixel_coordinates.  `dtype` and
`device` follow the inputs: tools/bench_dense_projection.py times this composition in float32 on the GPU.

With a rotated image the reference's own line raises (it multiplies [B, N, D] by [B, N]); the restatement broadcasts
the mask over the channels, out = S + rotated (1 - mask)[..., None], as surf_renderer_amd/dense_projection.py does."""
from typing import Dict, Mapping

import numpy as np
import torch

from projection_oracle import autograd, frame, pixel_coordinates

OUTPUTS = ("out", "mask")
INPUTS = ("surfels", "rgb", "rotated_image")

# what the wrong-constant check of tests/test_dense_projection_oracle_cpu.py turns: all off = the reference
WRONG = ("sigma_from_height", "no_half_pixel", "scale_by_width")


def sigma_of(rgb_shape, blur_size: float) -> float:
    """blur_size * rgb.size(-2) / 6: the WIDTH for [B, H, W, D] input and the SURFEL COUNT for [B, N, D] input."""
    return blur_size * rgb_shape[-2] / 6


def _coordinates(surfels, camera, wrong=()):
    px = pixel_coordinates(surfels, camera)
    if "scale_by_width" in wrong:           # W instead of W - 1 (and H instead of H - 1) in the pixel scale
        W, H = frame(camera)
        px = torch.stack(((px[..., 0] - W / 2.0) * (W / (W - 1.0)) + W / 2.0,
                          (px[..., 1] - H / 2.0) * (H / (H - 1.0)) + H / 2.0, px[..., 2]), dim=-1)
    return px


def project(surfels, rgb, camera: Mapping, rotated_image=None, blur_size=0.15, wrong=()) -> Dict[str, torch.Tensor]:
    """{'out': like rgb, 'mask': [*rgb.shape[:-1], 1]} of the inputs' dtype; every surfel weighs on every pixel."""
    W, H = frame(camera)
    B, N = surfels.shape[:2]
    px = _coordinates(surfels, camera, wrong)
    half = 0.0 if "no_half_pixel" in wrong else 0.5
    gy, gx = torch.meshgrid(torch.arange(H, dtype=px.dtype, device=px.device) + half,
                            torch.arange(W, dtype=px.dtype, device=px.device) + half, indexing="ij")
    sigma = sigma_of((H, 0) if "sigma_from_height" in wrong and rgb.dim() == 4 else rgb.shape, blur_size)
    dx = px[:, None, :, 0] - gx.reshape(1, -1, 1)                   # [B, P, N]
    dy = px[:, None, :, 1] - gy.reshape(1, -1, 1)
    scale = torch.exp((-dx ** 2 - dy ** 2) / (2 * sigma ** 2))
    mask = scale.sum(-1)                                             # [B, P]
    S = scale @ rgb.reshape(B, N, -1)                                # [B, P, D]
    if rotated_image is not None:
        out = S + rotated_image.reshape(B, N, -1) * (1 - mask)[..., None]
    else:
        out = S / (mask + 1e-10)[..., None]
    return {"out": out.reshape(rgb.shape), "mask": mask.reshape(*rgb.shape[:-1], 1)}


def project_separable(surfels, rgb, camera: Mapping, rotated_image=None, blur_size=0.15) -> Dict[str, torch.Tensor]:
    """The same function with the weight split into its two factors, ex [B, W, N] and ey [B, H, N]: the kernels' form."""
    W, H = frame(camera)
    B, N = surfels.shape[:2]
    px = pixel_coordinates(surfels, camera)
    h = 1.0 / (2 * sigma_of(rgb.shape, blur_size) ** 2)
    u, v = px[..., 0] - 0.5, px[..., 1] - 0.5
    ex = torch.exp(-(u[:, None, :] - torch.arange(W, dtype=px.dtype)[None, :, None]) ** 2 * h)
    ey = torch.exp(-(v[:, None, :] - torch.arange(H, dtype=px.dtype)[None, :, None]) ** 2 * h)
    values = torch.cat((rgb.reshape(B, N, -1), torch.ones((B, N, 1), dtype=px.dtype)), dim=-1)
    total = torch.einsum("bjn,bin,bnc->bjic", ey, ex, values).reshape(B, H * W, -1)
    S, mask = total[..., :-1], total[..., -1]
    if rotated_image is not None:
        out = S + rotated_image.reshape(B, N, -1) * (1 - mask)[..., None]
    else:
        out = S / (mask + 1e-10)[..., None]
    return {"out": out.reshape(rgb.shape), "mask": mask.reshape(*rgb.shape[:-1], 1)}


def z_margin(surfels, camera: Mapping) -> float:
    """min |Z| over the surfels, fp64: Z = 0 (nonzero_divide's switch) is the layer's one kink."""
    px = pixel_coordinates(torch.as_tensor(np.asarray(surfels, dtype=np.float64)), camera)
    return float(px[..., 2].abs().min())


def gradients(inputs, camera: Mapping, upstream, blur_size=0.15, wrt=INPUTS, fn=project, **kw):
    """projection_oracle.autograd() of `fn`."""
    return autograd(lambda x: fn(x["surfels"], x["rgb"], camera, x.get("rotated_image"), blur_size, **kw),
                    inputs, INPUTS, upstream, wrt)
