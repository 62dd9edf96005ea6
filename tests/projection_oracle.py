"""fp64 restatement of the reference's surfel re-projection layer, projection_renderer_differentiable_fast
(diffrend/torch/projection_layer.py:170-278 with project_image_coordinates :45-85, scatter_weighted_blended_oit
torch/utils.py:178-215, blur :155-167 and lookat torch/utils.py:376-427), in torch on the CPU, so that autograd
supplies the gradient oracle.  Test infrastructure: tests/test_projection_oracle_cpu.py pins it to the reference's
own float32 results (tests/golden/projection/pr1_*.npz), tests/test_hip_projection.py compares the kernels with it.

It keeps the reference's formulation -- four scatter-adds per quantity, dense convolutions -- and not the kernels'
gather, so the two are independent statements of the same function.  `dtype` and `device` exist for tools/
bench_projection.py, which times this composition in float32 on the GPU."""
import math
from typing import Dict, Mapping, Optional

import numpy as np
import torch

OUTPUTS = ("out", "mask", "image1", "depth")
INPUTS = ("surfels", "rgb", "rotated_image")
FLAGS = ("use_depth", "use_center_dist", "compute_new_depth", "blur_rotated_image", "detach_mask", "detach_mask2",
         "detach_depth_merge")
SIGMA, Z_SCALE = 0.5, 2.0          # scatter_weighted_blended_oit's defaults, which the layer never overrides


def nonzero_divide(x, y, epsilon=0.0):
    mask = (y.abs() > 0).to(y.dtype)
    return x / (y * mask + (1 - mask) + epsilon)


def _normalize(u):
    return nonzero_divide(u, torch.sqrt(torch.sum(u * u + 1e-10, dim=-1, keepdim=True)))


def lookat(eye, at, up):
    """[B, 3] each -> [B, 4, 4], the inverse of [x y z eye; 0 0 0 1]."""
    z = _normalize(eye - at)
    x = _normalize(torch.cross(_normalize(up), z, dim=-1))
    y = torch.cross(z, x, dim=-1)
    top = torch.cat((torch.stack((x, y, z), dim=-1), eye[..., None]), dim=-1)
    row = torch.zeros((eye.shape[0], 1, 4), dtype=eye.dtype, device=eye.device)
    row[..., 3] = 1
    return torch.linalg.inv(torch.cat((top, row), dim=-2))


def frame(camera: Mapping):
    vp = np.asarray(camera["viewport"]).reshape(-1)
    return int(vp[2] - vp[0]), int(vp[3] - vp[1])


def pixel_coordinates(surfels, camera: Mapping):
    """[B, N, 3] world -> [B, N, 3]: the pixel coordinate (x, y) and the depth -Z (project_image_coordinates)."""
    dt, dev = surfels.dtype, surfels.device
    eye, at, up = (torch.as_tensor(np.asarray(camera[k], dtype=np.float64)[..., :3]).to(dt) for k in ("eye", "at", "up"))
    view = lookat(eye, at, up).to(dev)                  # the camera is data: its matrix is made on the host
    W, H = frame(camera)
    f, fovy = float(camera["focal_length"]), float(camera["fovy"])
    cc = torch.cat((surfels, torch.ones_like(surfels[..., :1])), dim=-1) @ view.transpose(-1, -2)
    x = f * nonzero_divide(cc[..., 0], cc[..., 2])
    y = f * nonzero_divide(cc[..., 1], cc[..., 2])
    h = np.tan(fovy / 2) * 2 * f
    w = h * (float(W) / float(H))
    return torch.stack((x * (-(W - 1) / w) + W / 2.0, y * ((H - 1) / h) + H / 2.0, -cc[..., 2]), dim=-1)


def _oit(x, z, center_dist_2, idx, use_depth, use_center_dist):
    """scatter_weighted_blended_oit: x [B, N, C], idx [B, N] in 0..N with N the dump slot -> [B, N, C]."""
    B, N, C = x.shape
    alpha = (1 / (2 * np.pi * SIGMA ** 2) * torch.exp(-center_dist_2 / (2 * SIGMA ** 2)))[..., None] if use_center_dist else 1
    w = (torch.exp(-Z_SCALE * z) if use_depth else torch.ones_like(z))[..., None]
    num = torch.zeros((B, N + 1, C), dtype=x.dtype, device=x.device).scatter_add(1, idx[..., None].expand(B, N, C), x * alpha * w)
    den = torch.zeros((B, N + 1, 1), dtype=x.dtype, device=x.device).scatter_add(1, idx[..., None], alpha * w)
    return nonzero_divide(num, den, epsilon=1e-8)[:, :-1]


def blur_kernel(blur_size: float, height: int, dtype=torch.float64, device="cpu"):
    sigma = blur_size * height / 6
    half = math.floor(sigma * 3)
    k = torch.exp(-torch.arange(-half, half + 1, device=device).to(dtype) ** 2 / (2 * sigma ** 2))
    return half, k / k.sum()


def blur(image, blur_size: float):
    """[B, H, W, C] -> the same, blurred along both axes with zero padding; sigma follows the HEIGHT (image.size(-2) of
    the reference's NCHW tensor)."""
    B, H, W, C = image.shape
    half, k = blur_kernel(blur_size, H, image.dtype, image.device)
    x = image.permute(0, 3, 1, 2).reshape(B * C, 1, H, W)
    x = torch.nn.functional.conv2d(x, k.view(1, 1, 1, -1), padding=(0, half))
    x = torch.nn.functional.conv2d(x, k.view(1, 1, -1, 1), padding=(half, 0))
    return x.reshape(B, C, H, W).permute(0, 2, 3, 1)


def scattered(surfels, rgb, camera: Mapping, use_depth=True, use_center_dist=True, detach_depth_merge=False):
    """The pre-blur value [B, H, W, D], mask and depth [B, H, W, 1], and the pixel coordinates."""
    W, H = frame(camera)
    B, N = surfels.shape[:2]
    px = pixel_coordinates(surfels, camera)
    cell = torch.floor(px[..., :2] - 0.5).long()
    x = ((px[..., 0] - 0.5) - cell[..., 0].to(px.dtype))[..., None]
    y = ((px[..., 1] - 0.5) - cell[..., 1].to(px.dtype))[..., None]
    depth = px[..., 2].detach() if detach_depth_merge else px[..., 2]
    cd2 = (x ** 2 + y ** 2)[..., 0]
    values = torch.cat((rgb.reshape(B, N, -1), torch.ones_like(x), depth[..., None]), dim=-1)
    total = 0
    for (dx, dy), beta in (((0, 0), (1 - x) * (1 - y)), ((0, 1), (1 - x) * y), ((1, 0), x * (1 - y)), ((1, 1), x * y)):
        qx, qy = cell[..., 0] + dx, cell[..., 1] + dy
        off = (qy < 0) | (qx < 0) | (qy >= H) | (qx >= W)
        idx = torch.where(off, torch.full_like(qx, W * H), qy * W + qx)
        total = total + _oit(values * beta, depth, cd2, idx, use_depth, use_center_dist)
    total = total.reshape(B, H, W, -1)
    return total[..., :-2], total[..., -2:-1], total[..., -1:], px


def project(surfels, rgb, camera: Mapping, rotated_image=None, blur_size=0.15, use_depth=True, use_center_dist=True,
            compute_new_depth=False, blur_rotated_image=True, detach_mask=False, detach_mask2=False,
            detach_depth_merge=False) -> Dict[str, torch.Tensor]:
    """{'out', 'mask', 'image1'[, 'depth']} as [B, H, W, .] tensors of the inputs' dtype."""
    W, H = frame(camera)
    B = surfels.shape[0]
    rgb_out, soft_mask, depth_out, _ = scattered(surfels, rgb, camera, use_depth, use_center_dist, detach_depth_merge)
    rgb_out, soft_mask = blur(rgb_out, blur_size), blur(soft_mask, blur_size)
    nonzero = torch.where(soft_mask > 0, soft_mask, torch.ones_like(soft_mask)) + 1e-20
    image1 = torch.where(soft_mask > 0, rgb_out / nonzero, rgb_out)
    if rotated_image is not None:
        rot = rotated_image.reshape(B, H, W, -1)
        if blur_rotated_image:
            rot = blur(rot, blur_size)
        if detach_mask:
            out = torch.where(soft_mask > 1, rgb_out / nonzero.detach(), rgb_out + rot * (1 - soft_mask.detach()))
        elif detach_mask2:
            out = soft_mask.detach() * image1 + (1 - soft_mask.detach()) * rot
        else:
            out = torch.where(soft_mask > 1, rgb_out / nonzero, rgb_out + rot * (1 - soft_mask))
    else:
        out = image1
    res = {"out": out, "mask": soft_mask, "image1": image1}
    if compute_new_depth:
        res["depth"] = torch.where(soft_mask > 0, depth_out / nonzero, depth_out)
    return res


def decision_margin(surfels, rgb, camera: Mapping, rotated_image=None, blur_size=0.15, **flags) -> float:
    """How far a case is from its nearest kink, fp64: the smallest of
      - the distance of any component of `pixel coordinate - 0.5` from an integer (cell choice, frame bounds), over 1e-4;
      - |Z| over 1e-3;
      - the blurred mask of a pixel that is not exactly 0, over 1e-4;
      - with a rotated image, |blurred mask - 1|, over 1e-4.
    A case is clear when the result is >= 1."""
    surfels = torch.as_tensor(np.asarray(surfels, dtype=np.float64))
    rgb = torch.as_tensor(np.asarray(rgb, dtype=np.float64))
    _, mask, _, px = scattered(surfels, rgb, camera, flags.get("use_depth", True), flags.get("use_center_dist", True))
    mask = blur(mask, blur_size)
    uv = px[..., :2] - 0.5
    worst = [float((uv - torch.round(uv)).abs().min()) / 1e-4, float(px[..., 2].abs().min()) / 1e-3]
    if bool((mask != 0).any()):
        worst.append(float(mask[mask != 0].abs().min()) / 1e-4)
    if rotated_image is not None:
        worst.append(float((mask - 1).abs().min()) / 1e-4)
    return min(worst)


def autograd(fn, inputs: Mapping[str, Optional[np.ndarray]], names, upstream: Mapping[str, np.ndarray], wrt):
    """({output: value}, {input: d loss / d input}) in fp64 for loss = sum over the outputs present in `upstream` of
    sum(output * upstream[output]), with fn(leaves) -> {output: tensor} and leaves the inputs among `names` that are
    there; arrays keep the inputs' shapes.  An input the loss does not depend on gets zeros."""
    leaves = {k: torch.tensor(np.asarray(inputs[k], dtype=np.float64), requires_grad=k in wrt)
              for k in names if inputs.get(k) is not None}
    res = fn(leaves)
    loss = sum(torch.sum(res[k] * torch.as_tensor(np.asarray(upstream[k], dtype=np.float64)).reshape(res[k].shape))
               for k in res if k in upstream)
    if loss.requires_grad:
        loss.backward()
    return ({k: v.detach().numpy() for k, v in res.items()},
            {k: (leaves[k].grad.numpy() if leaves[k].grad is not None else np.zeros(leaves[k].shape))
             for k in wrt if k in leaves})


def gradients(inputs, camera: Mapping, upstream, blur_size=0.15, wrt=INPUTS, **flags):
    """autograd() of project(): outputs as [B, H, W, .]."""
    return autograd(lambda x: project(x["surfels"], x["rgb"], camera, x.get("rotated_image"), blur_size, **flags),
                    inputs, INPUTS, upstream, wrt)
