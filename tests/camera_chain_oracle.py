"""fp64 restatement of the depth lift and the two surfel warps with the camera's eye, at and up as autograd leaves: what
depth_to_surfels, projection_renderer_differentiable_fast and projection_reverse_renderer compute under
camera_grad=True.  In the reference the same calls are differentiable in the camera because world_to_cam_batched and
cam_to_world_batched (diffrend/torch/utils.py:567-647) build their matrices with torch ops through lookat / lookat_inv
(:376-427).  Test infrastructure: tests/test_camera_chain_oracle_cpu.py shows that with the camera detached this module
gives exactly what surfels_oracle, projection_oracle and reverse_projection_oracle give; tests/test_hip_camera_warp.py
compares the kernels' camera gradients with it.

Those three modules convert the camera with np.asarray (the camera is data there), so the camera path -- the matrices,
and the functions that call them -- is restated here; every tensor-in piece (lookat, _normalize, _oit, blur, sample, the
pixel grid) is theirs by import, in the same order of operations, so the values agree bit for bit.

A camera entry may be an array or a tensor ([B, 3] or [B, 4]); the w column is dropped before lookat, as the batched
reference functions drop it, so it gets a zero gradient.  `dtype` and `device` follow the inputs: tools/
bench_camera_warp.py times this composition in float32 on the GPU."""
from typing import Dict, Mapping, Optional

import numpy as np
import torch

import projection_oracle as po
import reverse_projection_oracle as ro
import surfels_oracle as so

CAMERA_KEYS = ("eye", "at", "up")


def vector(camera: Mapping, k: str, dtype):
    """camera[k] without its w column, as a tensor of `dtype`; a tensor stays attached to its leaf."""
    v = camera[k]
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))
    return t[..., :3].to(dtype)


def world_to_camera(camera: Mapping, dtype):
    """[B, 4, 4]: lookat(eye, at, up)."""
    return po.lookat(*(vector(camera, k, dtype) for k in CAMERA_KEYS))


def camera_to_world(camera: Mapping, dtype):
    """[B, 3, 3] rotation (columns x, y, z) and [B, 3] eye: lookat_inv(eye, at, up)."""
    eye, at, up = (vector(camera, k, dtype) for k in CAMERA_KEYS)
    z = po._normalize(eye - at)
    x = po._normalize(torch.cross(po._normalize(up), z, dim=-1))
    y = torch.cross(z, x, dim=-1)
    return torch.stack((x, y, z), dim=-1), eye


def lift(depth, camera: Mapping, frame="world", grid="numpy"):
    """surfels_oracle.lift with a camera that may hold tensors."""
    W, H = po.frame(camera)
    B = depth.shape[0]
    dt, dev = depth.dtype, depth.device
    f = float(camera["focal_length"])
    gx, gy = so.pixel_grid(camera, grid)
    x = torch.as_tensor(np.tile(gx, H)).to(dt).to(dev)
    y = torch.as_tensor(np.repeat(gy, W)).to(dt).to(dev)
    d = torch.relu(depth.reshape(B, H * W))
    pos = torch.stack((d * x / f, d * y / f, -d), dim=-1)
    if frame == "camera":
        return pos
    assert frame == "world", frame
    R, eye = camera_to_world(camera, dt)
    return pos @ R.to(dev).transpose(-1, -2) + eye.to(dev)[:, None]


def pixel_coordinates(surfels, camera: Mapping):
    """projection_oracle.pixel_coordinates with a camera that may hold tensors."""
    dt, dev = surfels.dtype, surfels.device
    view = world_to_camera(camera, dt).to(dev)
    W, H = po.frame(camera)
    f, fovy = float(camera["focal_length"]), float(camera["fovy"])
    cc = torch.cat((surfels, torch.ones_like(surfels[..., :1])), dim=-1) @ view.transpose(-1, -2)
    x = f * po.nonzero_divide(cc[..., 0], cc[..., 2])
    y = f * po.nonzero_divide(cc[..., 1], cc[..., 2])
    h = np.tan(fovy / 2) * 2 * f
    w = h * (float(W) / float(H))
    return torch.stack((x * (-(W - 1) / w) + W / 2.0, y * ((H - 1) / h) + H / 2.0, -cc[..., 2]), dim=-1)


def scattered(surfels, rgb, camera: Mapping, use_depth=True, use_center_dist=True, detach_depth_merge=False):
    """projection_oracle.scattered on pixel_coordinates above."""
    W, H = po.frame(camera)
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
        total = total + po._oit(values * beta, depth, cd2, idx, use_depth, use_center_dist)
    total = total.reshape(B, H, W, -1)
    return total[..., :-2], total[..., -2:-1], total[..., -1:], px


def project(surfels, rgb, camera: Mapping, rotated_image=None, blur_size=0.15, use_depth=True, use_center_dist=True,
            compute_new_depth=False, blur_rotated_image=True, detach_mask=False, detach_mask2=False,
            detach_depth_merge=False) -> Dict[str, torch.Tensor]:
    """projection_oracle.project on scattered above."""
    W, H = po.frame(camera)
    B = surfels.shape[0]
    rgb_out, soft_mask, depth_out, _ = scattered(surfels, rgb, camera, use_depth, use_center_dist, detach_depth_merge)
    rgb_out, soft_mask = po.blur(rgb_out, blur_size), po.blur(soft_mask, blur_size)
    nonzero = torch.where(soft_mask > 0, soft_mask, torch.ones_like(soft_mask)) + 1e-20
    image1 = torch.where(soft_mask > 0, rgb_out / nonzero, rgb_out)
    if rotated_image is not None:
        rot = rotated_image.reshape(B, H, W, -1)
        if blur_rotated_image:
            rot = po.blur(rot, blur_size)
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


def reverse_project(rgb, in_pos_wc, out_pos_wc, camera1: Mapping, camera2: Mapping, rotated_image=None,
                    compute_new_depth=False, depth_epsilon=1e-1, keep=None) -> Dict[str, torch.Tensor]:
    """reverse_projection_oracle.depths and .project on pixel_coordinates above."""
    B, H, W, _ = rgb.shape
    assert po.frame(camera1) == po.frame(camera2) == (W, H)
    c1 = pixel_coordinates(out_pos_wc, camera1).reshape(B, H, W, 3)
    c2 = pixel_coordinates(in_pos_wc, camera2).reshape(B, H, W, 3)
    d = c1[..., 2:]
    d_in = ro.sample(d, c2[..., :2])
    d_out = ro.sample(d_in, c1[..., :2])
    image1 = ro.sample(rgb, c1[..., :2])
    outside = (c1[..., 1] < 0.5) | (c1[..., 0] < 0.5) | (c1[..., 1] >= H - 0.5) | (c1[..., 0] >= W - 0.5)
    mask = (1 - outside[..., None].to(rgb.dtype)) * (d <= d_out + depth_epsilon).to(rgb.dtype)
    if keep is not None:
        mask = mask * keep
    res = {"out": image1 if rotated_image is None else mask * image1 + (1 - mask) * rotated_image, "mask": mask,
           "image1": image1}
    if compute_new_depth:
        res["depth"] = ro.sample(c2[..., 2:], c1[..., :2])
    return res


def autograd(fn, inputs: Mapping[str, Optional[np.ndarray]], names, cameras: Mapping[str, Mapping],
             upstream: Mapping[str, np.ndarray], wrt, camera_wrt=CAMERA_KEYS):
    """projection_oracle.autograd with camera leaves: ({output: value}, {input: gradient}, {camera label: {entry:
    gradient in the entry's own shape}}) in fp64, for fn(leaves, {label: camera with its `camera_wrt` entries as
    leaves}) -> {output: tensor}.  A leaf the loss does not depend on gets zeros."""
    leaves = {k: torch.tensor(np.asarray(inputs[k], dtype=np.float64), requires_grad=k in wrt)
              for k in names if inputs.get(k) is not None}
    cam_leaves = {label: {k: torch.tensor(np.asarray(cam[k], dtype=np.float64), requires_grad=True) for k in camera_wrt}
                  for label, cam in cameras.items()}
    res = fn(leaves, {label: dict(cam, **cam_leaves[label]) for label, cam in cameras.items()})
    loss = sum(torch.sum(res[k] * torch.as_tensor(np.asarray(upstream[k], dtype=np.float64)).reshape(res[k].shape))
               for k in res if k in upstream)
    if loss.requires_grad:
        loss.backward()

    def grad(t):
        return t.grad.numpy() if t.grad is not None else np.zeros(t.shape)

    return ({k: v.detach().numpy() for k, v in res.items()}, {k: grad(leaves[k]) for k in wrt if k in leaves},
            {label: {k: grad(t) for k, t in ls.items()} for label, ls in cam_leaves.items()})


def lift_gradients(inputs, camera: Mapping, upstream, frame="world", grid="numpy", wrt=so.INPUTS, camera_wrt=CAMERA_KEYS):
    return autograd(lambda x, c: {"pos": lift(x["depth"], c["camera"], frame, grid)}, inputs, so.INPUTS,
                    {"camera": camera}, upstream, wrt, camera_wrt)


def project_gradients(inputs, camera: Mapping, upstream, blur_size=0.15, wrt=po.INPUTS, camera_wrt=CAMERA_KEYS, **flags):
    return autograd(lambda x, c: project(x["surfels"], x["rgb"], c["camera"], x.get("rotated_image"), blur_size, **flags),
                    inputs, po.INPUTS, {"camera": camera}, upstream, wrt, camera_wrt)


def reverse_gradients(inputs, camera1: Mapping, camera2: Mapping, upstream, wrt=ro.INPUTS, camera_wrt=CAMERA_KEYS,
                      **flags):
    if flags.get("keep") is not None:
        flags = dict(flags, keep=torch.as_tensor(np.asarray(flags["keep"], dtype=np.float64)))
    return autograd(lambda x, c: reverse_project(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], c["camera1"], c["camera2"],
                                                 x.get("rotated_image"), **flags),
                    inputs, ro.INPUTS, {"camera1": camera1, "camera2": camera2}, upstream, wrt, camera_wrt)


def chain_gradients(depth, rgb, camera_a: Mapping, camera_b: Mapping, upstream_out, blur_size=0.15, round_pos=True,
                    **flags):
    """depth lifted by camera_a, projected into camera_b, loss = sum(out * upstream_out): ({'out'}, {'depth', 'rgb'},
    {'camera_a', 'camera_b'}).  `round_pos`: the surfels between the two layers are rounded to float32, as the layers
    hand them on (the rounding passes the gradient through unchanged), so that the second layer of the restatement
    starts from the fp32 inputs the second kernel starts from."""
    def fn(x, c):
        pos = lift(x["depth"], c["camera_a"])
        if round_pos:
            pos = pos + (pos.detach().float().double() - pos.detach())
        return {"out": project(pos, x["rgb"], c["camera_b"], None, blur_size, **flags)["out"]}

    return autograd(fn, {"depth": depth, "rgb": rgb}, ("depth", "rgb"), {"camera_a": camera_a, "camera_b": camera_b},
                    {"out": upstream_out}, ("depth", "rgb"))
