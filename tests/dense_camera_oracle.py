"""fp64 restatement of the dense Gaussian re-projection and of the world-frame plane fit with the camera's eye, at and
up as autograd leaves: what projection_renderer_differentiable and estimate_surface_normals_plane_fit_batched(frame=
'world') compute under camera_grad=True.  In the reference the same calls are differentiable in the camera because
world_to_cam_batched and cam_to_world_batched build their matrices with torch ops.  Test infrastructure:
tests/test_dense_camera_oracle_cpu.py shows that with the camera detached this module gives exactly what
dense_projection_oracle and normals_oracle give and that its camera gradients are those of central differences;
tests/test_dense_camera_golden_cpu.py pins it to the reference's own camera gradients; tests/test_hip_dense_camera.py
compares the kernels with it.

Nothing is restated twice.  The dense layer is dense_projection_oracle.project (or project_separable) itself, run while
that module's `pixel_coordinates` is camera_chain_oracle's, which takes a camera that may hold tensors and gives the same
bits for one that holds arrays.  The normals are normals_oracle.plane_fit in the camera frame, rotated by
camera_chain_oracle.camera_to_world's basis.  A camera entry may be an array or a tensor, [B, 3] or [B, 4] (the w column
is dropped before lookat and gets a zero gradient); for the normals also a shared [3] or [4], which gets the sum over
the views."""
from typing import Mapping
from unittest import mock

import numpy as np
import torch

import camera_chain_oracle as co
import dense_projection_oracle as do
import normals_oracle as no
import projection_oracle as po

CAMERA_KEYS = co.CAMERA_KEYS

# what the wrong-rotation check of tests/test_dense_camera_golden_cpu.py turns: all off = the reference
#   raw_up             unit(up) as the y axis instead of z x x (no orthogonalisation)
#   inverse_transpose  R^-T, which the reference applies to a normal, instead of R: equal but for normalize's 1e-10
WRONG_ROTATION = ("raw_up", "inverse_transpose")


def project(surfels, rgb, camera: Mapping, rotated_image=None, blur_size=0.15, fn=do.project, **kw):
    """dense_projection_oracle.project (`fn`: or project_separable) with a camera that may hold tensors."""
    with mock.patch.object(do, "pixel_coordinates", co.pixel_coordinates):
        return fn(surfels, rgb, camera, rotated_image, blur_size, **kw)


def per_view(camera: Mapping, B: int) -> Mapping:
    """The camera with a shared [3] / [4] eye, at or up expanded over the B views (a tensor stays attached)."""
    def expand(v):
        if isinstance(v, torch.Tensor):
            return v[None].expand(B, -1) if v.dim() == 1 else v
        v = np.asarray(v, dtype=np.float64)
        return np.tile(v, (B, 1)) if v.ndim == 1 else v
    return dict(camera, **{k: expand(camera[k]) for k in CAMERA_KEYS})


def rotation(camera: Mapping, B: int, dtype=torch.float64, wrong=()):
    """[B, 3, 3], columns x, y, z: normals_oracle.rotation with a camera that may hold tensors."""
    cam = per_view(camera, B)
    R = co.camera_to_world(cam, dtype)[0]
    if "raw_up" in wrong:
        R = torch.stack((R[..., 0], po._normalize(co.vector(cam, "up", dtype)), R[..., 2]), dim=-1)
    if "inverse_transpose" in wrong:
        R = torch.linalg.inv(R).transpose(-1, -2)
    return R


def plane_fit(pos, camera: Mapping, frame="world", wrong=()):
    """normals_oracle.plane_fit; in the world frame with a camera that may hold tensors."""
    n = no.plane_fit(pos, camera, "camera")
    if frame == "camera":
        return n
    assert frame == "world", frame
    B = pos.shape[0]
    R = rotation(camera, B, pos.dtype, wrong).to(pos.device)
    return (n.reshape(B, -1, 3) @ R.transpose(-1, -2)).reshape(pos.shape)


def project_gradients(inputs, camera: Mapping, upstream, blur_size=0.15, wrt=do.INPUTS, camera_wrt=CAMERA_KEYS,
                      fn=do.project, **kw):
    """(values, gradients, {'camera': camera gradients}) of the dense layer: camera_chain_oracle.autograd."""
    return co.autograd(lambda x, c: project(x["surfels"], x["rgb"], c["camera"], x.get("rotated_image"), blur_size, fn,
                                            **kw),
                       inputs, do.INPUTS, {"camera": camera}, upstream, wrt, camera_wrt)


def normals_gradients(inputs, camera: Mapping, upstream, frame="world", wrt=no.INPUTS, camera_wrt=CAMERA_KEYS, wrong=()):
    """(values, gradients, {'camera': camera gradients}) of the plane fit; the camera frame does not read the camera, so
    its camera gradients are zeros."""
    return co.autograd(lambda x, c: {"normal": plane_fit(x["pos"], c["camera"], frame, wrong)}, inputs, no.INPUTS,
                       {"camera": camera}, upstream, wrt, camera_wrt)


def round_through_float32(t):
    """t rounded to float32 as a layer hands it on; the gradient passes through unchanged."""
    return t + (t.detach().float().double() - t.detach())


def lift_project_gradients(depth, rgb, camera_a: Mapping, camera_b: Mapping, upstream, rotated_image=None, blur_size=0.15):
    """depth lifted by camera_a (world frame), projected densely into camera_b: ({'out', 'mask'}, {'depth', 'rgb'},
    {'camera_a', 'camera_b'})."""
    def fn(x, c):
        pos = round_through_float32(co.lift(x["depth"], c["camera_a"]))
        return project(pos, x["rgb"], c["camera_b"], x.get("rotated_image"), blur_size)

    return co.autograd(fn, {"depth": depth, "rgb": rgb, "rotated_image": rotated_image}, ("depth", "rgb", "rotated_image"),
                       {"camera_a": camera_a, "camera_b": camera_b}, upstream, ("depth", "rgb"))


def lift_normals_gradients(depth, camera: Mapping, upstream):
    """depth lifted in the camera frame, normals in the world frame: ({'normal'}, {'depth'}, {'camera'})."""
    def fn(x, c):
        pos = round_through_float32(co.lift(x["depth"], c["camera"], frame="camera"))
        return {"normal": plane_fit(pos, c["camera"], "world")}

    return co.autograd(fn, {"depth": depth}, ("depth",), {"camera": camera}, upstream, ("depth",))
