#!/usr/bin/env python3
"""Generate tests/golden/dense_camera/dc1_*.npz: the reference's OWN camera gradients of

  dense     projection_renderer_differentiable (diffrend/torch/projection_layer.py:108-152), in float64 (the unedited
            function runs in it: ref_harness.precision), on the frames 2x2, 3x5, 12x16 and 17x9 of
            tests/dense_projection_cases.py with rgb as [B, H, W, D] and as [B, N, D], without a rotated image (with one
            the reference's own line raises).  17x9 is recorded with [B, 4] cameras: w = 1 for eye and at, 0 for up.
  normals   cam_to_world_batched(None, estimate_surface_normals_plane_fit_batched(pos), camera)['normal']
            (diffrend/torch/utils.py), in float64 if the unedited functions run in it, else float32, on the cases 2x2,
            3x5, 12x16 and 17x9 of tests/normals_cases.py, every one in the world frame,

imported UNMODIFIED and run on the CPU under autograd with the camera's eye, at and up as leaves that require grad --
the gradient the layers' camera_grad=True gives.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  A case of exactly three views is recorded view by view (ref_harness.run_views).

Stored per fixture: what ref_harness.pack_layer stores (in/<input>, in/camera/<entry>, grad_in/<output>, ref/<output>,
grad/<input>), in/precision, the layer's own in/ keys (dense: in/blur_size), and grad/camera/<eye, at, up> =
d sum_outputs sum(output * grad_in) / d that tensor, in its own shape.  The subfolder keeps the fixtures out of the
top-level globs (the golden drift check, conftest.golden_cases)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import dense_projection_cases as dc  # noqa: E402
import normals_cases as nc  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402

KEYS = ("eye", "at", "up")
DENSE = [(f, layout) for f in ("2x2", "3x5", "12x16", "17x9") for layout in dc.LAYOUTS]
HOMOGENEOUS = ("17x9",)                  # dense frames recorded with [B, 4] cameras
NORMALS = ("2x2", "3x5", "12x16", "17x9")


def homogeneous(camera):
    """eye and at with w = 1, up with w = 0: the reference's conventions for [B, 4] cameras."""
    w = {"eye": 1.0, "at": 1.0, "up": 0.0}
    return dict(camera, **{k: np.concatenate((camera[k], np.full((camera[k].shape[0], 1), w[k], camera[k].dtype)), axis=1)
                           for k in KEYS})


def camera_leaves(camera, dtype):
    cam = R.layer_camera(camera, dtype)
    for k in KEYS:
        cam[k].requires_grad_()
    return cam


def finish(name, c, leaves, camera, res, dtype, extra):
    flat = R.pack_layer(c, leaves, res, dtype=dtype)
    for k in KEYS:
        g = camera[k].grad
        flat[f"grad/camera/{k}"] = g.numpy() if g is not None else np.zeros(tuple(camera[k].shape), flat["ref/" + next(iter(res))].dtype)
        print(f"{name} camera.{k:3s} |grad| max {np.abs(flat[f'grad/camera/{k}']).max():.4g}")
    flat["in/precision"] = np.asarray(str(dtype).replace("torch.", ""))
    flat.update(extra)
    R.write("dc1_" + name, flat)


def dense(frame, layout, dtype=torch.float64):
    c = dc.case(frame, layout)
    if frame in HOMOGENEOUS:
        c = dict(c, camera=homogeneous(c["camera"]))
    leaves = {k: torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("surfels", "rgb")}
    camera = camera_leaves(c["camera"], dtype)

    def run(views):
        with R.quiet(), R.precision(dtype):
            out, mask = ref_projection.projection_renderer_differentiable(
                leaves["surfels"][views], leaves["rgb"][views], R.camera_views(camera, views), rotated_image=None,
                blur_size=c["blur_size"])
        return {"out": out, "mask": mask}

    res = R.run_views(run, c["shape"][0])
    assert all(v.dtype == dtype for v in res.values())
    finish("dense_" + dc.tag(frame, layout), c, leaves, camera, res, dtype,
           {"in/blur_size": np.asarray(c["blur_size"], dtype=np.float64)})


def normals(name, dtype):
    c = dict(nc.case(name), frame="world")
    B, H, W = c["shape"]
    leaves = {"pos": torch.tensor(c["pos"], dtype=dtype, requires_grad=True)}
    camera = camera_leaves(c["camera"], dtype)

    def run(views):
        grid = leaves["pos"][views].reshape(-1, H, W, 3)
        with R.quiet():
            n = R.ref_utils.estimate_surface_normals_plane_fit_batched(grid)
            n = R.ref_utils.cam_to_world_batched(None, n.reshape(-1, H * W, 3), R.camera_views(camera, views))["normal"]
        return {"normal": n.reshape(leaves["pos"][views].shape)}

    with R.precision(dtype):
        res = R.run_views(run, B)
        assert res["normal"].dtype == dtype
        finish("normals_" + name, c, leaves, camera, res, dtype, {"in/frame": np.asarray("world")})


def normals_precision():
    """float64 if the unedited functions run in it, forward and backward, and return float64, else float32."""
    try:
        saved, R.write = R.write, lambda name, flat: None
        try:
            normals("3x5", torch.float64)
        finally:
            R.write = saved
        return torch.float64
    except (RuntimeError, TypeError, AssertionError) as e:
        print(f"float64 run of the normals failed: {e}")
        return torch.float32


if __name__ == "__main__":
    R.OUT = R.fixture_dir("dense_camera")
    for f, layout in DENSE:
        dense(f, layout)
    PRECISION = normals_precision()
    print(f"recording the normals in {PRECISION}")
    for n in NORMALS:
        normals(n, PRECISION)
