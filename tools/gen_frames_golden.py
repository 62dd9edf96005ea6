#!/usr/bin/env python3
"""Generate tests/golden/frames/fr1_*.npz: the reference's OWN world_to_cam, world_to_cam_batched, cam_to_world,
cam_to_world_batched (diffrend/torch/utils.py:539-647), project_surfels and project_image_coordinates
(diffrend/torch/projection_layer.py:19-85), imported UNMODIFIED and run on the CPU under autograd, on the seeded cases
tests/frames_cases.py lists as GOLDEN_* -- once in float64 (ref_harness.precision) and once in float32.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  A case of exactly three views is recorded view by view (ref_harness.run_views).

One fixture per transform case and direction, fr1_<case>_<direction>.npz:
    in/pos, in/normal (those the case has), in/camera/{eye, at, up}, grad_in/{pos, normal}
    ref64/{pos, normal}, ref64/grad/{pos, normal}, ref64/grad/camera/{eye, at, up}: d sum(out * grad_in) / d input
    ref32/{pos, normal}: the float32 run's values
    ref64/one/{pos, normal}, ref32/one/...: for a one-view case, the unbatched function's values on that view
and one per projection case, fr1_<case>.npz:
    in/surfels, in/camera/{eye, at, up, viewport, fovy, focal_length}, grad_in/{plane, px_coord}
    ref64/{plane, px_coord, px_idx}, ref32/{plane, px_coord, px_idx}; px_idx as int64 (the reference returns floats)
    ref64/grad_plane/{surfels, camera/...}: d sum(project_surfels * grad_in/plane) / d input, and
    ref64/grad_px_coord/{...} likewise for project_image_coordinates' px_coord.
The subfolder keeps the fixtures out of the top-level globs (the golden drift check, conftest.golden_cases)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import frames_cases as cases  # noqa: E402

with R.quiet():
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402

VIEW_KEYS = ("eye", "at", "up")
BATCHED = {"to_cam": R.ref_utils.world_to_cam_batched, "to_world": R.ref_utils.cam_to_world_batched}
UNBATCHED = {"to_cam": R.ref_utils.world_to_cam, "to_world": R.ref_utils.cam_to_world}


def leaf(a, dtype):
    return torch.tensor(np.asarray(a, dtype=np.float32), dtype=dtype, requires_grad=True)


def camera_leaves(camera, dtype):
    leaves = {k: leaf(camera[k], dtype) for k in VIEW_KEYS}
    return dict(camera, **leaves), leaves


def grad_of(t):
    return t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape), np.float64)


def backward(res, upstream, dtype):
    sum(torch.sum(res[k] * torch.tensor(g, dtype=dtype)) for k, g in upstream.items()).backward()


def pack_inputs(flat, c, keys):
    for k in keys:
        if c[k] is not None:
            flat["in/" + k] = c[k]
    for k, v in c["camera"].items():
        flat["in/camera/" + k] = np.asarray(v, dtype=np.float64 if k in ("fovy", "focal_length") else None)


def record_transform(c, direction, dtype, prefix, flat):
    B = c["camera"]["eye"].shape[0]
    leaves = {k: leaf(c[k], dtype) for k in ("pos", "normal") if c[k] is not None}
    camera, cam_leaves = camera_leaves(c["camera"], dtype)

    def run(views):
        with R.quiet():
            res = BATCHED[direction](*(leaves[k][views] if k in leaves else None for k in ("pos", "normal")),
                                     R.camera_views(camera, views))
        return {k: v for k, v in res.items() if v is not None}

    with R.precision(dtype):
        res = R.run_views(run, B)
        assert set(res) == set(c["upstream"]) and all(v.dtype == dtype for v in res.values())
        for k, v in res.items():
            flat[f"{prefix}/{k}"] = v.detach().numpy()
        if dtype == torch.float64:
            backward(res, c["upstream"], dtype)
            for k, t in leaves.items():
                flat[f"{prefix}/grad/{k}"] = grad_of(t)
            for k, t in cam_leaves.items():
                flat[f"{prefix}/grad/camera/{k}"] = grad_of(t)
        if B == 1:
            with R.quiet(), torch.no_grad():
                one = UNBATCHED[direction](*(leaves[k][0] if k in leaves else None for k in ("pos", "normal")),
                                           {k: camera[k][0] for k in VIEW_KEYS})
            for k, v in one.items():
                if v is not None:
                    flat[f"{prefix}/one/{k}"] = v.numpy()


def emit_transform(name, direction):
    c = cases.transform_case(name)
    flat = {}
    pack_inputs(flat, c, ("pos", "normal"))
    for k, g in c["upstream"].items():
        flat["grad_in/" + k] = g
    for prefix, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
        record_transform(c, direction, dtype, prefix, flat)
    R.write(f"fr1_{name}_{direction}", flat)


def record_project(c, dtype, prefix, flat):
    B = c["surfels"].shape[0]
    for out in ("plane", "px_coord"):
        surfels = leaf(c["surfels"], dtype)
        camera, cam_leaves = camera_leaves(c["camera"], dtype)

        def run(views):
            cam = R.camera_views(camera, views)
            with R.quiet():
                if out == "plane":
                    return {"plane": ref_projection.project_surfels(surfels[views], cam)}
                idx, px = ref_projection.project_image_coordinates(surfels[views], cam)
            return {"px_coord": px, "px_idx": idx}

        with R.precision(dtype):
            res = R.run_views(run, B)
            assert res[out].dtype == dtype
            for k, v in res.items():
                v = v.detach().numpy()
                if k == "px_idx":
                    assert np.array_equal(v, np.round(v))
                    v = v.astype(np.int64)
                flat[f"{prefix}/{k}"] = v
            if dtype == torch.float64:
                backward(res, {out: c["upstream"][out]}, dtype)
                flat[f"{prefix}/grad_{out}/surfels"] = grad_of(surfels)
                for k, t in cam_leaves.items():
                    flat[f"{prefix}/grad_{out}/camera/{k}"] = grad_of(t)


def emit_project(name):
    c = cases.project_case(name)
    flat = {}
    pack_inputs(flat, c, ("surfels",))
    for k, g in c["upstream"].items():
        flat["grad_in/" + k] = g
    for prefix, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
        record_project(c, dtype, prefix, flat)
    R.write("fr1_" + name, flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("frames")
    for n in cases.GOLDEN_TRANSFORM:
        for d in cases.DIRECTIONS:
            emit_transform(n, d)
    for n in cases.GOLDEN_PROJECT:
        emit_project(n)
