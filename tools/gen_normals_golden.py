#!/usr/bin/env python3
"""Generate tests/golden/normals/nm1_*.npz: the reference's OWN estimate_surface_normals_plane_fit_batched
(diffrend/torch/utils.py:926-963), imported UNMODIFIED and run on the CPU under autograd, on the seeded cases of
tests/normals_cases.py -- once in float64 (ref_harness.precision) and once in float32.  A world-frame case adds the
reference's cam_to_world_batched(None, normal, camera)['normal']; the case normals_cases.UNBATCHED is also recorded
through the unbatched estimate_surface_normals_plane_fit, which must equal the batched record bit for bit in float64.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  A case of exactly three views is recorded view by view (ref_harness.run_views).

Stored per fixture: in/pos (in the case's own shape), in/camera/{eye, at, up, viewport, fovy, focal_length}, in/frame,
grad_in/normal (the case's upstream gradient), and for P in (ref64, ref32): P/normal and P/grad/pos =
d sum(normal * grad_in) / d pos, in that precision; for the unbatched case also P/unbatched/normal and
P/unbatched/grad/pos.  The subfolder keeps the fixtures out of the top-level globs (the golden drift check,
conftest.golden_cases)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import normals_cases as cases  # noqa: E402


def record(c, dtype, unbatched=False):
    B, H, W = c["shape"]
    leaves = {"pos": torch.tensor(c["pos"], dtype=dtype, requires_grad=True)}
    camera = R.layer_camera(c["camera"], dtype)

    def run(views):
        grid = leaves["pos"][views].reshape(-1, H, W, 3)
        with R.quiet():
            if unbatched:
                assert grid.shape[0] == 1
                n = R.ref_utils.estimate_surface_normals_plane_fit(grid[0], None)[None]
            else:
                n = R.ref_utils.estimate_surface_normals_plane_fit_batched(grid)
            if c["frame"] == "world":
                n = R.ref_utils.cam_to_world_batched(None, n.reshape(-1, H * W, 3), R.camera_views(camera, views))["normal"]
        return {"normal": n.reshape(leaves["pos"][views].shape)}

    with R.precision(dtype):
        return R.pack_layer(c, leaves, R.run_views(run, B), dtype=dtype)


def emit(name, variant):
    c = cases.case(name, variant)
    flat = {}
    for prefix, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
        for k, v in record(c, dtype).items():
            if k.startswith(("ref/", "grad/")):
                flat[prefix + "/" + (k[len("ref/"):] if k.startswith("ref/") else k)] = v
            else:
                flat[k] = v
        if name == cases.UNBATCHED and variant is None:
            one = record(c, dtype, unbatched=True)
            flat[prefix + "/unbatched/normal"], flat[prefix + "/unbatched/grad/pos"] = one["ref/normal"], one["grad/pos"]
            if dtype == torch.float64:
                assert np.array_equal(one["ref/normal"], flat["ref64/normal"])
                assert np.array_equal(one["grad/pos"], flat["ref64/grad/pos"])
    flat["in/frame"] = np.asarray(c["frame"])
    R.write("nm1_" + cases.tag(name, variant), flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("normals")
    for n, v in cases.ALL:
        emit(n, v)
