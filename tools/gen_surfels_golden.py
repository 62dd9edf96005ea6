#!/usr/bin/env python3
"""Generate tests/golden/surfels/sf1_*.npz: the reference's OWN depth lift, cam_to_world_batched(z_to_pcl_CC_batched(
-depth, camera), None, camera)['pos'] (diffrend/torch/renderer.py:510-534, torch/utils.py:622-647), imported UNMODIFIED
and run on the CPU under autograd, on the seeded cases of tests/surfels_cases.py -- once in float64 (ref_harness.
precision) and once in float32.  The `camera` variant records z_to_pcl_CC_batched alone.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  A case of exactly three views is recorded view by view (ref_harness.run_views).  The reference returns
homogeneous points; the generator asserts that the fourth column is exactly 1 and stores the first three.

Stored per fixture: in/depth (in the case's own shape), in/camera/{eye, at, up, viewport, fovy, focal_length}, in/frame,
grad_in/pos (the case's upstream gradient), and for P in (ref64, ref32): P/pos [B, N, 3] and P/grad/depth =
d sum(pos * grad_in) / d depth, in that precision.  The subfolder keeps the fixtures out of the top-level globs (the
golden drift check, conftest.golden_cases)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import surfels_cases as cases  # noqa: E402


def record(c, dtype):
    B, H, W = c["shape"]
    leaves = {"depth": torch.tensor(c["depth"], dtype=dtype, requires_grad=True)}
    camera = R.layer_camera(c["camera"], dtype)

    def run(views):
        cam = R.camera_views(camera, views)
        with R.quiet():
            pos = R.ref_tch.z_to_pcl_CC_batched(-leaves["depth"][views].reshape(-1, H * W), cam)
            if c["frame"] == "world":
                pos = R.ref_utils.cam_to_world_batched(pos, None, cam)["pos"]
                assert pos.shape[-1] == 4 and bool((pos[..., 3] == 1).all())
        return {"pos": pos[..., :3]}

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
    flat["in/frame"] = np.asarray(c["frame"])
    R.write("sf1_" + cases.tag(name, variant), flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("surfels")
    for n, v in cases.ALL:
        emit(n, v)
