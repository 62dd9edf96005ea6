#!/usr/bin/env python3
"""Generate tests/golden/dense_projection/dp1_*.npz: the reference's OWN projection_renderer_differentiable
(diffrend/torch/projection_layer.py:108-152), imported UNMODIFIED and run on the CPU under autograd, on the seeded
cases of tests/dense_projection_cases.py (RECORDED: every frame with rgb as [B, H, W, D], the small ones as [B, N, D]
too), WITHOUT a rotated image: with one the reference's own line raises a broadcast error for every frame of more than
one pixel, so that branch has no reference result to record.  dp2_*.npz are the RECORDED edge cases of tests/
dense_projection_edge_cases.py (a frame of one row; surfels 1e3 to 1e12 pixels off the frame), as grids without a rotated
image.  The reference raised on neither.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  The function is tried in float64 first (ref_harness.precision); PRECISION below records which precision
the unedited function ran in, and every fixture carries it as in/precision.  A case of exactly three views is recorded
view by view (ref_harness.run_views).

Stored per fixture: in/{surfels, rgb}, in/camera/{eye, at, up, viewport, fovy, focal_length}, in/blur_size,
in/precision, grad_in/{out, mask} (the case's upstream gradients), ref/{out, mask} and grad/{surfels, rgb} = d
sum_outputs sum(output * grad_in) / d input.  Inputs and upstream gradients are float32 values; results are in the
recorded precision.  The subfolder keeps the fixtures out of the top-level globs (the golden drift check,
conftest.golden_cases)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import dense_projection_cases as cases  # noqa: E402
import dense_projection_edge_cases as edges  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402


def run_reference(c, dtype):
    """({output: tensor}, {input: leaf}) of the reference on case `c` in `dtype`."""
    leaves = {k: torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("surfels", "rgb")}
    camera = R.layer_camera(c["camera"], dtype)

    def run(views):
        with R.quiet(), R.precision(dtype):
            out, mask = ref_projection.projection_renderer_differentiable(
                leaves["surfels"][views], leaves["rgb"][views], R.camera_views(camera, views), rotated_image=None,
                blur_size=c["blur_size"])
        return {"out": out, "mask": mask}

    return R.run_views(run, c["shape"][0]), leaves


def pick_precision():
    """float64 if the unedited function runs in it, forward and backward, and returns float64, else float32."""
    try:
        c = cases.case("3x5")
        res, leaves = run_reference(c, torch.float64)
        if all(v.dtype == torch.float64 for v in res.values()):
            R.pack_layer(c, leaves, res, dtype=torch.float64)
            return torch.float64
    except (RuntimeError, TypeError) as e:
        print(f"float64 run failed: {e}")
    return torch.float32


def emit(c, fixture, dtype):
    res, leaves = run_reference(c, dtype)
    flat = R.pack_layer(c, leaves, res, dtype=dtype)
    flat["in/blur_size"] = np.asarray(c["blur_size"], dtype=np.float64)
    flat["in/precision"] = np.asarray(str(dtype).replace("torch.", ""))
    R.write(fixture, flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("dense_projection")
    PRECISION = pick_precision()
    print(f"recording in {PRECISION}")
    for f, layout in cases.RECORDED:
        emit(cases.case(f, layout), "dp1_" + cases.tag(f, layout), PRECISION)
    for n, layout in edges.RECORDED:           # a list of their own: the seeded fixtures above stay as they are
        emit(edges.case(n, layout), "dp2_" + edges.tag(n, layout), PRECISION)
