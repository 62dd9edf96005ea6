#!/usr/bin/env python3
"""Generate tests/golden/projection/pr1_*.npz: the reference's OWN projection_renderer_differentiable_fast
(diffrend/torch/projection_layer.py:170-278), imported UNMODIFIED and run on the CPU under autograd, on the seeded
cases of tests/projection_cases.py and the flag variants of its 12x16 case; and pr2_*.npz, the same on the RECORDED edge
cases of tests/projection_edge_cases.py (half-width 0, frames of one row and one column, exact coordinates with Z = 0,
a view of nothing but dropped surfels): the arms on which the restatement is otherwise pinned to nothing.  The reference
raised on none of them.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  The reference runs this function in float32 only (its blur builds float32 taps, so the float64 shim of
ref_harness.precision ends in a dtype error), so the fixtures hold float32 results; tests/
test_projection_oracle_cpu.py states what that leaves of the comparison.  It also needs rgb as [B, H, W, D], so a
[B, N, D] case is handed over reshaped.  A case of exactly three views is recorded view by view (ref_harness.run_views).

Stored per fixture: in/{surfels, rgb, rotated_image}, in/camera/{eye, at, up, viewport, fovy, focal_length},
in/blur_size, in/flags (JSON), grad_in/<output> (the case's upstream gradients), ref/<output> [B, H, W, .] and
grad/<input> = d sum_outputs sum(output * grad_in) / d input, float32.  The subfolder keeps the fixtures out of the
top-level globs (the golden drift check, conftest.golden_cases)."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import projection_cases as cases  # noqa: E402
import projection_edge_cases as edges  # noqa: E402
from projection_oracle import INPUTS  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402


def emit(c, fixture):
    B, H, W, D = c["shape"]
    leaves = {k: torch.tensor(c[k], requires_grad=True) for k in INPUTS if c[k] is not None}
    camera = R.layer_camera(c["camera"])

    def run(views):
        with R.quiet():
            out, proj_out = ref_projection.projection_renderer_differentiable_fast(
                leaves["surfels"][views], leaves["rgb"][views].reshape(-1, H, W, D), R.camera_views(camera, views),
                rotated_image=leaves["rotated_image"][views].reshape(-1, H, W, D) if "rotated_image" in leaves else None,
                blur_size=c["blur_size"], **c["flags"])
        return dict(proj_out, out=out)

    flat = R.pack_layer(c, leaves, R.run_views(run, B))
    flat["in/blur_size"] = np.asarray(c["blur_size"], dtype=np.float64)
    flat["in/flags"] = np.asarray(json.dumps(c["flags"], sort_keys=True))
    R.write(fixture, flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("projection")
    for n, v in cases.ALL:
        emit(cases.case(n, v), "pr1_" + cases.tag(n, v))
    for n in edges.RECORDED:                   # a list of their own: the seeded fixtures above stay as they are
        assert edges.margin(edges.case(n)) >= 1.0, n
        emit(edges.case(n), "pr2_" + n)
