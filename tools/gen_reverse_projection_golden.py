#!/usr/bin/env python3
"""Generate tests/golden/reverse_projection/rp1_*.npz: the reference's OWN projection_reverse_renderer (diffrend/torch/
projection_layer.py:281-333), imported UNMODIFIED and run on the CPU in float32 under autograd, on the seeded cases of
tests/reverse_projection_cases.py and the variants of its 12x16 case that change the function; and rp2_*.npz, the same on
the RECORDED edge cases of tests/reverse_projection_edge_cases.py (frames of one row and of one column).  The reference
raised on neither.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  A case of exactly three views is recorded view by view (ref_harness.run_views).  The reference's mask
does not require grad, so a fixture's gradients are those of the other outputs.

Stored per fixture: in/{rgb, in_pos_wc, out_pos_wc, rotated_image}, in/camera{1,2}/{eye, at, up, viewport, fovy,
focal_length}, in/flags (JSON), grad_in/<output> (the case's upstream gradients), ref/<output> [B, H, W, .] and
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
import reverse_projection_cases as cases  # noqa: E402
import reverse_projection_edge_cases as edges  # noqa: E402
from reverse_projection_oracle import INPUTS  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402


def emit(c, fixture):
    leaves = {k: torch.tensor(c[k], requires_grad=True) for k in INPUTS if c[k] is not None}
    cameras = [R.layer_camera(c[cam]) for cam in ("camera1", "camera2")]

    def run(views):
        with R.quiet():
            out, proj_out = ref_projection.projection_reverse_renderer(
                leaves["rgb"][views], leaves["in_pos_wc"][views], leaves["out_pos_wc"][views],
                *(R.camera_views(cam, views) for cam in cameras),
                rotated_image=leaves["rotated_image"][views] if "rotated_image" in leaves else None, **c["flags"])
        return dict(proj_out, out=out)

    flat = R.pack_layer(c, leaves, R.run_views(run, c["shape"][0]), cameras=("camera1", "camera2"))
    flat["in/flags"] = np.asarray(json.dumps(c["flags"], sort_keys=True))
    R.write(fixture, flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("reverse_projection")
    for n, v in cases.FIXTURES:
        emit(cases.case(n, v), "rp1_" + cases.tag(n, v))
    for n in edges.RECORDED:                   # a list of their own: the seeded fixtures above stay as they are
        assert edges.margin(edges.case(n)) >= 1.0, n
        emit(edges.case(n), "rp2_" + n)
