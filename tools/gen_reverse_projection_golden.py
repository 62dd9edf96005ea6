#!/usr/bin/env python3
"""Generate tests/golden/reverse_projection/rp1_*.npz: the reference's OWN projection_reverse_renderer (diffrend/torch/
projection_layer.py:281-333), imported UNMODIFIED and run on the CPU in float32 under autograd, on the seeded cases of
tests/reverse_projection_cases.py and the variants of its 12x16 case that change the function.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  A case of exactly three views is recorded view by view (see emit).  The reference's mask does not
require grad, so a fixture's gradients are those of the other outputs.

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
from reverse_projection_oracle import INPUTS  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402


def emit(name, variant):
    c = cases.case(name, variant)
    B, H, W, D = c["shape"]
    leaves = {k: torch.tensor(c[k], requires_grad=True) for k in INPUTS if c[k] is not None}
    cameras = [{k: (torch.tensor(np.asarray(v, dtype=np.float32)) if k in ("eye", "at", "up") else v)
                for k, v in c[cam].items()} for cam in ("camera1", "camera2")]

    def run(views):
        cam1, cam2 = ({k: (v[views] if k in ("eye", "at", "up") else v) for k, v in cam.items()} for cam in cameras)
        with R.quiet():
            out, proj_out = ref_projection.projection_reverse_renderer(
                leaves["rgb"][views], leaves["in_pos_wc"][views], leaves["out_pos_wc"][views], cam1, cam2,
                rotated_image=leaves["rotated_image"][views] if "rotated_image" in leaves else None, **c["flags"])
        return dict(proj_out, out=out)

    if B == 3:
        # lookat_rot_inv calls torch.cross(up, z) without `dim`, which for [3, 3] operands -- three views, and only
        # three -- still means dim 0: the cross product is taken ACROSS the views.  That is an accident of B == 3,
        # not a meaning of the layer, so such a case is recorded view by view
        per_view = [run(slice(b, b + 1)) for b in range(B)]
        res = {k: torch.cat([r[k] for r in per_view]) for k in per_view[0]}
    else:
        res = run(slice(None))
    assert set(res) == set(c["upstream"]), (sorted(res), sorted(c["upstream"]))
    sum(torch.sum(res[k] * torch.tensor(g)) for k, g in c["upstream"].items()).backward()
    flat = {"in/" + k: c[k] for k in leaves}
    for cam in ("camera1", "camera2"):
        for k, v in c[cam].items():
            flat[f"in/{cam}/{k}"] = np.asarray(v, dtype=np.float64 if k in ("fovy", "focal_length") else None)
    flat["in/flags"] = np.asarray(json.dumps(c["flags"], sort_keys=True))
    for k, g in c["upstream"].items():
        assert res[k].dtype == torch.float32 and tuple(res[k].shape) == g.shape, k
        flat["grad_in/" + k] = g
        flat["ref/" + k] = res[k].detach().numpy()
    for k, t in leaves.items():
        flat["grad/" + k] = t.grad.numpy() if t.grad is not None else np.zeros(t.shape, np.float32)
    R.write("rp1_" + cases.tag(name, variant), flat)


if __name__ == "__main__":
    R.OUT = os.path.join(R.REPO, "tests", "golden", "reverse_projection")
    for n, v in cases.FIXTURES:
        emit(n, v)
