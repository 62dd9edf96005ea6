#!/usr/bin/env python3
"""Generate tests/golden/regularizers/r1_*.npz: the seven geometric regularisers of the reference's trainers
(diffrend/torch/GAN/gan.py:619-633) from the reference's OWN functions (diffrend/torch/utils.py: unit_norm2_L2loss,
away_from_camera_penalty, spatial_3x3, depth_rgb_gradient_consistency, normal_consistency_cost; the z-range penalty and
the position-variance term as the trainers write them inline), running UNMODIFIED on the CPU in float64 under autograd.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  The inputs are the seeded cases of tests/regularizer_cases.py.  Stored per fixture, with the view axis:
in/{pos, normal, image, depth} (float32), in/{z_min, z_max, z_scale, unit_normal_scale}, in/flat (the deliberately
degenerate pixels, where a case has some), weights (B, 7) in REGULARIZER_TERMS order, every weight non-zero,
ref/<term> (B,) and grad/<input> = d (sum_views sum_k weights[k] term_k) / d input, float64.  The subfolder keeps the
fixtures out of the top-level globs (the golden drift check, conftest.golden_cases)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import regularizer_cases as cases  # noqa: E402
from regularizer_oracle import INPUTS, TERMS  # noqa: E402

FIXTURES = ("2x2", "3x5", "17x9_b3", "36x48", "flat_patch", "near_flat")


def reference_terms(pos, normal, image, depth, z_min, z_max, z_scale, unit_normal_scale):
    """One view through the reference's functions, called as the trainers call them."""
    U = R.ref_utils
    relu = torch.nn.functional.relu
    z_pos = pos[..., 2]
    var = torch.mean(pos[..., 0].var() + pos[..., 1].var() + pos[..., 2].var())
    return {"z": torch.mean((z_scale * relu(z_min - torch.abs(z_pos))) ** 2 + (z_scale * relu(torch.abs(z_pos) - z_max)) ** 2),
            "unit_normal": U.unit_norm2_L2loss(normal, unit_normal_scale),
            "normal_consistency": U.normal_consistency_cost(pos, normal, norm=1),
            "spatial": U.spatial_3x3(pos),
            "spatial_var": 1 / (var + 1e-4),
            "image_depth_consistency": U.depth_rgb_gradient_consistency(image, depth),
            "away_from_camera": U.away_from_camera_penalty(pos, normal)}


def emit(name):
    c = cases.case(name)
    assert np.all(c["weights"] != 0)
    leaves = {k: torch.tensor(c[k].astype(np.float64), requires_grad=True) for k in INPUTS}
    B = c["depth"].shape[0]
    values = {k: [] for k in TERMS}
    loss = 0.0
    with R.precision(torch.float64), R.quiet():
        for b in range(B):
            t = reference_terms(*(leaves[k][b] for k in INPUTS), c["z_min"], c["z_max"], c["z_scale"], c["unit_normal_scale"])
            for k, name_k in enumerate(TERMS):
                assert t[name_k].dtype == torch.float64
                values[name_k].append(float(t[name_k].detach()))
                loss = loss + float(c["weights"][b, k]) * t[name_k]
        loss.backward()
    out = {"in/" + k: c[k] for k in INPUTS}
    for k in ("z_min", "z_max", "z_scale", "unit_normal_scale"):
        out["in/" + k] = np.asarray(c[k], dtype=np.float64)
    if c["flat"] is not None:
        out["in/flat"] = c["flat"]
    out["weights"] = c["weights"]
    for k in TERMS:
        out["ref/" + k] = np.asarray(values[k], dtype=np.float64)
    for k in INPUTS:
        out["grad/" + k] = leaves[k].grad.numpy()
    R.write("r1_" + name, out)


if __name__ == "__main__":
    R.OUT = os.path.join(R.REPO, "tests", "golden", "regularizers")
    for n in FIXTURES:
        emit(n)
