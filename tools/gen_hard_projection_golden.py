#!/usr/bin/env python3
"""Generate tests/golden/hard_projection/hp1_*.npz: the reference's OWN projection_renderer (diffrend/torch/
projection_layer.py:88-106), imported UNMODIFIED and run on the CPU under autograd, on the seeded cases of tests/
hard_projection_cases.py -- once in float64 (ref_harness.precision) and once in float32 -- together with the pixel index
its project_image_coordinates gives every surfel in both precisions.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  A case of exactly three views is recorded view by view (ref_harness.run_views).  The generator asserts
the kink condition of every case, and that the float32 and the float64 indices are equal.  hp2_tie_*.npz are the two tie
cases of tests/hard_projection_edge_cases.py: surfels placed on exact rounding ties, where the record pins torch.round's
ties-to-even to the reference itself.

Stored per fixture: in/{surfels, rgb}, in/camera/{eye, at, up, viewport, fovy, focal_length}, grad_in/out (the case's
upstream gradient), and for P in (ref64, ref32): P/out (like rgb), P/mask (bool, like rgb: True where no surfel landed),
P/index [B, N] int64 (N = dropped) and P/grad/rgb = d sum(out * grad_in) / d rgb, in that precision.  The subfolder keeps
the fixtures out of the top-level globs (the golden drift check, conftest.golden_cases)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import hard_projection_cases as cases  # noqa: E402
import hard_projection_edge_cases as edges  # noqa: E402
import hard_projection_oracle as ho  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402


def record(c, dtype):
    B = c["shape"][0]
    leaves = {"surfels": torch.tensor(c["surfels"], dtype=dtype, requires_grad=True),
              "rgb": torch.tensor(c["rgb"], dtype=dtype, requires_grad=True)}
    camera = R.layer_camera(c["camera"], dtype)
    extra = {}

    def run(views):
        cam = R.camera_views(camera, views)
        with R.quiet():
            out, mask = ref_projection.projection_renderer(leaves["surfels"][views], leaves["rgb"][views], cam)
            index, _ = ref_projection.project_image_coordinates(leaves["surfels"][views].detach(), cam)
        extra.setdefault("mask", []).append(mask)
        extra.setdefault("index", []).append(index)
        return {"out": out}

    with R.precision(dtype):
        flat = R.pack_layer(c, leaves, R.run_views(run, B), dtype=dtype)
    assert not np.any(flat.pop("grad/surfels")), "the reference sends no gradient to the surfels"
    flat["ref/mask"] = torch.cat(extra["mask"]).numpy().astype(np.bool_)
    flat["ref/index"] = torch.cat(extra["index"]).numpy().astype(np.int64)
    assert flat["ref/mask"].shape == c["rgb"].shape and flat["ref/index"].shape == c["surfels"].shape[:2]
    return flat


def emit(name, edge=False):
    """hp1_<name> for a seeded case; hp2_<name> for a case of tests/hard_projection_edge_cases.py, whose named surfels
    sit on a rounding tie on purpose and whose other surfels are held to the kink condition."""
    c = edges.case(name) if edge else cases.case(name)
    if edge:
        assert edges.margin(c, c["named"]) >= 1.0, name
    else:
        assert ho.kink_margin(c["surfels"], c["camera"]) >= 1.0, name
    flat = {}
    for prefix, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
        for k, v in record(c, dtype).items():
            if k.startswith(("ref/", "grad/")):
                flat[prefix + "/" + (k[len("ref/"):] if k.startswith("ref/") else k)] = v
            else:
                flat[k] = v
    assert np.array_equal(flat["ref64/index"], flat["ref32/index"]), name
    assert np.array_equal(flat["ref64/mask"], flat["ref32/mask"]), name
    R.write(("hp2_" if edge else "hp1_") + name, flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("hard_projection")
    for n in cases.NAMES:
        emit(n)
    for n in edges.RECORDED:                   # a list of their own: the seeded fixtures above stay as they are
        emit(n, edge=True)
