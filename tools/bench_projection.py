#!/usr/bin/env python3
"""projection_renderer_differentiable_fast against the torch composition it replaces, forward + backward, on the GPU.

Workload: B = 64 views at 128 x 128 with D = 3, a rotated image and compute_new_depth, surfels / rgb / rotated_image all
requiring grad, the loss a random weighting of out, mask, image1 and depth.  The surfels are a jittered depth map seen
from the target cameras (tools/projection_bench.surfel_workload), about one per cell.  Two forms, in one process, alternating
round by round after a warm-up so that both see the same machine state:
    fused        one projection_renderer_differentiable_fast call and its backward (HIP kernels and one torch.sort)
    composition  the reference's formulation -- 24 scatter-adds, dense convolutions -- as tests/projection_oracle.py
                 restates it, in float32 on the same GPU, one backward
Each round times a window of at least --window seconds per form with device events.  One JSON line: the median ms per
batch of each form, the run-to-run spread (min .. max over the rounds) of both, their ratio, and how far each form is
from the same composition evaluated once in float64 on the same inputs (max|form - fp64| / max|fp64| per array, and the
share of elements off by more than 1e-4 of the maximum).  The float32 composition picks another cell than float64 for
the few surfels whose pixel coordinate is within float32 rounding of an integer, so its maximum error is large where
the kernels', which compute in fp64, is not.
Fails without a GPU."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import projection_oracle as po  # noqa: E402
from surf_renderer_amd import projection_renderer_differentiable_fast  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_projection: no GPU")
dev = torch.device("cuda:0")
B, S, D = args.views, args.size, 3
FLAGS = {"compute_new_depth": True}
rng, camera, host = pb.surfel_workload(B, S, D)
x = pb.leaves(host, dev)
ups = pb.upstreams(rng, po.OUTPUTS, B, S, D, dev)
values = {}


def fused():
    pb.clear(x)
    out, proj_out = projection_renderer_differentiable_fast(x["surfels"], x["rgb"], camera, x["rotated_image"], **FLAGS)
    values["fused"] = dict(proj_out, out=out)
    pb.loss(values["fused"], ups).backward()


def project(x):
    return po.project(x["surfels"], x["rgb"], camera, x["rotated_image"], **FLAGS)


def composition():
    pb.clear(x)
    values["composition"] = project(x)
    pb.loss(values["composition"], ups).backward()


forms = {"fused": fused, "composition": composition}
want_v, want_g = pb.composition_fp64(project, x, ups)
agree = {}
for name, fn in forms.items():                                # warm-up, and each form against float64
    fn(); fn()
    torch.cuda.synchronize()
    agree[name] = pb.agreement(values[name], x, want_v, want_g, po.OUTPUTS)
del want_v, want_g
calls, times, med = pb.timed(forms, args.rounds, args.window)
out = {"workload": "projection_fwd_bwd", "views": B, "size": S, "channels": D, "rounds": args.rounds,
       "window_s_at_least": args.window, "calls_per_window": calls}
out.update({name: pb.spread(ts) for name, ts in times.items()})
out.update(pb.against_composition(times, med))
out["against_float64_composition"] = agree
print(json.dumps(out))
