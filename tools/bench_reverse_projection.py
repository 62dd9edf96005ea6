#!/usr/bin/env python3
"""projection_reverse_renderer against the torch composition it replaces, forward + backward, on the GPU.

Workload: B = 64 views at 128 x 128 with D = 3, a rotated image and compute_new_depth, rgb / in_pos_wc / out_pos_wc /
rotated_image all requiring grad, the loss a random weighting of out, image1 and depth (the mask carries no gradient).
The positions are what 64 camera pairs see of the two-layer surface of tests/reverse_projection_cases.py, pixel centre
by pixel centre.  Two forms, in one process, alternating round by round after a warm-up so that both see the same
machine state:
    fused        one projection_reverse_renderer call and its backward (HIP kernels and one torch.sort)
    composition  the reference's formulation -- two batched projections and four grid_sample calls -- as tests/
                 reverse_projection_oracle.py restates it, in float32 on the same GPU, one backward
Each round times a window of at least --window seconds per form with device events.  One JSON line: the median ms per
batch of each form, the run-to-run spread (min .. max over the rounds) of both, their ratio, how far each form is from
the same composition evaluated once in float64 on the same inputs (max|form - fp64| / max|fp64| per array, and the share
of elements off by more than 1e-4 of the maximum; float32 decides a few masks and bilinear cells the other way), and
whether two fused calls agree bit for bit (the composition's grid_sample backward adds with float atomics).
Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import reverse_projection_cases as cases  # noqa: E402
import reverse_projection_oracle as ro  # noqa: E402
from surf_renderer_amd import projection_reverse_renderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_reverse_projection: no GPU")
dev = torch.device("cuda:0")
B, S, D = args.views, args.size, 3
FLAGS = {"compute_new_depth": True, "depth_epsilon": 0.1}
TIMED = ("out", "image1", "depth")
rng = np.random.RandomState(0)
cams = [cases.draw_camera(rng, B, side) for side in (-0.9, 0.9)]
camera = [{"eye": c[0], "at": c[1], "up": c[2], "viewport": [0, 0, S, S], "fovy": float(cases.CAMERAS[k][0]),
           "focal_length": cases.CAMERAS[k][1]} for k, c in enumerate(cams)]
x = pb.leaves({"rgb": rng.uniform(0, 1, (B, S, S, D)), "in_pos_wc": cases.seen(*cams[0], S, S, *cases.CAMERAS[0]),
               "out_pos_wc": cases.seen(*cams[1], S, S, *cases.CAMERAS[1]),
               "rotated_image": rng.uniform(0, 1, (B, S, S, D))}, dev)
ups = pb.upstreams(rng, TIMED, B, S, D, dev)
values = {}


def fused():
    pb.clear(x)
    out, proj_out = projection_reverse_renderer(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], *camera,
                                                rotated_image=x["rotated_image"], **FLAGS)
    values["fused"] = dict(proj_out, out=out)
    pb.loss(values["fused"], ups).backward()


def project(x):
    return ro.project(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], *camera, x["rotated_image"], **FLAGS)


def composition():
    pb.clear(x)
    values["composition"] = project(x)
    pb.loss(values["composition"], ups).backward()


def snapshot(name):
    torch.cuda.synchronize()
    return [values[name][k].detach().clone() for k in ro.OUTPUTS] + [t.grad.clone() for t in x.values()]


forms = {"fused": fused, "composition": composition}
want_v, want_g = pb.composition_fp64(project, x, ups)
agree, repeatable = {}, {}
for name, fn in forms.items():                                # warm-up, each form against float64 and against itself
    fn()
    first = snapshot(name)
    fn()
    repeatable[name] = all(bool(torch.equal(a, b)) for a, b in zip(first, snapshot(name)))
    agree[name] = pb.agreement(values[name], x, want_v, want_g, ro.OUTPUTS)
del want_v, want_g, first
calls, times, med = pb.timed(forms, args.rounds, args.window)
out = {"workload": "reverse_projection_fwd_bwd", "views": B, "size": S, "channels": D, "rounds": args.rounds,
       "window_s_at_least": args.window, "calls_per_window": calls,
       "mask_mean": round(float(values["fused"]["mask"].detach().mean()), 4)}
out.update({name: dict(pb.spread(ts), two_calls_bit_identical=repeatable[name]) for name, ts in times.items()})
out.update(pb.against_composition(times, med))
out["against_float64_composition"] = agree
print(json.dumps(out))
