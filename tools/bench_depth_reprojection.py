#!/usr/bin/env python3
"""depth_to_surfels, alone and followed by projection_renderer, against the torch compositions they replace, forward +
backward, on the GPU.

Workload: B = 64 views at 128 x 128, a depth map in 1.5..3 that requires grad, and for the second figure an image with
D = 3 that requires grad and a second set of cameras 0.3 to the side of the first.  Two figures, each with two forms in
one process, alternating round by round after a warm-up so that both see the same machine state:
    lift             fused        one depth_to_surfels call and its backward (two HIP kernels)
                     composition  tests/surfels_oracle.py's lift on the numpy grid, in float32 on the same GPU
                     loss         a random weighting of the surfels
    lift_projection  fused        depth_to_surfels, then projection_renderer into the second cameras (HIP kernels and one
                                  torch.sort), one backward
                     composition  surfels_oracle.lift, then tests/hard_projection_oracle.py's project (scatter-adds, i.e.
                                  float atomics on the GPU), in float32, one backward
                     loss         a random weighting of the projected image and of the surfels, so that the backward of
                                  both layers runs (the hard projection sends no gradient to the surfels)
Each round times a window of at least --window seconds per form with device events.  One JSON line per figure: the
median ms per batch of each form, the run-to-run spread (min .. max over the rounds) of both, their ratio, and how far
each form is from the same composition evaluated once in float64 on the same inputs (max|form - fp64| / max|fp64| per
array, and the share of elements off by more than 1e-4 of the maximum).  The float32 composition lands the few surfels
whose pixel coordinate is within float32 rounding of a tie on another pixel than float64 does, so its maximum error is
large where the kernels', which compute in fp64, is not.
Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import hard_projection_oracle as ho  # noqa: E402
import surfels_oracle as so  # noqa: E402
from projection_cases import FOCAL, FOVY, draw_camera  # noqa: E402
from surf_renderer_amd import depth_to_surfels, projection_renderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_depth_reprojection: no GPU")
dev = torch.device("cuda:0")
B, S, D = args.views, args.size, 3
rng = np.random.RandomState(0)


def _camera(side):
    eye, at, up = draw_camera(rng, B, side=side)
    return {"eye": eye, "at": at, "up": up, "viewport": [0, 0, S, S], "fovy": float(FOVY), "focal_length": FOCAL}


camera1, camera2 = _camera(0.0), _camera(0.3)
x = pb.leaves({"depth": rng.uniform(1.5, 3.0, (B, S, S)), "rgb": rng.uniform(0, 1, (B, S, S, D))}, dev)
ups = {"pos": torch.tensor(rng.uniform(-1, 1, (B, S * S, 3)).astype(np.float32), device=dev),
       "out": torch.tensor(rng.uniform(-1, 1, (B, S, S, D)).astype(np.float32), device=dev)}
FIGURES = {  # figure -> (the leaves it differentiates, its outputs, fused, composition)
    "lift": (("depth",), ("pos",),
             lambda x: {"pos": depth_to_surfels(x["depth"], camera1)},
             lambda x: {"pos": so.lift(x["depth"], camera1)}),
    "lift_projection": (("depth", "rgb"), ("pos", "out"),
                        lambda x: _chain(x, depth_to_surfels(x["depth"], camera1), projection_renderer),
                        lambda x: _chain(x, so.lift(x["depth"], camera1),
                                         lambda p, rgb, cam: (ho.project(p, rgb, cam)["out"], None))),
}


def _chain(x, pos, project):
    return {"pos": pos, "out": project(pos, x["rgb"], camera2)[0]}


for figure, (wrt, outputs, fused_fn, composition_fn) in FIGURES.items():
    leaves = {k: x[k] for k in wrt}
    weights = {k: ups[k] for k in outputs}
    values = {}

    def run(name, fn):
        pb.clear(leaves)
        values[name] = fn(leaves)
        pb.loss(values[name], weights).backward()

    forms = {"fused": lambda: run("fused", fused_fn), "composition": lambda: run("composition", composition_fn)}
    want_v, want_g = pb.composition_fp64(composition_fn, leaves, weights)
    agree = {}
    for name, fn in forms.items():                                # warm-up, and each form against float64
        fn(); fn()
        torch.cuda.synchronize()
        agree[name] = pb.agreement(values[name], leaves, want_v, want_g, outputs)
    del want_v, want_g
    calls, times, med = pb.timed(forms, args.rounds, args.window)
    out = {"workload": figure + "_fwd_bwd", "views": B, "size": S, "channels": D, "rounds": args.rounds,
           "window_s_at_least": args.window, "calls_per_window": calls}
    out.update({name: pb.spread(ts) for name, ts in times.items()})
    out.update(pb.against_composition(times, med))
    out["against_float64_composition"] = agree
    print(json.dumps(out), flush=True)
