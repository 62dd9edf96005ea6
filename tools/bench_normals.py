#!/usr/bin/env python3
"""estimate_surface_normals_plane_fit_batched, alone and after depth_to_surfels, against the torch compositions they
replace, forward + backward, on the GPU.

Workload: B = 64 views at 128 x 128.  Two figures, each with two forms in one process, alternating round by round after
a warm-up so that both see the same machine state:
    normals        fused        one estimate_surface_normals_plane_fit_batched call on a grid of points [B, H, W, 3]
                                that requires grad, and its backward (three HIP kernels)
                   composition  tests/normals_oracle.py's plane_fit -- the reference's batched function restated: a
                                reflected pad, eight differences stacked as [8, B, H, W, 3], about 25 elementwise and
                                reduction launches -- in float32 on the same GPU, one backward
                   loss         a random weighting of the normals
    depth_normals  fused        depth_to_surfels(frame='camera'), then the plane fit, one backward (five HIP kernels)
                   composition  tests/surfels_oracle.py's lift, then plane_fit, in float32, one backward
                   loss         a random weighting of the normals and of the points, from a depth map that requires grad
The points are those of tests/normals_cases.py: lifted from depth = 3 + a smooth term + noise of at most 0.05.
Each round times a window of at least --window seconds per form with device events.  One JSON line per figure: the
median ms per batch of each form, the run-to-run spread (min .. max over the rounds) of both, their ratio, whether the
slowest fused round beats the fastest round of the composition (fused_faster_beyond_spread), and how far
each form is from the same composition evaluated once in float64 on the same inputs (max|form - fp64| / max|fp64| per
array, and the share of elements off by more than 1e-4 of the maximum).
Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import normals_cases as nc  # noqa: E402
import normals_oracle as no  # noqa: E402
import surfels_oracle as so  # noqa: E402
from projection_cases import FOCAL, FOVY, draw_camera  # noqa: E402
from surf_renderer_amd import depth_to_surfels, estimate_surface_normals_plane_fit_batched  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_normals: no GPU")
dev = torch.device("cuda:0")
B, S = args.views, args.size
rng = np.random.RandomState(0)
eye, at, up = draw_camera(rng, B)
camera = {"eye": eye, "at": at, "up": up, "viewport": [0, 0, S, S], "fovy": float(FOVY), "focal_length": FOCAL}
depth = nc.draw_depth(rng, B, S, S)
x = pb.leaves({"depth": depth, "pos": nc.lifted(depth, camera)}, dev)
ups = {"normal": torch.tensor(rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32), device=dev),
       "pos": torch.tensor(rng.uniform(-1, 1, (B, S * S, 3)).astype(np.float32), device=dev)}


def _chain(pos, fit):
    return {"pos": pos, "normal": fit(pos).reshape(B, S, S, 3)}


FIGURES = {  # figure -> (the leaves it differentiates, its outputs, fused, composition)
    "normals": (("pos",), ("normal",),
                lambda x: {"normal": estimate_surface_normals_plane_fit_batched(x["pos"])},
                lambda x: {"normal": no.plane_fit(x["pos"])}),
    "depth_normals": (("depth",), ("pos", "normal"),
                      lambda x: _chain(depth_to_surfels(x["depth"], camera, frame="camera"),
                                       lambda p: estimate_surface_normals_plane_fit_batched(p, camera)),
                      lambda x: _chain(so.lift(x["depth"], camera, frame="camera"), lambda p: no.plane_fit(p, camera))),
}

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
    out = {"workload": figure + "_fwd_bwd", "views": B, "size": S, "rounds": args.rounds,
           "window_s_at_least": args.window, "calls_per_window": calls}
    out.update({name: pb.spread(ts) for name, ts in times.items()})
    out.update(pb.against_composition(times, med))
    out["against_float64_composition"] = agree
    print(json.dumps(out), flush=True)
