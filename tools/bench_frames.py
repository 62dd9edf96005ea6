#!/usr/bin/env python3
"""cam_to_world_batched and project_image_coordinates against the float32 torch compositions they replace, forward +
backward, on the GPU, with the camera detached and with its eye, at and up as leaves (camera_grad=True).

Workload: B = 64 views of N = 128 x 128 points each.
    cam_to_world      pos [B, N, 3] and normal [B, N, 3] that require grad; loss: a random weighting of both outputs
    px_coordinates    surfels [B, N, 3] that require grad, spread over a 128 x 128 frame; loss: a random weighting of
                      px_coord (px_idx carries no gradient)
Each with two forms in one process, alternating round by round after a warm-up so that both see the same machine state:
    fused        one call of the layer and its backward (HIP kernels; with camera leaves also the host's fp64 chain
                 through lookat)
    composition  tests/frames_oracle.py's restatement of the same function in float32 on the same GPU, the camera
                 leaves float32 tensors on the GPU
Each round times a window of at least --window seconds per form with device events; the rounds are run --runs times
(twice by default) and every run is reported.  One JSON line per workload, camera mode and run: the median ms per batch of
each form, the run-to-run spread (min .. max over the rounds) of both, their ratio, and how far each form is from the
same composition evaluated once in float64 on the same inputs (max|form - fp64| / max|fp64| per array).
Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import frames_oracle as fo  # noqa: E402
from surf_renderer_amd import cam_to_world_batched, project_image_coordinates  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_frames: no GPU")
dev = torch.device("cuda:0")
B, S = args.views, args.size
N = S * S
VIEW_KEYS = ("eye", "at", "up")

rng, camera, host = pb.surfel_workload(B, S, 1)
points = {"pos": rng.uniform(-2.0, 2.0, (B, N, 3)), "normal": rng.uniform(-1.0, 1.0, (B, N, 3))}
ups = {"pos": torch.tensor(rng.uniform(-1, 1, (B, N, 4)).astype(np.float32), device=dev),
       "normal": torch.tensor(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32), device=dev),
       "px_coord": torch.tensor(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32), device=dev)}


def camera_of(x):
    """the workload's camera, with the entries that are leaves of this figure taken from `x`"""
    return dict(camera, **{k: x[k] for k in VIEW_KEYS if k in x})


def _fused_coords(x):
    return {"px_coord": project_image_coordinates(x["surfels"], camera_of(x), camera_grad="eye" in x)[1]}


WORKLOADS = {  # workload -> (its point leaves, its outputs, fused, composition)
    "cam_to_world": (points, ("pos", "normal"),
                     lambda x: cam_to_world_batched(x["pos"], x["normal"], camera_of(x), camera_grad="eye" in x),
                     lambda x: fo.cam_to_world_batched(x["pos"], x["normal"], camera_of(x))),
    "px_coordinates": ({"surfels": host["surfels"]}, ("px_coord",), _fused_coords,
                       lambda x: {"px_coord": fo.project_image_coordinates(x["surfels"], camera_of(x))[1]}),
}

for workload, (inputs, outputs, fused_fn, composition_fn) in WORKLOADS.items():
    for camera_leaves in (False, True):
        leaves = pb.leaves(dict(inputs, **({k: camera[k] for k in VIEW_KEYS} if camera_leaves else {})), dev)
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
            agree[name] = pb.agreement(values[name], leaves, want_v, want_g, outputs, share=False)
        del want_v, want_g
        for r in range(args.runs):
            calls, times, med = pb.timed(forms, args.rounds, args.window)
            out = {"workload": workload + "_fwd_bwd", "camera": "leaves" if camera_leaves else "detached", "run": r + 1,
                   "views": B, "points_per_view": N, "rounds": args.rounds, "window_s_at_least": args.window,
                   "calls_per_window": calls}
            out.update({name: pb.spread(ts) for name, ts in times.items()})
            out.update(pb.against_composition(times, med))
            if r == 0:
                out["against_float64_composition"] = agree
            print(json.dumps(out), flush=True)
