#!/usr/bin/env python3
"""camera_grad=True of the depth lift and the fast projection against the same calls with the cameras detached, and
against the torch composition a caller would otherwise run for a pose gradient, forward + backward, on the GPU.

Workload: B = 64 views at 128 x 128 with D = 3: a depth map in 1.5..3 lifted by the first set of cameras
(depth_to_surfels) and projected into a second set 0.3 to the side (projection_renderer_differentiable_fast), the loss a
random weighting of `out`; depth and rgb require grad in every form.  Three forms, in one process, alternating round by
round after a warm-up so that all see the same machine state:
    camera_grad   both calls with camera_grad=True and all six camera tensors (eye, at, up of both sets) as fp32 GPU
                  leaves: the kView kernels, the finish kernel, and the fp64 autograd chain through lookat on the host
    detached      the same two calls with the cameras as data -- camera_grad minus detached is the price of the feature
    composition   tests/camera_chain_oracle.py's lift and project with the same six leaves, in float32 on the same GPU
Each round times a window of at least --window seconds per form with device events.  One JSON line: the median ms per
batch of each form with its run-to-run spread (min .. max over the rounds), the price of the feature, the ratio to the
composition, and how far the camera gradients of camera_grad and of the composition are from the composition evaluated
once in float64 on the same inputs (max|form - fp64| / max|fp64| per tensor).
Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import camera_chain_oracle as co  # noqa: E402
from projection_cases import FOCAL, FOVY, draw_camera  # noqa: E402
from surf_renderer_amd import depth_to_surfels, projection_renderer_differentiable_fast  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_camera_warp: no GPU")
dev = torch.device("cuda:0")
B, S, D = args.views, args.size, 3
rng = np.random.RandomState(0)


def _camera(side):
    eye, at, up = draw_camera(rng, B, side=side)
    return {"eye": eye, "at": at, "up": up, "viewport": [0, 0, S, S], "fovy": float(FOVY), "focal_length": FOCAL}


data = {"a": _camera(0.0), "b": _camera(0.3)}
x = pb.leaves({"depth": rng.uniform(1.5, 3.0, (B, S, S)), "rgb": rng.uniform(0, 1, (B, S, S, D))}, dev)
cams = {f"{c}_{k}": torch.tensor(data[c][k], device=dev, requires_grad=True) for c in data for k in co.CAMERA_KEYS}
ups = {"out": torch.tensor(rng.uniform(-1, 1, (B, S, S, D)).astype(np.float32), device=dev)}
everything = dict(x, **cams)


def camera(c, tensors):
    return dict(data[c], **{k: tensors[f"{c}_{k}"] for k in co.CAMERA_KEYS}) if tensors else data[c]


def fused(t, tensors, **kw):
    pos = depth_to_surfels(t["depth"], camera("a", tensors), **kw)
    return {"out": projection_renderer_differentiable_fast(pos, t["rgb"], camera("b", tensors), **kw)[0]}


def composition(t):
    return {"out": co.project(co.lift(t["depth"], camera("a", t)), t["rgb"], camera("b", t))["out"]}


values = {}


def run(name, fn):
    pb.clear(everything)
    values[name] = fn()
    pb.loss(values[name], ups).backward()


forms = {"camera_grad": lambda: run("camera_grad", lambda: fused(x, cams, camera_grad=True)),
         "detached": lambda: run("detached", lambda: fused(x, None)),
         "composition": lambda: run("composition", lambda: composition(everything))}
want_v, want_g = pb.composition_fp64(composition, everything, ups)
agree = {}
for name, fn in forms.items():                                # warm-up, and the camera gradients against float64
    fn(); fn()
    torch.cuda.synchronize()
    if name != "detached":
        agree[name] = pb.agreement(values[name], cams, want_v, want_g, (), share=False)
del want_v, want_g
calls, times, med = pb.timed(forms, args.rounds, args.window)
out = {"workload": "lift_projection_camera_grad_fwd_bwd", "views": B, "size": S, "channels": D, "rounds": args.rounds,
       "window_s_at_least": args.window, "calls_per_window": calls}
out.update({name: pb.spread(ts) for name, ts in times.items()})
out["camera_grad_over_detached"] = round(med["camera_grad"] / med["detached"], 3)
out["price_of_the_feature_ms"] = round(med["camera_grad"] - med["detached"], 4)
out["price_beyond_spread"] = bool(min(times["camera_grad"]) > max(times["detached"]))
out["speedup_over_composition_median"] = round(med["composition"] / med["camera_grad"], 2)
out["faster_than_composition_beyond_spread"] = bool(max(times["camera_grad"]) < min(times["composition"]))
out["camera_gradients_against_float64_composition"] = agree
print(json.dumps(out))
