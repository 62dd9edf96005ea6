#!/usr/bin/env python3
"""camera_grad=True of estimate_surface_normals_plane_fit_batched(frame='world') against the same call with the camera
detached and against the float32 torch composition with the same camera leaves, forward + backward, on the GPU.

Workload: tools/bench_normals.py's points (B = 64 views at 128 x 128, lifted from depth = 3 + a smooth term + noise of at
most 0.05), pos requiring grad, the loss a random weighting of the world-frame normals.  Three forms, in one process,
alternating round by round after a warm-up so that all see the same machine state:
    camera_grad   the call with camera_grad=True and eye, at, up as fp32 GPU leaves: k_normals_bwd<true>, the finish
                  kernel, and the fp64 autograd chain through lookat on the host
    detached      the same call with the camera as data -- camera_grad minus detached is the price of the feature
    composition   tests/dense_camera_oracle.py's plane_fit with the same leaves, in float32 on the same GPU
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
import dense_camera_oracle as dco  # noqa: E402
import normals_cases as nc  # noqa: E402
from projection_cases import FOCAL, FOVY, draw_camera  # noqa: E402
from surf_renderer_amd import estimate_surface_normals_plane_fit_batched  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_normals_camera: no GPU")
dev = torch.device("cuda:0")
B, S = args.views, args.size
rng = np.random.RandomState(0)
eye, at, up = draw_camera(rng, B)
data = {"eye": eye, "at": at, "up": up, "viewport": [0, 0, S, S], "fovy": float(FOVY), "focal_length": FOCAL}
x = pb.leaves({"pos": nc.lifted(nc.draw_depth(rng, B, S, S), data)}, dev)
cams = {k: torch.tensor(data[k], device=dev, requires_grad=True) for k in dco.CAMERA_KEYS}
ups = {"normal": torch.tensor(rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32), device=dev)}
everything = dict(x, **cams)


def camera(tensors):
    return dict(data, **{k: tensors[k] for k in dco.CAMERA_KEYS}) if tensors else data


def fused(t, tensors, **kw):
    return {"normal": estimate_surface_normals_plane_fit_batched(t["pos"], camera(tensors), frame="world", **kw)}


def composition(t):
    return {"normal": dco.plane_fit(t["pos"], camera(t), "world")}


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
out = {"workload": "world_normals_camera_grad_fwd_bwd", "views": B, "size": S, "rounds": args.rounds,
       "window_s_at_least": args.window, "calls_per_window": calls}
out.update({name: pb.spread(ts) for name, ts in times.items()})
out["camera_grad_over_detached"] = round(med["camera_grad"] / med["detached"], 3)
out["price_of_the_feature_ms"] = round(med["camera_grad"] - med["detached"], 4)
out["price_beyond_spread"] = bool(min(times["camera_grad"]) > max(times["detached"]))
out["speedup_over_composition_median"] = round(med["composition"] / med["camera_grad"], 2)
out["faster_than_composition_beyond_spread"] = bool(max(times["camera_grad"]) < min(times["composition"]))
out["camera_gradients_against_float64_composition"] = agree
print(json.dumps(out))
