#!/usr/bin/env python3
"""camera_grad=True of projection_renderer_differentiable_camera against projection_renderer_differentiable, and --
where it fits -- against the float32 torch composition a caller would otherwise run for a pose gradient, forward +
backward, on the GPU.

Workload: tools/bench_dense_projection.py's (B views at S x S with D = 3, rgb and the rotated image as [B, S, S, D],
blur_size 0.15, surfels / rgb / rotated_image all requiring grad, the loss a random weighting of out and mask).  Forms,
in one process, alternating round by round after a warm-up so that all see the same machine state:
    camera_grad   projection_renderer_differentiable_camera with camera_grad=True and eye, at, up as fp32 GPU leaves: k_dproj_surfel_bwd<D, true, true>,
                  the finish kernel, and the fp64 autograd chain through lookat on the host
    detached      projection_renderer_differentiable with the camera as data -- camera_grad minus detached is the price of the feature
    composition   (--composition; it holds a [B, P, N] weight, so 8 views at 48 x 48 fit and 64 at 128 x 128 do not)
                  tests/dense_camera_oracle.py's project with the same leaves, in float32 on the same GPU
Each round times a window of at least --window seconds per form with device events.  One JSON line: the median ms per
batch of each form with its run-to-run spread (min .. max over the rounds), the price of the feature, and with the
composition the ratio to it and how far the camera gradients of camera_grad and of the composition are from the
composition evaluated once in float64 on the same inputs (max|form - fp64| / max|fp64| per tensor).
Fails without a GPU."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import dense_camera_oracle as dco  # noqa: E402
import dense_projection_oracle as do  # noqa: E402
from surf_renderer_amd import projection_renderer_differentiable  # noqa: E402
from surf_renderer_amd import projection_renderer_differentiable_camera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--size", type=int, default=48)
ap.add_argument("--composition", action="store_true", help="also time the float32 torch composition")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_dense_camera: no GPU")
dev = torch.device("cuda:0")
B, S, D, BLUR = args.views, args.size, 3, 0.15
rng, data, host = pb.surfel_workload(B, S, D)
x = pb.leaves(host, dev)
cams = {k: torch.tensor(data[k], device=dev, requires_grad=True) for k in dco.CAMERA_KEYS}
ups = pb.upstreams(rng, do.OUTPUTS, B, S, D, dev)
everything = dict(x, **cams)


def camera(tensors):
    return dict(data, **{k: tensors[k] for k in dco.CAMERA_KEYS}) if tensors else data


def fused(t, tensors, **kw):
    fn = projection_renderer_differentiable_camera if kw else projection_renderer_differentiable
    out, mask = fn(t["surfels"], t["rgb"], camera(tensors), t["rotated_image"], blur_size=BLUR, **kw)
    return {"out": out, "mask": mask}


def composition(t):
    return dco.project(t["surfels"], t["rgb"], camera(t), t["rotated_image"], BLUR)


values = {}


def run(name, fn):
    pb.clear(everything)
    values[name] = fn()
    pb.loss(values[name], ups).backward()


forms = {"camera_grad": lambda: run("camera_grad", lambda: fused(x, cams, camera_grad=True)),
         "detached": lambda: run("detached", lambda: fused(x, None))}
agree = {}
if args.composition:
    forms["composition"] = lambda: run("composition", lambda: composition(everything))
    want_v, want_g = pb.composition_fp64(composition, everything, ups)
for name, fn in forms.items():                                # warm-up, and the camera gradients against float64
    fn(); fn()
    torch.cuda.synchronize()
    if args.composition and name != "detached":
        agree[name] = pb.agreement(values[name], cams, want_v, want_g, (), share=False)
calls, times, med = pb.timed(forms, args.rounds, args.window)
out = {"workload": "dense_projection_camera_grad_fwd_bwd", "views": B, "size": S, "channels": D, "blur_size": BLUR,
       "rounds": args.rounds, "window_s_at_least": args.window, "calls_per_window": calls}
out.update({name: pb.spread(ts) for name, ts in times.items()})
out["camera_grad_over_detached"] = round(med["camera_grad"] / med["detached"], 3)
out["price_of_the_feature_ms"] = round(med["camera_grad"] - med["detached"], 4)
out["price_beyond_spread"] = bool(min(times["camera_grad"]) > max(times["detached"]))
if args.composition:
    out["speedup_over_composition_median"] = round(med["composition"] / med["camera_grad"], 2)
    out["faster_than_composition_beyond_spread"] = bool(max(times["camera_grad"]) < min(times["composition"]))
    out["camera_gradients_against_float64_composition"] = agree
print(json.dumps(out))
