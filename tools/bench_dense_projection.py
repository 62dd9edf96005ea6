#!/usr/bin/env python3
"""projection_renderer_differentiable on the GPU: against the torch composition it replaces where that fits, and alone
at the project's standing layer workload.

Inputs: B views at S x S with D = 3, rgb and the rotated image as [B, S, S, D], blur_size 0.15 (sigma = 0.025 S pixels),
surfels / rgb / rotated_image all requiring grad, the loss a random weighting of out and mask.  The surfels are a
jittered depth map seen from the target cameras (tools/projection_bench.surfel_workload).

    --mode compare   (default 8 views at 48 x 48)  two forms in one process, alternating round by round after a warm-up:
        fused        one projection_renderer_differentiable call and its backward (5 HIP kernel launches)
        composition  the reference's dense formulation -- the [B, P, N] weight and one matrix product -- as tests/
                     dense_projection_oracle.py restates it, in float32 on the same GPU, one backward
      and how far each is from the same composition evaluated once in float64 (max|form - fp64| / max|fp64| per array).
    --mode headline  (default 64 views at 128 x 128)  fused only, where the composition's weight alone would take
      B P N 4 bytes: the forward alone (under no_grad) and forward + backward, torch.cuda.max_memory_allocated over one
      forward + backward, and the forward's and backward's fp64 instruction-issue floors
      (pairs x instructions per pair x 1.963 ns per wave-instruction per SIMD / 64 lanes / 1024 SIMDs; the 1.963 ns
      is profiles/r02_ubench_valu.txt's v_fma_f64 figure -- a microbenchmark, not this kernel).

Each round times a window of at least --window seconds per form with device events.  One JSON line: the median ms per
batch of each form and the run-to-run spread (min .. max over the rounds).  Fails without a GPU."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import dense_projection_oracle as do  # noqa: E402
from surf_renderer_amd import projection_renderer_differentiable  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("compare", "headline"), default="compare")
ap.add_argument("--views", type=int)
ap.add_argument("--size", type=int)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_dense_projection: no GPU")
dev = torch.device("cuda:0")
B = args.views or (8 if args.mode == "compare" else 64)
S = args.size or (48 if args.mode == "compare" else 128)
D, N, BLUR = 3, S * S, 0.15
FMA_NS = 1.963                     # per wave-instruction per SIMD
rng, camera, host = pb.surfel_workload(B, S, D)
x = pb.leaves(host, dev)
ups = pb.upstreams(rng, do.OUTPUTS, B, S, D, dev)
values = {}


def fused():
    pb.clear(x)
    out, mask = projection_renderer_differentiable(x["surfels"], x["rgb"], camera, x["rotated_image"], blur_size=BLUR)
    values["fused"] = {"out": out, "mask": mask}
    pb.loss(values["fused"], ups).backward()


def fused_forward():
    with torch.no_grad():
        projection_renderer_differentiable(x["surfels"], x["rgb"], camera, x["rotated_image"], blur_size=BLUR)


def project(x):
    return do.project(x["surfels"], x["rgb"], camera, x["rotated_image"], BLUR)


def composition():
    pb.clear(x)
    values["composition"] = project(x)
    pb.loss(values["composition"], ups).backward()


out = {"workload": "dense_projection_" + args.mode, "views": B, "size": S, "channels": D, "blur_size": BLUR,
       "sigma_pixels": BLUR * S / 6, "rounds": args.rounds, "window_s_at_least": args.window}
if args.mode == "compare":
    forms = {"fused": fused, "composition": composition}
    want_v, want_g = pb.composition_fp64(project, x, ups)
    agree = {}
    for name, fn in forms.items():                                # warm-up, and each form against float64
        fn(); fn()
        torch.cuda.synchronize()
        agree[name] = pb.agreement(values[name], x, want_v, want_g, do.OUTPUTS, share=False)
    del want_v, want_g
    out["max_err_over_max_against_float64_composition"] = agree
else:
    forms = {"fused_forward": fused_forward, "fused": fused}
    for fn in forms.values():
        fn(); fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fused()
    torch.cuda.synchronize()
    out["memory"] = {"allocated_before_mb": round(before / 2 ** 20, 1),
                     "max_allocated_during_fwd_bwd_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
                     "composition_weight_alone_gb": round(B * N * N * 4 / 1e9, 1),
                     "composition_weight_and_product_gb": round(B * N * N * 4 * (1 + D) / 1e9, 1)}
calls, times, med = pb.timed(forms, args.rounds, args.window)
out["calls_per_window"] = calls
out.update({name: pb.spread(ts) for name, ts in times.items()})
if args.mode == "compare":
    out.update(pb.against_composition(times, med))
else:
    pairs = float(B) * N * N
    floor = {"forward": pairs * (D + 2) * FMA_NS / 64 / 1024 * 1e-6, "backward": pairs * 2 * (D + 1) * FMA_NS / 64 / 1024 * 1e-6}
    bwd = med["fused"] - med["fused_forward"]
    out["pairs"] = pairs
    out["issue_floor_ms"] = {k: round(v, 3) for k, v in floor.items()}
    out["achieved_over_floor"] = {"forward": round(med["fused_forward"] / floor["forward"], 2),
                                  "backward_as_total_less_forward": round(bwd / floor["backward"], 2)}
print(json.dumps(out))
