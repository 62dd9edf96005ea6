#!/usr/bin/env python3
"""projection_renderer_differentiable on the GPU: against the torch composition it replaces where that fits, and alone
at the project's standing layer workload.

Inputs: B views at S x S with D = 3, rgb and the rotated image as [B, S, S, D], blur_size 0.15 (sigma = 0.025 S pixels),
surfels / rgb / rotated_image all requiring grad, the loss a random weighting of out and mask.  The surfels are a
jittered depth map seen from the target cameras (tests/projection_cases.lift).

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

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import dense_projection_oracle as do  # noqa: E402
from projection_cases import FOCAL, FOVY, lift  # noqa: E402
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
rng = np.random.RandomState(0)
eye = (rng.uniform(-0.5, 0.5, (B, 3)) + [0.0, 0.5, 4.0]).astype(np.float32)
at = rng.uniform(-0.3, 0.3, (B, 3)).astype(np.float32)
up = (rng.uniform(-0.2, 0.2, (B, 3)) + [0.0, 1.0, 0.0]).astype(np.float32)
gy, gx = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
world = lift(gx.reshape(1, N) + rng.uniform(-1.2, 1.2, (B, N)), gy.reshape(1, N) + rng.uniform(-1.2, 1.2, (B, N)),
             rng.uniform(1.5, 3.0, (B, N)), eye, at, up, S, S)
camera = {"eye": eye, "at": at, "up": up, "viewport": [0, 0, S, S], "fovy": float(FOVY), "focal_length": FOCAL}
host = {"surfels": world, "rgb": rng.uniform(0, 1, (B, S, S, D)), "rotated_image": rng.uniform(0, 1, (B, S, S, D))}
x = {k: torch.tensor(v.astype(np.float32), device=dev, requires_grad=True) for k, v in host.items()}
ups = {"out": torch.tensor(rng.uniform(-1, 1, (B, S, S, D)).astype(np.float32), device=dev),
       "mask": torch.tensor(rng.uniform(-1, 1, (B, S, S, 1)).astype(np.float32), device=dev)}
values = {}


def clear():
    for t in x.values():
        t.grad = None


def loss(res):
    return sum((res[k] * ups[k]).sum() for k in do.OUTPUTS)


def fused():
    clear()
    out, mask = projection_renderer_differentiable(x["surfels"], x["rgb"], camera, x["rotated_image"], blur_size=BLUR)
    values["fused"] = {"out": out, "mask": mask}
    loss(values["fused"]).backward()


def fused_forward():
    with torch.no_grad():
        projection_renderer_differentiable(x["surfels"], x["rgb"], camera, x["rotated_image"], blur_size=BLUR)


def composition():
    clear()
    values["composition"] = do.project(x["surfels"], x["rgb"], camera, x["rotated_image"], BLUR)
    loss(values["composition"]).backward()


def composition_fp64():
    """({output: value}, {input: gradient}) of the composition in float64 on the same float32 inputs; not timed."""
    x64 = {k: t.detach().double().requires_grad_(True) for k, t in x.items()}
    res = do.project(x64["surfels"], x64["rgb"], camera, x64["rotated_image"], BLUR)
    sum((res[k] * ups[k].double()).sum() for k in do.OUTPUTS).backward()
    return {k: v.detach() for k, v in res.items()}, {k: t.grad for k, t in x64.items()}


def window(fn, n):
    """ms per call over n calls, by device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n


out = {"workload": "dense_projection_" + args.mode, "views": B, "size": S, "channels": D, "blur_size": BLUR,
       "sigma_pixels": BLUR * S / 6, "rounds": args.rounds, "window_s_at_least": args.window}
if args.mode == "compare":
    forms = {"fused": fused, "composition": composition}
    want_v, want_g = composition_fp64()
    agree = {}
    for name, fn in forms.items():                                # warm-up, and each form against float64
        fn(); fn()
        torch.cuda.synchronize()
        got = {"value_" + k: (values[name][k].detach().double(), want_v[k]) for k in do.OUTPUTS}
        got.update({"grad_" + k: (t.grad.double(), want_g[k]) for k, t in x.items()})
        agree[name] = {k: float(f"{float((a - b).abs().max() / b.abs().max()):.3g}") for k, (a, b) in got.items()}
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
calls = {name: max(1, int(np.ceil(1e3 * args.window / window(fn, 3)))) for name, fn in forms.items()}
times = {name: [] for name in forms}
for _ in range(args.rounds):
    for name, fn in forms.items():
        times[name].append(window(fn, calls[name]))
med = {name: float(np.median(ts)) for name, ts in times.items()}
out["calls_per_window"] = calls
for name, ts in times.items():
    out[name] = {"ms_per_batch": round(med[name], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                 "spread_ms": round(max(ts) - min(ts), 4)}
if args.mode == "compare":
    out["speedup_median"] = round(med["composition"] / med["fused"], 2)
    # faster by more than the spread: the slowest fused round against the fastest round of the composition
    out["fused_faster_beyond_spread"] = bool(max(times["fused"]) < min(times["composition"]))
else:
    pairs = float(B) * N * N
    floor = {"forward": pairs * (D + 2) * FMA_NS / 64 / 1024 * 1e-6, "backward": pairs * 2 * (D + 1) * FMA_NS / 64 / 1024 * 1e-6}
    bwd = med["fused"] - med["fused_forward"]
    out["pairs"] = pairs
    out["issue_floor_ms"] = {k: round(v, 3) for k, v in floor.items()}
    out["achieved_over_floor"] = {"forward": round(med["fused_forward"] / floor["forward"], 2),
                                  "backward_as_total_less_forward": round(bwd / floor["backward"], 2)}
print(json.dumps(out))
