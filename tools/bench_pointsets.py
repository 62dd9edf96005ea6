#!/usr/bin/env python3
"""hausdorff_batched and a two-sided Chamfer sum through nearest_points against the two float32 torch formulations a
user has without them, forward + backward, on the GPU.

Workloads (both on u, v [B, N, 3] that require grad, normal variates, v scaled 1.1 and shifted 0.2):
    hausdorff    loss = hausdorff_batched(u, v)[0].sum()
    chamfer      loss = dist_u.mean(-1).sum() + dist_v.mean(-1).sum()
Forms, in one process, alternating round by round after a warm-up so that all see the same machine state:
    fused        nearest_points (HIP kernels; the stable sort of the backward is torch's)
    reference    the reference's formulation, sqrt(sum((u[:, :, None] - v[:, None]) ** 2, -1)) with min over each axis:
                 a [B, N, M, 3] difference tensor
    cdist        torch.cdist(u, v) with min over each axis: a [B, N, M] distance matrix
The comparison runs at --views x --size^2 points (8 x 48^2 by default, where the reference's pair tensor, 510 MB, still
fits); the fused form alone then runs at --big-views x --big-size^2 (64 x 128^2), where it reports its peak allocated
memory (beside what was allocated before the call: the leaves, their gradients and what the warm-up left) and the
forward kernel's time against its fp64 issue-rate floor: the forward streams N M pairs per view and
direction at FP64_PER_PAIR fp64 wave-instructions per 64 pairs (counted in profiles/pointsets_isa_meta.txt), and a SIMD
issues one fp64 instruction per NS_PER_FP64 ns (profiles/r02_ubench_valu.txt: v_add / v_mul / v_fma_f64).
Each round times a window of at least --window seconds per form with device events; the rounds are run --runs times
(twice by default) and every run is reported, one JSON line each.  Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
from surf_renderer_amd import hausdorff_batched, nearest_points  # noqa: E402

FP64_PER_PAIR, NS_PER_FP64, SIMDS = 7.75, 1.92, 256 * 4

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--size", type=int, default=48)
ap.add_argument("--big-views", type=int, default=64)
ap.add_argument("--big-size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_pointsets: no GPU")
dev = torch.device("cuda:0")


def clouds(B, N):
    rng = np.random.RandomState(0)
    return pb.leaves({"u": rng.standard_normal((B, N, 3)), "v": rng.standard_normal((B, N, 3)) * 1.1 + 0.2}, dev)


def nearest_fused(x):
    r = nearest_points(x["u"], x["v"])
    return r.dist_u, r.dist_v


def nearest_reference(x):
    D = torch.sqrt(torch.sum((x["u"][:, :, None, :] - x["v"][:, None, :, :]) ** 2, dim=-1))
    return D.min(dim=2).values, D.min(dim=1).values


def nearest_cdist(x):
    D = torch.cdist(x["u"], x["v"])
    return D.min(dim=2).values, D.min(dim=1).values


def hausdorff_of(nearest):
    def loss(x):
        dist_u, dist_v = nearest(x)
        return torch.maximum(dist_v.amax(dim=-1), dist_u.amax(dim=-1)).sum()
    return loss


def chamfer_of(nearest):
    return lambda x: sum(d.mean(dim=-1).sum() for d in nearest(x))


NEAREST = {"fused": nearest_fused, "reference": nearest_reference, "cdist": nearest_cdist}
WORKLOADS = {"hausdorff": hausdorff_of, "chamfer": chamfer_of}


def step(x, loss):
    pb.clear(x)
    loss(x).backward()


B, N = args.views, args.size ** 2
x = clouds(B, N)
assert float(hausdorff_batched(x["u"], x["v"])[0].sum().detach()) == float(hausdorff_of(nearest_fused)(x).detach())
for workload, of in WORKLOADS.items():
    forms = {name: (lambda f=of(fn): step(x, f)) for name, fn in NEAREST.items()}
    grads = {}
    for name, fn in forms.items():                                    # warm-up, and each form's gradient
        fn(); fn()
        torch.cuda.synchronize()
        grads[name] = x["u"].grad.double().clone()
    for r in range(args.runs):
        calls, times, med = pb.timed(forms, args.rounds, args.window)
        out = {"workload": workload + "_fwd_bwd", "run": r + 1, "views": B, "points_per_view": N, "rounds": args.rounds,
               "window_s_at_least": args.window, "calls_per_window": calls}
        out.update({name: pb.spread(ts) for name, ts in times.items()})
        out.update({"speedup_median_over_" + k: round(med[k] / med["fused"], 2) for k in ("reference", "cdist")})
        out["fused_faster_beyond_spread"] = {k: bool(max(times["fused"]) < min(times[k])) for k in ("reference", "cdist")}
        if r == 0:
            out["grad_u_max_difference_from_fused_over_max"] = {
                k: float(f"{float((grads[k] - grads['fused']).abs().max() / grads['fused'].abs().max()):.3g}")
                for k in ("reference", "cdist")}
        print(json.dumps(out), flush=True)
del x, forms, grads

# the fused form alone, where no pair tensor fits
B, N = args.big_views, args.big_size ** 2
x = clouds(B, N)
floor_ms = 2.0 * B * N * N / 64.0 * FP64_PER_PAIR * NS_PER_FP64 / SIMDS * 1e-6
for workload, of in WORKLOADS.items():
    loss = of(nearest_fused)
    forms = {"fused": lambda: step(x, loss), "fused_forward": lambda: nearest_points(x["u"].detach(), x["v"].detach())}
    for fn in forms.values():
        fn(); fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    forms["fused"]()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    for r in range(args.runs):
        calls, times, med = pb.timed(forms, args.rounds, args.window)
        out = {"workload": workload + "_fwd_bwd_large", "run": r + 1, "views": B, "points_per_view": N,
               "rounds": args.rounds, "window_s_at_least": args.window, "calls_per_window": calls}
        out.update({name: pb.spread(ts) for name, ts in times.items()})
        out.update({"peak_allocated_MB": round(peak / 1e6, 1), "allocated_before_the_call_MB": round(base / 1e6, 1),
                    "pair_tensor_MB_reference": round(B * N * N * 3 * 4 / 1e6), "forward_fp64_issue_floor_ms": round(floor_ms, 3),
                    "forward_over_floor": round(med["fused_forward"] / floor_ms, 2)})
        print(json.dumps(out), flush=True)
