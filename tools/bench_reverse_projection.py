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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
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
host = {"rgb": rng.uniform(0, 1, (B, S, S, D)), "in_pos_wc": cases.seen(*cams[0], S, S, *cases.CAMERAS[0]),
        "out_pos_wc": cases.seen(*cams[1], S, S, *cases.CAMERAS[1]), "rotated_image": rng.uniform(0, 1, (B, S, S, D))}
x = {k: torch.tensor(v.astype(np.float32), device=dev, requires_grad=True) for k, v in host.items()}
ups = {k: torch.tensor(rng.uniform(-1, 1, (B, S, S, D if k in ("out", "image1") else 1)).astype(np.float32), device=dev)
       for k in TIMED}
values = {}


def clear():
    for t in x.values():
        t.grad = None


def loss(res):
    return sum((res[k] * ups[k]).sum() for k in TIMED)


def fused():
    clear()
    out, proj_out = projection_reverse_renderer(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], *camera,
                                                rotated_image=x["rotated_image"], **FLAGS)
    values["fused"] = dict(proj_out, out=out)
    loss(values["fused"]).backward()


def composition():
    clear()
    values["composition"] = ro.project(x["rgb"], x["in_pos_wc"], x["out_pos_wc"], *camera, x["rotated_image"], **FLAGS)
    loss(values["composition"]).backward()


def composition_fp64():
    """({output: value}, {input: gradient}) of the composition in float64 on the same float32 inputs; not timed."""
    x64 = {k: t.detach().double().requires_grad_(True) for k, t in x.items()}
    res = ro.project(x64["rgb"], x64["in_pos_wc"], x64["out_pos_wc"], *camera, x64["rotated_image"], **FLAGS)
    sum((res[k] * ups[k].double()).sum() for k in TIMED).backward()
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


def snapshot(name):
    torch.cuda.synchronize()
    return [values[name][k].detach().clone() for k in ro.OUTPUTS] + [t.grad.clone() for t in x.values()]


forms = {"fused": fused, "composition": composition}
want_v, want_g = composition_fp64()
agree, repeatable = {}, {}
for name, fn in forms.items():                                # warm-up, each form against float64 and against itself
    fn()
    first = snapshot(name)
    fn()
    repeatable[name] = all(bool(torch.equal(a, b)) for a, b in zip(first, snapshot(name)))
    got = {"value_" + k: (values[name][k].detach().double(), want_v[k]) for k in ro.OUTPUTS}
    got.update({"grad_" + k: (t.grad.double(), want_g[k]) for k, t in x.items()})
    agree[name] = {k: {"max_err_over_max": float(f"{float((a - b).abs().max() / b.abs().max()):.3g}"),
                       "share_off_by_1e-4_of_max": float(f"{float(((a - b).abs() > 1e-4 * b.abs().max()).double().mean()):.3g}")}
                   for k, (a, b) in got.items()}
del want_v, want_g, first
calls = {name: max(1, int(np.ceil(1e3 * args.window / window(fn, 3)))) for name, fn in forms.items()}
times = {name: [] for name in forms}
for _ in range(args.rounds):
    for name, fn in forms.items():
        times[name].append(window(fn, calls[name]))
med = {name: float(np.median(ts)) for name, ts in times.items()}
out = {"workload": "reverse_projection_fwd_bwd", "views": B, "size": S, "channels": D, "rounds": args.rounds,
       "window_s_at_least": args.window, "calls_per_window": calls,
       "mask_mean": round(float(values["fused"]["mask"].detach().mean()), 4)}
for name, ts in times.items():
    out[name] = {"ms_per_batch": round(med[name], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                 "spread_ms": round(max(ts) - min(ts), 4), "two_calls_bit_identical": repeatable[name]}
out["speedup_median"] = round(med["composition"] / med["fused"], 2)
# faster by more than the spread: the slowest fused round against the fastest round of the composition
out["fused_faster_beyond_spread"] = bool(max(times["fused"]) < min(times["composition"]))
out["against_float64_composition"] = agree
print(json.dumps(out))
