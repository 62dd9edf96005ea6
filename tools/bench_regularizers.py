#!/usr/bin/env python3
"""splat_regularizers against the torch composition it replaces, forward + backward, on the GPU.

Workload: B = 64 views at 128 x 128 (the README's splat batch), pos / normal / image / depth all requiring grad, the
loss a weighted sum of all seven terms over the batch.  Two forms, in one process, alternating round by round after a
warm-up so that both see the same machine state:
    fused        one splat_regularizers call (srh_regularizers_fwd, two launches) and one backward launch
    composition  the same terms from tests/regularizer_oracle.py in float32 on the same GPU, evaluated per view as the
                 trainers do (diffrend/torch/GAN/gan.py:601-640), summed, one backward
Each round times a window of at least --window seconds per form with device events.  One JSON line: the median
ms per batch of each form, the run-to-run spread (min .. max over the rounds) of both, their ratio, and the largest
disagreement of the two forms' values and gradients (fp32 composition against fp64-arithmetic kernels).
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
import regularizer_oracle as ro  # noqa: E402
from surf_renderer_amd import REGULARIZER_TERMS, splat_regularizers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_regularizers: no GPU")
dev = torch.device("cuda:0")
B, S = args.views, args.size
Z_MIN, Z_MAX = 2.0, 4.0
rng = np.random.RandomState(0)
host = {"pos": np.stack([rng.uniform(-1, 1, (B, S, S)), rng.uniform(-1, 1, (B, S, S)), -rng.uniform(1.5, 4.5, (B, S, S))], -1),
        "normal": rng.uniform(-1, 1, (B, S, S, 3)), "image": rng.uniform(0, 1, (B, S, S, 3)),
        "depth": rng.uniform(1, 5, (B, S, S))}
x = {k: torch.tensor(v.astype(np.float32), device=dev, requires_grad=True) for k, v in host.items()}
w = torch.tensor((rng.uniform(0.5, 2.0, (B, 7)) * rng.choice([-1.0, 1.0], (B, 7))).astype(np.float32), device=dev)
values = {}


def clear():
    for t in x.values():
        t.grad = None


def fused():
    clear()
    terms = splat_regularizers(x, Z_MIN, Z_MAX)
    values["fused"] = terms
    sum((w[:, k] * terms[name]).sum() for k, name in enumerate(REGULARIZER_TERMS)).backward()


def composition():
    clear()
    loss, per_view = 0.0, []
    for b in range(B):
        t = ro.terms(x["pos"][b], x["normal"][b], x["image"][b], x["depth"][b], Z_MIN, Z_MAX)
        per_view.append(t)
        loss = loss + sum(w[b, k] * t[name] for k, name in enumerate(ro.TERMS))
    values["composition"] = {k: torch.stack([t[k] for t in per_view]) for k in ro.TERMS}
    loss.backward()


def window(fn, n):
    """ms per call over n calls, by device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n


forms = {"fused": fused, "composition": composition}
agree = {}
grads = {}
for name, fn in forms.items():                                # warm-up, and the two forms' results side by side
    fn(); fn()
    torch.cuda.synchronize()
    grads[name] = {k: t.grad.clone() for k, t in x.items()}
for k in REGULARIZER_TERMS:
    a, b = values["fused"][k].detach().double(), values["composition"][k].detach().double()
    agree["value_" + k] = float(((a - b).abs() / b.abs().clamp_min(1e-30)).max())
for k in x:
    a, b = grads["fused"][k].double(), grads["composition"][k].double()
    agree["grad_" + k] = float((a - b).abs().max() / b.abs().max())
calls = {name: max(1, int(np.ceil(1e3 * args.window / window(fn, 3)))) for name, fn in forms.items()}
times = {name: [] for name in forms}
for _ in range(args.rounds):
    for name, fn in forms.items():
        times[name].append(window(fn, calls[name]))
med = {name: float(np.median(ts)) for name, ts in times.items()}
out = {"workload": "splat_regularizers_fwd_bwd", "views": B, "size": S, "rounds": args.rounds,
       "window_s_at_least": args.window, "calls_per_window": calls}
for name, ts in times.items():
    out[name] = {"ms_per_batch": round(med[name], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                 "spread_ms": round(max(ts) - min(ts), 4)}
out["speedup_median"] = round(med["composition"] / med["fused"], 2)
# faster by more than the spread: the slowest fused round against the fastest round of the composition
out["fused_faster_beyond_spread"] = bool(max(times["fused"]) < min(times["composition"]))
out["max_rel_disagreement_between_forms"] = {k: float(f"{v:.3g}") for k, v in agree.items()}
print(json.dumps(out))
