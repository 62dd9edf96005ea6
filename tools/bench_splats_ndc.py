#!/usr/bin/env python3
"""render_splats_NDC_batch against the torch composition it replaces, forward + backward, on the GPU.

Workload: B = 64 views at 128 x 128, 2 lights, 2 materials; z [B, N] and the normals [B, N, 4] require grad (what
optimize_NDC_test hands to Adam: pos is stacked from the fixed pixel grid and z on every call), the loss an L1 loss on
`image` against a fixed target.  Two forms, in one process, alternating round by round after a warm-up so that both see
the same machine state:
    fused        one render_splats_NDC_batch call (one srh_splat_ndc_fwd launch) and one backward launch
    composition  tests/splats_ndc_oracle.py's restatement of the reference in float32 on the same GPU, one view at a
                 time as the reference's callers do, the losses summed, one backward
Each round times a window of at least --window seconds per form with device events.  One JSON line: the median ms per
batch of each form, the run-to-run spread (min .. max over the rounds) of both, their ratio, and the largest
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
import splats_ndc_oracle as oracle  # noqa: E402
from surf_renderer_amd import render_splats_NDC_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_splats_ndc: no GPU")
dev = torch.device("cuda:0")
B, S = args.views, args.size
N = S * S
rng = np.random.RandomState(0)


def gpu(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=dev, requires_grad=grad)


gx, gy = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S))
xy = gpu(np.stack((gx.ravel(), gy.ravel()), -1))                                   # (N, 2), shared by the views
z = gpu(rng.uniform(-0.9, 0.9, (B, N)), grad=True)
nrm = np.concatenate((rng.uniform(-0.3, 0.3, (B, N, 2)), rng.uniform(0.8, 1.1, (B, N, 1)), np.zeros((B, N, 1))), -1)
normal = gpu(nrm, grad=True)
eye = np.stack([[0.5 + 0.03 * b, 1.0 - 0.02 * b, 6.0, 1.0] for b in range(B)]).astype(np.float32)
scene = {
    "camera": {"viewport": [0, 0, S, S], "fovy": float(np.deg2rad(45.0)), "near": 1.0, "far": 10.0, "eye": eye,
               "at": np.array([0.1, -0.2, 0.0, 1.0], np.float32), "up": np.array([0.2, 1.0, 0.3, 0.0], np.float32)},
    "lights": {"pos": gpu([[3.0, 4.0, 8.0, 1.0], [-4.0, 1.0, 1.0, 1.0]]), "color_idx": torch.tensor([1, 2], device=dev),
               "attenuation": gpu([[1.0, 0.0, 0.0], [0.6, 0.04, 0.003]]), "ambient": gpu([0.05, 0.04, 0.06])},
    "colors": gpu([[0, 0, 0], [0.9, 0.8, 0.7], [0.3, 0.5, 0.9]]),
    "materials": {"albedo": gpu([[0.7, 0.6, 0.5], [0.3, 0.8, 0.4]]), "coeffs": gpu([[0.8, 0.2, 5.0], [0.6, 0.4, 12.0]])},
    "objects": {"disk": {"material_idx": torch.tensor((rng.uniform(size=N) < 0.4).astype(np.int64), device=dev)}},
}
target = gpu(rng.uniform(0, 1, (B, S, S, 3)))
criterion = torch.nn.L1Loss()
values = {}


def positions():
    return torch.cat((xy.unsqueeze(0).expand(B, N, 2), z.unsqueeze(-1)), dim=2)


def clear():
    z.grad = normal.grad = None


def fused():
    clear()
    scene["objects"]["disk"].update(pos=positions(), normal=normal)
    res = render_splats_NDC_batch(scene)
    values["fused"] = res["image"]
    criterion(res["image"], target).backward()


_SHADING = {"lights.pos": scene["lights"]["pos"], "colors": scene["colors"],
            "lights.attenuation": scene["lights"]["attenuation"], "lights.ambient": scene["lights"]["ambient"],
            "materials.albedo": scene["materials"]["albedo"], "materials.coeffs": scene["materials"]["coeffs"]}


def composition():
    clear()
    pos = positions()
    loss, images = 0.0, []
    for b in range(B):
        sc = dict(scene, camera=dict(scene["camera"], eye=eye[b]))
        res = oracle.render(sc, dict(_SHADING, **{"disk.pos": pos[b], "disk.normal": normal[b]}))
        images.append(res["image"])
        loss = loss + criterion(res["image"], target[b]) / B
    values["composition"] = torch.stack(images)
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
agree, grads = {}, {}
for name, fn in forms.items():                                # warm-up, and the two forms' results side by side
    fn(); fn()
    torch.cuda.synchronize()
    grads[name] = {"z": z.grad.clone(), "normal": normal.grad.clone()}
a, b = values["fused"].detach().double(), values["composition"].detach().double()
agree["value_image"] = float((a - b).abs().max() / b.abs().max())
for k in ("z", "normal"):
    a, b = grads["fused"][k].double(), grads["composition"][k].double()
    agree["grad_" + k] = float((a - b).abs().max() / b.abs().max())
calls = {name: max(1, int(np.ceil(1e3 * args.window / window(fn, 3)))) for name, fn in forms.items()}
times = {name: [] for name in forms}
for _ in range(args.rounds):
    for name, fn in forms.items():
        times[name].append(window(fn, calls[name]))
med = {name: float(np.median(ts)) for name, ts in times.items()}
out = {"workload": "render_splats_NDC_fwd_bwd", "views": B, "size": S, "rounds": args.rounds,
       "window_s_at_least": args.window, "calls_per_window": calls}
for name, ts in times.items():
    out[name] = {"ms_per_batch": round(med[name], 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                 "spread_ms": round(max(ts) - min(ts), 4)}
out["speedup_median"] = round(med["composition"] / med["fused"], 2)
# faster by more than the spread: the slowest fused round against the fastest round of the composition
out["fused_faster_beyond_spread"] = bool(max(times["fused"]) < min(times["composition"]))
out["max_rel_disagreement_between_forms"] = {k: float(f"{v:.3g}") for k, v in agree.items()}
print(json.dumps(out))
