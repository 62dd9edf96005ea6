#!/usr/bin/env python3
"""radiance_SH9_batched and irradiance_batched against the same formulas composed in float32 torch on the same GPU, and
the projection against the reference's formulation in numpy on one host core (tests/sh9_oracle.py's restatement of it:
the reference itself is not needed).

Workloads:
    projection   a --probe^2 x 3 probe, values uniform in [0, 2], alone and as a batch of --probe-views;
                 loss = sum(L g_L).  Forms: forward, and forward + backward with the probe as the leaf.
    irradiance   --views x --size^2 normals, C = 3, an M per view; loss = sum(E g_E).  Forms: forward + backward with
                 normal and M as leaves, and with M detached (the kernel variant without the reduction).
Forms, in one process, alternating round by round after a warm-up so that all see the same machine state:
    fused        the HIP kernels
    torch        the composition: the pixel grid, atan2, sin, cos and the nine harmonics made on the device in every
                 call, as the reference makes them on the host; float32
Each round times a window of at least --window seconds per form with device events; the rounds are run --runs times
(twice by default) and every run is reported, one JSON line each.  `bytes_fused` is what the fused call must move (the
probe read or its gradient written once; normals, upstream gradients, E and the normals' gradient once each), and
`GBps_whole_call` that over the whole call's time, launches and torch's allocations included -- not a kernel's rate.
--once runs every fused call three times and exits: the workload of a kernel trace.  Fails without a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import sh9_oracle as oracle  # noqa: E402
from surf_renderer_amd import irradiance_batched, radiance_SH9_batched  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--probe", type=int, default=1000)
ap.add_argument("--probe-views", type=int, default=8)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
ap.add_argument("--once", action="store_true", help="three calls of every fused form and nothing else")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_sh_lighting: no GPU")
dev = torch.device("cuda:0")
C = 3


def torch_project(env):
    """radiance_SH9's formulas on a batch, float32 on the device, the mask applied by multiplication as the reference's"""
    B, H, W, _ = env.shape
    i = torch.arange(H, device=env.device, dtype=torch.float32)[:, None]
    j = torch.arange(W, device=env.device, dtype=torch.float32)[None, :]
    v, u = (W / 2.0 - i) / (W / 2.0) + 0 * j, (j - H / 2.0) / (H / 2.0) + 0 * i
    r = torch.sqrt(u ** 2 + v ** 2)
    theta, phi = np.pi * r, torch.atan2(v, u)
    domega = (2 * np.pi / W) * (2 * np.pi / H) * torch.sinc(theta)
    X, Y, Z = torch.cos(phi) * torch.sin(theta), torch.sin(phi) * torch.sin(theta), torch.cos(theta)
    basis = oracle.real_sh9_cart(X, Y, Z, torch) * (domega * (r <= 1.0))[..., None]
    return torch.einsum("bijc,ijk->bck", env, basis)


def torch_irradiance(M, n):
    a = torch.einsum("bnr,brsc->bnsc", n, M[:, :3]) + M[:, None, 3]
    return (a[:, :, :3] * n[..., None]).sum(2) + a[:, :, 3]


def step(x, fn, up):
    pb.clear(x)
    (fn() * up).sum().backward()


def report(workload, shape, forms, pairs, extra):
    for fn in forms.values():
        fn(); fn()
    torch.cuda.synchronize()
    for r in range(args.runs):
        calls, times, med = pb.timed(forms, args.rounds, args.window)
        out = dict({"workload": workload, "run": r + 1}, **shape, rounds=args.rounds, window_s_at_least=args.window,
                   calls_per_window=calls)
        out.update({name: pb.spread(ts) for name, ts in times.items()})
        out["ratio_of_medians"] = {f"{b}_over_{a}": round(med[b] / med[a], 2) for a, b in pairs}
        out["fused_apart_from_every_round_of"] = {b: bool(max(times[a]) < min(times[b]) or min(times[a]) > max(times[b]))
                                                   for a, b in pairs}
        out.update(extra(med))
        print(json.dumps(out), flush=True)


def projection(B):
    S = args.probe
    rng = np.random.RandomState(0)
    x = pb.leaves({"envmap": rng.uniform(0, 2, (B, S, S, C))}, dev)
    g_L = torch.tensor(rng.uniform(-1, 1, (B, C, 9)).astype(np.float32), device=dev)
    env = x["envmap"]
    forms = {"fused_forward": lambda: radiance_SH9_batched(env.detach()),
             "torch_forward": lambda: torch_project(env.detach()),
             "fused": lambda: step(x, lambda: radiance_SH9_batched(env), g_L),
             "torch": lambda: step(x, lambda: torch_project(env), g_L)}
    if args.once:
        return [f() for f in (forms["fused"],) * 3]
    # what the two forms compute, against the float64 restatement of view 0
    want, A = oracle.project(env[0].detach().cpu().numpy())
    differ = {k: float(f"{float(np.abs(f(env.detach())[0].cpu().numpy() - want).max() / np.abs(want).max()):.3g}")
              for k, f in (("fused", radiance_SH9_batched), ("torch", torch_project))}
    host = []
    probe64 = env[0].detach().cpu().numpy().astype(np.float64)
    for _ in range(3):                                           # the numpy formulation, one probe, one host core
        t0 = time.perf_counter()
        oracle.project(probe64)
        host.append(1e3 * (time.perf_counter() - t0))
    one_way = B * S * S * C * 4
    report("projection", {"views": B, "probe": [S, S, C]}, forms, [("fused_forward", "torch_forward"), ("fused", "torch")],
           lambda med: {"L_max_difference_from_float64_over_max": differ,
                        "numpy_one_probe_ms": [round(t, 1) for t in host], "numpy_threads": torch.get_num_threads(),
                        "bytes_fused": {"forward": one_way, "forward_backward": 2 * one_way},
                        "GBps_whole_call": {"forward": round(one_way / med["fused_forward"] / 1e6, 1),
                                            "forward_backward": round(2 * one_way / med["fused"] / 1e6, 1)}})


def irradiance():
    B, N = args.views, args.size ** 2
    rng = np.random.RandomState(1)
    n = rng.standard_normal((B, N, 3))
    x = pb.leaves({"normal": n / np.linalg.norm(n, axis=-1, keepdims=True), "M": rng.uniform(-1, 1, (B, 4, 4, C))}, dev)
    g_E = torch.tensor(rng.uniform(-1, 1, (B, N, C)).astype(np.float32), device=dev)
    M, nn = x["M"], x["normal"]
    forms = {"fused": lambda: step(x, lambda: irradiance_batched(M, nn), g_E),
             "torch": lambda: step(x, lambda: torch_irradiance(M, nn), g_E),
             "fused_M_detached": lambda: step(x, lambda: irradiance_batched(M.detach(), nn), g_E),
             "torch_M_detached": lambda: step(x, lambda: torch_irradiance(M.detach(), nn), g_E)}
    if args.once:
        return [f() for f in (forms["fused"], forms["fused_M_detached"]) * 3]
    grads = {}
    for name in ("fused", "torch"):
        forms[name]()
        grads[name] = M.grad[0].double().cpu().numpy()
    t = oracle.irradiance_view(M[0].detach().cpu().numpy(), nn[0].detach().cpu().numpy(), g_E[0].cpu().numpy())
    differ = {k: float(f"{float(np.abs(g - t['grad_M']).max() / np.abs(t['grad_M']).max()):.3g}") for k, g in grads.items()}
    moved = B * N * (12 + 4 * C) + B * N * (12 + 4 * C + 12)      # forward: n in, E out; backward: n, g_E in, grad_n out
    report("irradiance_fwd_bwd", {"views": B, "normals_per_view": N, "channels": C}, forms,
           [("fused", "torch"), ("fused_M_detached", "torch_M_detached")],
           lambda med: {"grad_M_max_difference_from_float64_over_max": differ, "bytes_fused": moved,
                        "GBps_whole_call": {k: round(moved / med[k] / 1e6, 1) for k in ("fused", "fused_M_detached")}})


projection(1)
projection(args.probe_views)
irradiance()
