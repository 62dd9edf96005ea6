"""What tools/bench_projection.py, bench_dense_projection.py and bench_reverse_projection.py share: the seeded workload
of the two surfel layers, the leaves and the loss, the timed windows, the comparison with the float64 composition and
the timing part of the report.  Each tool keeps its forms, its command line and its JSON keys."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from projection_cases import FOCAL, FOVY, draw_camera, jittered_grid, lift  # noqa: E402


def surfel_workload(B, S, D):
    """(rng, camera, {input: fp64 array}) of B views at S x S: a jittered depth map seen from the target cameras, about
    one surfel per cell, with rgb and a rotated image as [B, S, S, D].  RandomState(0), and the stream goes on to the
    upstream gradients (upstreams)."""
    rng = np.random.RandomState(0)
    eye, at, up = draw_camera(rng, B)
    px, py = jittered_grid(rng, B, S, S, 1.2)
    world = lift(px, py, rng.uniform(1.5, 3.0, (B, S * S)), eye, at, up, S, S)
    camera = {"eye": eye, "at": at, "up": up, "viewport": [0, 0, S, S], "fovy": float(FOVY), "focal_length": FOCAL}
    return rng, camera, {"surfels": world, "rgb": rng.uniform(0, 1, (B, S, S, D)),
                         "rotated_image": rng.uniform(0, 1, (B, S, S, D))}


def leaves(host, dev):
    return {k: torch.tensor(v.astype(np.float32), device=dev, requires_grad=True) for k, v in host.items()}


def upstreams(rng, outputs, B, S, D, dev):
    return {k: torch.tensor(rng.uniform(-1, 1, (B, S, S, D if k in ("out", "image1") else 1)).astype(np.float32), device=dev)
            for k in outputs}


def clear(x):
    for t in x.values():
        t.grad = None


def loss(res, ups):
    return sum((res[k] * ups[k]).sum() for k in ups)


def composition_fp64(project, x, ups):
    """({output: value}, {input: gradient}) of project({input: tensor}) in float64 on the same float32 inputs; not
    timed."""
    x64 = {k: t.detach().double().requires_grad_(True) for k, t in x.items()}
    res = project(x64)
    sum((res[k] * ups[k].double()).sum() for k in ups).backward()
    return {k: v.detach() for k, v in res.items()}, {k: t.grad for k, t in x64.items()}


def agreement(values, x, want_v, want_g, outputs, share=True):
    """Per value_<output> and grad_<input>: max|form - fp64| / max|fp64|, and with `share` the share of elements off by
    more than 1e-4 of the maximum."""
    got = {"value_" + k: (values[k].detach().double(), want_v[k]) for k in outputs}
    got.update({"grad_" + k: (t.grad.double(), want_g[k]) for k, t in x.items()})
    worst = {k: float(f"{float((a - b).abs().max() / b.abs().max()):.3g}") for k, (a, b) in got.items()}
    if not share:
        return worst
    return {k: {"max_err_over_max": worst[k],
                "share_off_by_1e-4_of_max": float(f"{float(((a - b).abs() > 1e-4 * b.abs().max()).double().mean()):.3g}")}
            for k, (a, b) in got.items()}


def window(fn, n):
    """ms per call over n calls, by device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n


def timed(forms, rounds, window_s):
    """(calls per window, {form: ms per call of each round}, {form: the median}): the forms alternate round by round,
    each in windows of at least `window_s` seconds of device time."""
    calls = {name: max(1, int(np.ceil(1e3 * window_s / window(fn, 3)))) for name, fn in forms.items()}
    times = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            times[name].append(window(fn, calls[name]))
    return calls, times, {name: float(np.median(ts)) for name, ts in times.items()}


def spread(ts):
    return {"ms_per_batch": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
            "spread_ms": round(max(ts) - min(ts), 4)}


def against_composition(times, med):
    """The ratio of the medians, and whether the slowest fused round beats the fastest round of the composition: faster
    by more than the spread."""
    return {"speedup_median": round(med["composition"] / med["fused"], 2),
            "fused_faster_beyond_spread": bool(max(times["fused"]) < min(times["composition"]))}
