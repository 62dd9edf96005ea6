#!/usr/bin/env python3
"""What camera_grad=True costs render_splats_along_ray_batch: 64 views at 128^2, forward + backward of an L1 loss on
`image`, with camera.eye [B, 4], at and up as leaves, against
  detached   the same call on the same tree with the camera detached (the added cost is the difference), and
  torch      the float32 torch composition of the reference's formulation with the same camera leaves
             (tests/splat_camera_oracle.py over tests/splat_oracle.py), one view per call on the same GPU.
One process, the three alternating round by round, device events around `--steps` calls, the median of `--rounds`
rounds, all of it twice.  Prints one JSON line per run.  The parent commit's detached call is not timed here: the
detached kernels are the parent's instruction for instruction (profiles/splat_camera_isa_meta.txt).
usage: tools/bench_splat_camera.py [--steps N] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import splat_camera_oracle as oracle  # noqa: E402
import splat_oracle  # noqa: E402
from bench_splats import scene_of, timed, view  # noqa: E402
from surf_renderer_amd import render_splats_along_ray_batch  # noqa: E402

B, S = 64, 128


def hip_step(scene, target, camera_grad):
    kw = {"camera_grad": True} if camera_grad else {}
    res = render_splats_along_ray_batch(scene, **kw)
    (res["image"] - target).abs().sum().backward()


def torch_step(scene, target):
    cam = scene["camera"]
    loss = 0.0
    for b in range(B):
        leaves = {"disk.pos": scene["objects"]["disk"]["pos"][b], "lights.pos": scene["lights"]["pos"][b],
                  "colors": scene["colors"], "lights.attenuation": scene["lights"]["attenuation"],
                  "lights.ambient": scene["lights"]["ambient"], "materials.albedo": scene["materials"]["albedo"],
                  "materials.coeffs": scene["materials"]["coeffs"],
                  "camera.eye": cam["eye"][b], "camera.at": cam["at"], "camera.up": cam["up"]}
        with oracle._attached(splat_oracle, leaves):
            res = splat_oracle.render(view(scene, b), leaves)
        loss = loss + (res["image"] - target[b]).abs().sum()
    loss.backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    detached = scene_of(B, S)
    leaves = scene_of(B, S)
    view(leaves, 0)                                       # bench_splats caches the host copies it needs: before the leaves
    for k in ("eye", "at", "up"):
        leaves["camera"][k].requires_grad_(True)
    target = render_splats_along_ray_batch(detached)["image"].detach() * 0.9 + 0.01
    # the two paths agree on the camera gradient before anything is timed
    hip_step(leaves, target, True)
    got = {k: leaves["camera"][k].grad.clone() for k in ("eye", "at", "up")}
    for k in got:
        leaves["camera"][k].grad = None
    torch_step(leaves, target)
    for k, g in got.items():
        w = leaves["camera"][k].grad
        assert (g - w).abs().max().item() <= 1e-2 * w.abs().max().item(), (k, (g - w).abs().max().item())
    paths = {"camera_grad": lambda: hip_step(leaves, target, True), "detached": lambda: hip_step(detached, target, False),
             "torch": lambda: torch_step(leaves, target)}
    for run in range(2):
        ms = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                ms[k].append(timed(fn, args.steps if k != "torch" else 1, 1))
        print(json.dumps({"run": run, "views": B, "size": S, "steps": args.steps, "rounds": args.rounds,
                          **{k + "_ms": round(statistics.median(v), 4) for k, v in ms.items()},
                          **{k + "_ms_range": [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}), flush=True)


if __name__ == "__main__":
    main()
