#!/usr/bin/env python3
"""What camera gradients cost at BASELINE config 4 (bunny.obj, 1024 x 1024, shading='torch') through ResidentScene:
forward + backward with (a) the scene's leaves only and (b) the same plus the camera's eye / at / up, alternating in one
process, timed with device events.  Prints one JSON line per case with the median and the spread of the per-round means.

--kernels runs ONE iteration set of (b) and nothing else, for a kernel trace taken from outside:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_camera_grad.py --kernels
(the camera variant of k_render_bwd_tch and k_camera_finish are then in DIR's kernel statistics).
--scene-only times (a) alone (the form that also runs on a commit without camera gradients, for the run-to-run spread).
usage: tools/time_camera_grad.py [--steps N] [--rounds R] [--kernels | --scene-only]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from surf_renderer_amd import ResidentScene, synthetic

DEV = "cuda:0"


def scene(camera_leaves: bool):
    mesh = synthetic.bunny_mesh_scene(1024, 1024)
    tri = mesh["objects"]["triangle"]
    face = torch.tensor(np.asarray(tri["face"], dtype=np.float32), device=DEV, requires_grad=True)
    normal = torch.tensor(np.asarray(tri["normal"], dtype=np.float32), device=DEV, requires_grad=True)
    mesh["objects"]["triangle"] = dict(tri, face=face, normal=normal)
    leaves = [face, normal]
    if camera_leaves:
        cam = {k: torch.tensor(mesh["camera"][k], dtype=torch.float32, device=DEV, requires_grad=True)
               for k in ("eye", "at", "up")}
        mesh["camera"] = dict(mesh["camera"], **cam)
        leaves += list(cam.values())
    return ResidentScene(mesh, device=DEV, shading="torch", validate=False), leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--scene-only", action="store_true")
    args = ap.parse_args()
    target = torch.rand((1024, 1024, 3), device=DEV)
    cases = {} if args.scene_only else {"b: scene leaves + camera eye / at / up": scene(True)}
    if not args.kernels:
        cases = {"a: scene leaves only": scene(False), **cases}

    def step(rs, leaves):
        for t in leaves:
            t.grad = None
        ((rs.render()["image"] - target) ** 2).sum().backward()

    for rs, leaves in cases.values():
        for _ in range(10):
            step(rs, leaves)
    torch.cuda.synchronize()
    if args.kernels:
        for rs, leaves in cases.values():
            for _ in range(args.steps):
                step(rs, leaves)
        torch.cuda.synchronize()
        return
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for name, (rs, leaves) in cases.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.steps):
                step(rs, leaves)
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / args.steps)
    for name, ms in times.items():
        print(json.dumps({"config": "4: bunny.obj 1024x1024, shading='torch', ResidentScene forward + backward",
                          "case": name, "ms_per_iteration_median": round(float(np.median(ms)), 4),
                          "ms_per_round": [round(float(x), 4) for x in ms], "steps_per_round": args.steps,
                          "iterations": args.steps * args.rounds}), flush=True)


if __name__ == "__main__":
    main()
