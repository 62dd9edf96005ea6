#!/usr/bin/env python3
"""Forward + backward through render(scene, shading='torch') at BASELINE config 4 (bunny.obj, 1024x1024) for losses on
different outputs: image only, image + normal + pos, normal only -- and, for comparison, the image loss through the
autograd function without the normal / pos outputs (what render() ran before they became differentiable).
Interleaved rounds; prints one JSON line per loss with the median and the spread of the per-round means.
usage: tools/bench_aux_grad.py [--steps N] [--rounds R]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from surf_renderer_amd import renderer, synthetic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    mesh = synthetic.bunny_mesh_scene(1024, 1024)
    tri = mesh["objects"]["triangle"]
    face = torch.tensor(np.asarray(tri["face"], dtype=np.float32), device="cuda:0", requires_grad=True)
    normal = torch.tensor(np.asarray(tri["normal"], dtype=np.float32), device="cuda:0", requires_grad=True)
    mesh["objects"]["triangle"] = {"face": face, "normal": normal,
                                   "material_idx": torch.tensor(np.asarray(tri["material_idx"]), device="cuda:0")}
    mesh["lights"]["pos"] = torch.tensor(np.asarray(mesh["lights"]["pos"], dtype=np.float32), device="cuda:0")
    mesh["colors"] = torch.tensor(np.asarray(mesh["colors"], dtype=np.float32), device="cuda:0")
    mesh["materials"]["albedo"] = torch.tensor(np.asarray(mesh["materials"]["albedo"], dtype=np.float32), device="cuda:0")
    g_n = torch.rand((1024, 1024, 3), device="cuda:0") - 0.5

    def image_without_aux():
        buf = renderer.flatten_scene(mesh, "cuda:0", validate=False, keep_graph=True)
        cam = renderer.camera_struct(mesh["camera"], "torch")
        inputs = [buf.tensors[k] for k in renderer._float_keys(buf, "torch")]
        image = renderer._RenderFunction.apply(buf, cam, None, "auto", renderer._Shade("torch"), (), *inputs)[0]
        image.sum().backward()

    def image():
        renderer.render(mesh, device="cuda:0", validate=False, shading="torch")["image"].sum().backward()

    def image_normal_pos():
        res = renderer.render(mesh, device="cuda:0", validate=False, shading="torch")
        (res["image"].sum() + (res["normal"] * g_n).sum() + 0.01 * res["pos"].sum()).backward()

    def normal_only():
        (renderer.render(mesh, device="cuda:0", validate=False, shading="torch")["normal"] * g_n).sum().backward()

    losses = {"image loss, no normal / pos outputs (the previous render() path)": image_without_aux,
              "image loss": image, "image + normal + pos loss": image_normal_pos, "normal loss only": normal_only}
    times = {k: [] for k in losses}
    for fn in losses.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in losses.items():
            face.grad = normal.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps)
    for name, ts in times.items():
        ms = 1e3 * np.asarray(ts)
        print(json.dumps({"config": "4: bunny.obj 1024x1024, shading='torch', forward + backward through render() "
                                    "(Python flatten included)", "loss": name,
                          "ms_per_iteration_median": float(np.median(ms)), "ms_per_round": [round(float(x), 4) for x in ms],
                          "steps_per_round": args.steps}), flush=True)


if __name__ == "__main__":
    main()
