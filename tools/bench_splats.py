#!/usr/bin/env python3
"""Forward + backward of the splat renderer: render_splats_along_ray_batch (one HIP forward launch and one backward pass
per batch) against the fp32 torch restatement of tests/splat_oracle.py under autograd on the same GPU, one view per
call in a Python loop as the reference's GAN trainer renders its batch.  Sizes: the GAN's default (128^2, B = 4,
samples 1), B = 64, 128^2 with samples = 2, and 512^2 with B = 1.  Estimated normals, two lights.  Device events after
a warm-up; outputs are checked against the restatement at every size.  Prints one JSON line per size.
usage: tools/bench_splats.py [--steps N] [--warmup W]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import splat_oracle  # noqa: E402
from surf_renderer_amd import render_splats_along_ray_batch  # noqa: E402

DEV = "cuda:0"


def scene_of(B, S, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S), indexing="ij")
    z = np.stack([-(4.0 + 0.5 * np.sin(2 * xx + b) * np.cos(1.5 * yy)) for b in range(B)]).reshape(B, S * S)
    z = z + 0.01 * rng.standard_normal(z.shape)
    t = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV, requires_grad=g)  # noqa: E731
    return {"camera": {"viewport": [0, 0, S, S], "fovy": float(np.deg2rad(30.0)), "focal_length": 0.1,
                       "eye": t(np.stack([[0.3 * b, 1.0, 2.0, 1.0] for b in range(B)])),
                       "at": t([0, 0, 0, 1]), "up": t([0, 1, 0, 0]), "far": 100.0},
            "lights": {"pos": t(np.stack([[[2.0 + b, 2.0, 3.0, 1.0], [-2.0, 1.0, 2.0, 1.0]] for b in range(B)]), True),
                       "color_idx": torch.tensor([1, 2], device=DEV),
                       "attenuation": t([[1, 0, 0], [1, 0.05, 0.01]], True), "ambient": t([0.05, 0.05, 0.05], True)},
            "colors": t([[0, 0, 0], [0.8, 0.8, 0.8], [0.3, 0.4, 0.9]], True),
            "materials": {"albedo": t([[0.6, 0.6, 0.6]], True), "coeffs": t([[0.8, 0.2, 8.0]], True)},
            "objects": {"disk": {"pos": t(z, True), "material_idx": torch.zeros(S * S, dtype=torch.long, device=DEV)}}}


def view(scene, b):
    """View b for the torch restatement.  The camera and the index arrays go in as host values, as the reference's
    own callers hold them, so the baseline makes no device-to-host round trip for them; the differentiable arrays stay
    on the GPU."""
    host = scene.setdefault("_host", {})
    if not host:
        host["eye"] = scene["camera"]["eye"].cpu().numpy()
        host["at"] = scene["camera"]["at"].cpu().numpy()
        host["up"] = scene["camera"]["up"].cpu().numpy()
        host["color_idx"] = scene["lights"]["color_idx"].cpu().numpy()
        host["material_idx"] = scene["objects"]["disk"]["material_idx"].cpu().numpy()
    cam = dict(scene["camera"], eye=host["eye"][b], at=host["at"], up=host["up"])
    return {"camera": cam, "lights": dict(scene["lights"], color_idx=host["color_idx"]),
            "colors": scene["colors"], "materials": scene["materials"],
            "objects": {"disk": dict(scene["objects"]["disk"], material_idx=host["material_idx"])}}


def torch_step(scene, B, samples):
    loss = 0.0
    for b in range(B):
        sc = view(scene, b)
        leaves = {"disk.pos": scene["objects"]["disk"]["pos"][b], "lights.pos": scene["lights"]["pos"][b],
                  "colors": scene["colors"], "lights.attenuation": scene["lights"]["attenuation"],
                  "lights.ambient": scene["lights"]["ambient"], "materials.albedo": scene["materials"]["albedo"],
                  "materials.coeffs": scene["materials"]["coeffs"]}
        res = splat_oracle.render(sc, leaves, samples=samples)
        loss = loss + res["image"].sum() + 0.1 * res["depth"].sum()
    loss.backward()
    return loss


def hip_step(scene, samples):
    res = render_splats_along_ray_batch(scene, samples=samples)
    loss = res["image"].sum() + 0.1 * res["depth"].sum()
    loss.backward()
    return loss


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def check(scene, B, samples):
    """hip outputs and z gradients against the fp32 torch restatement (fp32 vs fp64 arithmetic: loose tolerances)."""
    z = scene["objects"]["disk"]["pos"]
    z.grad = None
    res = render_splats_along_ray_batch(scene, samples=samples)
    (res["image"].sum() + 0.1 * res["depth"].sum()).backward()
    g_hip = z.grad.clone()
    z.grad = None
    torch_step(scene, B, samples)
    g_tch = z.grad.clone()
    for b in (0, B - 1):
        want = splat_oracle.render(view(scene, b), {"disk.pos": z[b].detach(), "lights.pos": scene["lights"]["pos"][b].detach(),
                                                    "colors": scene["colors"].detach(),
                                                    "lights.attenuation": scene["lights"]["attenuation"].detach(),
                                                    "lights.ambient": scene["lights"]["ambient"].detach(),
                                                    "materials.albedo": scene["materials"]["albedo"].detach(),
                                                    "materials.coeffs": scene["materials"]["coeffs"].detach()},
                                   samples=samples)
        err = (res["image"][b].detach() - want["image"]).abs().max().item()
        assert err < 1e-3 * max(want["image"].abs().max().item(), 1.0), ("image", b, err)
    gerr = (g_hip - g_tch).abs().max().item() / max(g_tch.abs().max().item(), 1e-12)
    assert gerr < 1e-2, ("z gradient", gerr)
    return err, gerr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for B, S, K in ((4, 128, 1), (64, 128, 1), (4, 128, 2), (1, 512, 1)):
        scene = scene_of(B, S)
        err, gerr = check(scene, B, K)
        hip_ms = timed(lambda: hip_step(scene, K), args.steps, args.warmup)
        tch_ms = timed(lambda: torch_step(scene, B, K), max(args.steps // 4, 2), 1)
        print(json.dumps({"batch": B, "size": S, "samples": K, "hip_ms": round(hip_ms, 4), "torch_ms": round(tch_ms, 3),
                          "speedup": round(tch_ms / hip_ms, 1), "image_err": err, "grad_z_rel_err": gerr}), flush=True)


if __name__ == "__main__":
    main()
