"""Generate tests/golden/p1_*.npz: forward outputs and gradients of the reference's splat renderer,
render_splats_along_ray (diffrend/torch/renderer.py:537-751), running UNMODIFIED on the CPU under autograd:

    loss = sum image * g_i + sum depth * g_d + sum normal * g_n + sum pos * g_p

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by
hand -- no test reads the reference.  Stored (tests/splat_oracle.pack / unpack): the inputs, the four upstream
gradients, ref/{image, depth, normal, pos} and d loss / d leaf for every differentiable input (float32, as the
reference computes).
"""
import json
import os
import sys

import numpy as np
import torch

from oracle import ref_harness as R

sys.path.insert(0, os.path.join(R.REPO, "tests"))
from splat_oracle import pack  # noqa: E402


def surface(H, W, seed):
    """Camera-space depths of a smooth bumpy surface in front of the camera (z < 0)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    z = -(5.0 + 0.6 * np.sin(2.1 * xx + 0.4) * np.cos(1.7 * yy) + 0.8 * xx * yy + 0.3 * yy)
    z += 0.02 * rng.standard_normal((H, W))
    return z.astype(np.float32)


def base_scene(H, W, seed=3):
    rng = np.random.RandomState(seed)
    return {
        "camera": {"viewport": [0, 0, W, H], "fovy": float(np.deg2rad(45.0)), "focal_length": 0.8,
                   "eye": np.array([0.8, 1.5, 6.0, 1.0], np.float32), "at": np.array([0.1, -0.2, 0.0, 1.0], np.float32),
                   "up": np.array([0.2, 1.0, 0.3, 0.0], np.float32), "far": 100.0},
        "lights": {"pos": np.array([[3.0, 4.0, 8.0, 1.0], [-4.0, 1.0, 5.0, 1.0]], np.float32),
                   "color_idx": np.array([1, 2]),
                   "attenuation": np.array([[1.0, 0.0, 0.0], [0.6, 0.04, 0.003]], np.float32),
                   "ambient": np.array([0.05, 0.04, 0.06], np.float32)},
        "colors": np.array([[0, 0, 0], [0.9, 0.8, 0.7], [0.3, 0.5, 0.9]], np.float32),
        "materials": {"albedo": np.array([[0.7, 0.6, 0.5], [0.3, 0.8, 0.4]], np.float32),
                      "coeffs": np.array([[0.8, 0.2, 5.0], [0.6, 0.4, 12.0]], np.float32)},
        "objects": {"disk": {"pos": surface(H, W, seed).reshape(-1),
                             "material_idx": (rng.uniform(size=H * W) < 0.4).astype(np.int64)}},
    }


def emit(name, scene, **kw):
    if not R.wanted(name):
        return
    tsc, leaves = R.torch_scene(scene)                 # the splat scene has the same leaves; its disk.pos is the z field
    with R.quiet():
        res = R.ref_tch.render_splats_along_ray(tsc, normal_estimation_method="plane", **kw)
    rng = np.random.RandomState(11)
    g = {k: rng.uniform(-1, 1, size=tuple(res[k].shape)).astype(np.float32) for k in ("image", "depth", "normal", "pos")}
    loss = sum(torch.sum(res[k] * torch.tensor(g[k])) for k in g)
    loss.backward()

    out = pack(scene)
    for k in g:
        out["grad_in/" + k] = g[k]
        out["ref/" + k] = res[k].detach().numpy()
    out["kwargs"] = np.asarray(json.dumps(kw))
    R.pack_grads(out, leaves)
    R.write(name, out)


def given_normals(H, W, seed):
    rng = np.random.RandomState(seed)
    n = np.stack([rng.uniform(-0.4, 0.4, H * W), rng.uniform(-0.4, 0.4, H * W), rng.uniform(0.7, 1.2, H * W)], 1)
    return n.astype(np.float32)                     # deliberately not unit: the renderer takes them as they are


def main():
    H, W = 36, 48
    emit("p1_estimated_36x48", base_scene(H, W))

    sc = base_scene(30, 40, seed=5)
    z = sc["objects"]["disk"]["pos"]
    sc["objects"]["disk"]["pos"] = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)       # [N, 3]: column 2
    sc["objects"]["disk"]["normal"] = given_normals(30, 40, 6)
    sc["objects"]["disk"]["light_vis"] = np.random.RandomState(7).uniform(0, 1, (2, 30 * 40)).astype(np.float32)
    emit("p1_given_normals_vis_30x40", sc)

    emit("p1_samples2_20x28", base_scene(20, 28, seed=8), samples=2)
    sc = base_scene(12, 16, seed=9)
    sc["objects"]["disk"]["light_vis"] = (np.random.RandomState(2).uniform(size=(2, 12 * 16)) < 0.8).astype(np.float32)
    emit("p1_samples3_12x16", sc, samples=3)
    emit("p1_quartic_36x48", base_scene(H, W, seed=10), use_quartic=True)

    sc = base_scene(H, W, seed=12)
    z = sc["objects"]["disk"]["pos"].reshape(H, W)
    z[10:18, 20:30] = -4.5                                   # a flat patch facing the camera
    z[2, 3] = z[30, 40] = 0.25                               # splats behind the camera plane: Z = 0, no z gradient
    z[25, 7] = 0.0
    emit("p1_zpos_flat_36x48", sc)

    emit("p1_norm_depth_36x48", base_scene(H, W, seed=13), norm_depth_image_only=True)
