"""Generate tests/golden/s1*.npz: the reference torch backend's render(scene, shadow=True), forward, CPU, float32.

Test infrastructure; runs only where the reference checkout is present (oracle/ref_harness.py).  The reference source
is run unmodified, but its shadow branch converts a mask with `.type(torch.cuda.FloatTensor)` (torch/renderer.py:311), which raises on a machine without a
GPU.  This module therefore aliases `torch.cuda.FloatTensor` to `torch.FloatTensor` *in its own process* around the
call -- the only deviation, and one that changes where the tensor lives, not a value in it.  Stored: the scene, the
keyword arguments, image / depth / nearest (the reference does not return the visibility itself; the image carries it:
a light that the reference finds blocked contributes nothing to the pixel).
"""
import json

import numpy as np
import torch

from oracle import ref_harness as R
from oracle.golden_io import pack_scene
from oracle.ref_harness import f32
from surf_renderer_amd import synthetic


def emit(name, sc, **kw):
    if not R.wanted(name):
        return
    lit = R.render(R.torch_scene(sc, requires_grad=False)[0], **kw)
    saved, torch.cuda.FloatTensor = torch.cuda.FloatTensor, torch.FloatTensor          # see the docstring
    try:
        res = R.render(R.torch_scene(sc, requires_grad=False)[0], shadow=True, **kw)
    finally:
        torch.cuda.FloatTensor = saved
    flat = pack_scene(sc)
    flat["out/image"] = res["image"].numpy()
    flat["out/depth"] = res["depth"].numpy()
    flat["out/nearest"] = res["nearest"].numpy().astype(np.int64)
    flat["kwargs"] = np.asarray(json.dumps(kw))
    R.write(name, flat)
    changed = (np.abs(res["image"].numpy() - lit["image"].numpy()).max(axis=-1) > 1e-6).mean()
    print(f"{name:34s} {flat['out/depth'].shape} pixels darkened by a shadow {changed:6.1%}")


def main():
    # s1a: the mixed scene of t2 (all four primitive types; spheres and triangles shadow the planes)
    a = synthetic.demo_scene(64, 48, with_planes=True)
    a["camera"]["near"] = 0.5
    a["lights"]["attenuation"] = f32([[1, 0, 0], [0.2, 0.05, 0], [1, 0, 0.001], [0.7, 0.02, 0.0005]])
    a["lights"]["ambient"] = f32([0.02, 0.015, 0.01])
    a["materials"]["coeffs"] = f32([[1, 0, 0], [0.8, 0.2, 4], [0.6, 0.4, 16], [0.9, 0.1, 2], [0.5, 0.5, 8], [0.7, 0.3, 32]])
    emit("s1a_mixed_shadow_64x48", a)
    emit("s1a_mixed_shadow_64x48_ds", a, double_sided=True)
    # s1b: a disc cloud shadowing itself
    b = synthetic.disk_cloud_scene(600, 64, 64, radius=0.12, seed=23)
    b["lights"]["attenuation"] = f32([[1, 0, 0]] * 4)
    b["lights"]["ambient"] = f32([0.01, 0.01, 0.01])
    b["materials"]["coeffs"] = f32([[0.9, 0.1, 3.0]])
    emit("s1b_disk_cloud_shadow_64x64_ds", b, double_sided=True)
