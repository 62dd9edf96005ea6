#!/usr/bin/env python3
"""Generate tests/golden/n1_*.npz: gradients of a loss on ALL FOUR outputs of the reference torch backend -- image,
depth, normal and pos -- from the UNMODIFIED reference running under autograd on the CPU, the way
oracle/gen_golden_grad_tch.py produces the image + depth fixtures (same scene, same upstream image / depth gradients):

    loss = sum image * g_i + sum_hit depth * g_d + sum_hit normal . g_n + sum_hit pos . g_p

with the three per-pixel terms masked by torch.where(hit, ., 0): the hip backend ignores the upstream gradients of
misses (the reference differentiates object 0's intersection there).

Test infrastructure; needs the reference checkout (located as oracle/gen_golden_grad_tch.py locates it) and is run by
hand -- no test reads the reference.  Stored: the scene, the four upstream gradients, ref/{image, depth,
nearest, normal, pos} and d loss / d input for every differentiable input (float32, as the reference computes).
usage: tools/gen_golden_aux_grad.py
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from oracle.gen_golden_grad_tch import build_scene, f32, ref_tch  # noqa: E402  (puts the reference on sys.path)
from oracle.golden_io import pack_scene  # noqa: E402


def emit(name, camera=None, **kw):
    sc = build_scene()
    if camera:
        sc["camera"].update(camera)
    H, W = 36, 48
    rng = np.random.RandomState(7)                     # the g10 / g11 image and depth upstream gradients ...
    g_img = f32(rng.uniform(-1, 1, size=(H, W, 3)))
    g_dep = f32(rng.uniform(-1, 1, size=(H, W)))
    rng = np.random.RandomState(11)                    # ... and new ones for normal and pos
    g_nrm = f32(rng.uniform(-1, 1, size=(H, W, 3)))
    g_pos = f32(rng.uniform(-1, 1, size=(H, W, 3)))

    def leaf(a):
        return torch.tensor(np.asarray(a, dtype=np.float32), requires_grad=True)

    leaves = {}
    tsc = {"camera": dict(sc["camera"], proj_type=sc["camera"].get("proj_type", "perspective")),
           "tonemap": {"type": "gamma", "gamma": torch.tensor([0.8])}}
    for k in ("eye", "at", "up"):
        tsc["camera"][k] = torch.tensor(sc["camera"][k], dtype=torch.float32)
    tsc["lights"] = {"pos": leaf(sc["lights"]["pos"]), "color_idx": torch.tensor(sc["lights"]["color_idx"]),
                     "attenuation": leaf(sc["lights"]["attenuation"]), "ambient": leaf(sc["lights"]["ambient"])}
    for k in ("pos", "attenuation", "ambient"):
        leaves["lights." + k] = tsc["lights"][k]
    tsc["colors"] = leaves["colors"] = leaf(sc["colors"])
    tsc["materials"] = {"albedo": leaf(sc["materials"]["albedo"]), "coeffs": leaf(sc["materials"]["coeffs"])}
    leaves["materials.albedo"] = tsc["materials"]["albedo"]
    leaves["materials.coeffs"] = tsc["materials"]["coeffs"]
    tsc["objects"] = {}
    for kind, grp in sc["objects"].items():
        tg = {"material_idx": torch.tensor(grp["material_idx"])}
        for nm, val in grp.items():
            if nm != "material_idx":
                tg[nm] = leaves[f"{kind}.{nm}"] = leaf(val)
        tsc["objects"][kind] = tg

    with contextlib.redirect_stdout(io.StringIO()):
        res = ref_tch.render(tsc, tiled=False, shadow=False, **kw)
    image, depth, normal, pos = res["image"], res["depth"], res["normal"], res["pos"]
    hit = depth <= sc["camera"]["far"]
    hit3 = hit[:, :, None].expand(H, W, 3)

    def masked(x, g, m):
        return torch.sum(torch.where(m, x * torch.tensor(g, dtype=torch.float32), torch.zeros_like(x)))

    loss = torch.sum(image * torch.tensor(g_img, dtype=torch.float32)) + masked(depth, g_dep, hit) + \
        masked(normal, g_nrm, hit3) + masked(pos, g_pos, hit3)
    loss.backward()

    out = pack_scene(sc)
    out["grad_in/image"] = g_img
    out["grad_in/depth"] = g_dep
    out["grad_in/normal"] = g_nrm
    out["grad_in/pos"] = g_pos
    out["ref/image"] = image.detach().numpy()
    out["ref/depth"] = depth.detach().numpy()
    out["ref/normal"] = normal.detach().numpy()
    out["ref/pos"] = pos.detach().numpy()
    out["ref/nearest"] = res["nearest"].detach().numpy().astype(np.int64)
    out["kwargs"] = np.asarray(json.dumps(kw))
    for k, v in leaves.items():
        out["grad/" + k] = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), dtype=np.float32)
        print(f"{k:22s} |grad| max {np.abs(out['grad/' + k]).max():.4g}")
    path = os.path.join(REPO, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print("hit fraction", float(hit.float().mean()), "->", path)


if __name__ == "__main__":
    emit("n1_aux_grad_phong")
    emit("n1_aux_grad_phong_ds_quartic", double_sided=True, use_quartic=True)
    # orthographic: per-pixel ray origins on the image plane (camera as in g11_torch_autograd_ortho)
    emit("n1_aux_grad_ortho", camera={"proj_type": "ortho", "fovy": float(np.deg2rad(100.0)), "focal_length": 4.0})
