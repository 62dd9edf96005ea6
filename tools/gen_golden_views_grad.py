#!/usr/bin/env python3
"""Generate tests/golden/v1_views_grad_*.npz: the gradients of a BATCH of views, from the reference torch backend running
under autograd on the CPU as its own callers run it -- one scene dict, and per batch element ``assign disk.pos /
lights.pos / eye / at, then render()`` (diffrend/torch/GAN/gan.py:325-378), with ONE summed loss

    loss = sum_v ( sum image_v * g_i[v] + sum_hit depth_v * g_d[v] )

and one backward.  This is what ``render_views(scene, cameras, overrides=...)`` under autograd must reproduce: a leaf all
views share gets the sum over the views, a per-view leaf the gradient of its own view.

Scene: oracle/gen_golden_grad_tch.build_scene() MINUS objects.sphere (the reference's sphere gradients are NaN,
tests/test_aux_grad_golden_cpu.py), viewport 72 x 22.  Four views with their own eye / at; the last one looks away from
the scene (eye z = 30, at z = 60) and hits nothing.  Per view: disk.pos and lights.pos = the base values plus a seeded
offset in x, y, z, and seeded upstream gradients.  Everything else is shared.  Camera tensors do not require grad, so the
reference runs without any shim.

Stored (data only): the scene, cameras/{eye,at} (4,4), view/{disk.pos,lights.pos} (4,...), grad_in/{image,depth} (4,...),
ref/{image,depth,nearest} (4,...), grad/<leaf> for shared leaves, grad/<leaf>/<v> for per-view ones, kwargs.

Test infrastructure; needs the reference checkout (located as oracle/gen_golden_grad_tch.py locates it) and is run by
hand -- no test reads the reference.
usage: tools/gen_golden_views_grad.py
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

H, W = 22, 72
EYES = f32([[0.3, 1.0, 10.0, 1.0], [2.5, -0.5, 9.0, 1.0], [-3.0, 2.0, 8.5, 1.0], [0.0, 0.5, 30.0, 1.0]])
ATS = f32([[0.0, 0.0, 0.0, 1.0], [0.5, 0.2, 0.0, 1.0], [-0.5, 0.3, -1.0, 1.0], [0.0, 0.5, 60.0, 1.0]])
PER_VIEW = ("disk.pos", "lights.pos")


def emit(name, **kw):
    sc = build_scene()
    del sc["objects"]["sphere"]
    sc["camera"]["viewport"] = [0, 0, W, H]
    n = len(EYES)
    rng = np.random.RandomState(23)
    offs = {"disk.pos": f32(rng.uniform(-0.4, 0.4, size=(n,) + np.shape(sc["objects"]["disk"]["pos"]))),
            "lights.pos": f32(rng.uniform(-0.8, 0.8, size=(n,) + np.shape(sc["lights"]["pos"])))}
    for o in offs.values():
        o[..., 3] = 0.0
    view = {"disk.pos": f32(np.asarray(sc["objects"]["disk"]["pos"])[None] + offs["disk.pos"]),
            "lights.pos": f32(np.asarray(sc["lights"]["pos"])[None] + offs["lights.pos"])}
    g_img = f32(rng.uniform(-1, 1, size=(n, H, W, 3)))
    g_dep = f32(rng.uniform(-1, 1, size=(n, H, W)))

    def leaf(a):
        return torch.tensor(np.asarray(a, dtype=np.float32), requires_grad=True)

    shared = {}
    tsc = {"camera": dict(sc["camera"], proj_type="perspective"),
           "tonemap": {"type": "gamma", "gamma": torch.tensor([0.8])}}
    tsc["camera"]["up"] = torch.tensor(sc["camera"]["up"], dtype=torch.float32)
    tsc["lights"] = {"pos": None, "color_idx": torch.tensor(sc["lights"]["color_idx"]),
                     "attenuation": leaf(sc["lights"]["attenuation"]), "ambient": leaf(sc["lights"]["ambient"])}
    shared["lights.attenuation"] = tsc["lights"]["attenuation"]
    shared["lights.ambient"] = tsc["lights"]["ambient"]
    tsc["colors"] = shared["colors"] = leaf(sc["colors"])
    tsc["materials"] = {"albedo": leaf(sc["materials"]["albedo"]), "coeffs": leaf(sc["materials"]["coeffs"])}
    shared["materials.albedo"] = tsc["materials"]["albedo"]
    shared["materials.coeffs"] = tsc["materials"]["coeffs"]
    tsc["objects"] = {}
    for kind, grp in sc["objects"].items():
        tg = {"material_idx": torch.tensor(grp["material_idx"])}
        for nm, val in grp.items():
            if nm != "material_idx" and f"{kind}.{nm}" not in PER_VIEW:
                tg[nm] = shared[f"{kind}.{nm}"] = leaf(val)
        tsc["objects"][kind] = tg
    own = {k: [leaf(view[k][v]) for v in range(n)] for k in PER_VIEW}

    loss = 0.0
    ref = {"image": [], "depth": [], "nearest": []}
    for v in range(n):
        # the reference's batch loop: assign the element's leaves and camera, then render
        tsc["objects"]["disk"]["pos"] = own["disk.pos"][v]
        tsc["lights"]["pos"] = own["lights.pos"][v]
        tsc["camera"]["eye"] = torch.tensor(EYES[v], dtype=torch.float32)
        tsc["camera"]["at"] = torch.tensor(ATS[v], dtype=torch.float32)
        with contextlib.redirect_stdout(io.StringIO()):
            res = ref_tch.render(tsc, tiled=False, shadow=False, **kw)
        image, depth = res["image"], res["depth"]
        hit = depth <= sc["camera"]["far"]
        loss = loss + torch.sum(image * torch.tensor(g_img[v], dtype=torch.float32)) + \
            torch.sum(torch.where(hit, depth * torch.tensor(g_dep[v], dtype=torch.float32), torch.zeros_like(depth)))
        ref["image"].append(image.detach().numpy())
        ref["depth"].append(depth.detach().numpy())
        ref["nearest"].append(res["nearest"].detach().numpy().astype(np.int64))
        print(f"view {v}: hit fraction {float(hit.float().mean()):.3f}")
    loss.backward()

    out = pack_scene(sc)
    out["cameras/eye"], out["cameras/at"] = EYES, ATS
    for k in PER_VIEW:
        out["view/" + k] = view[k].astype(np.float32)
    out["grad_in/image"] = g_img.astype(np.float32)
    out["grad_in/depth"] = g_dep.astype(np.float32)
    out["ref/image"] = np.stack(ref["image"]).astype(np.float32)
    out["ref/depth"] = np.stack(ref["depth"]).astype(np.float32)
    out["ref/nearest"] = np.stack(ref["nearest"]).astype(np.int32)
    out["kwargs"] = np.asarray(json.dumps(kw))
    for k, t in shared.items():
        out["grad/" + k] = t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape), dtype=np.float32)
        print(f"{k:22s} |grad| max {np.abs(out['grad/' + k]).max():.4g}")
    for k in PER_VIEW:
        for v, t in enumerate(own[k]):
            out[f"grad/{k}/{v}"] = t.grad.numpy() if t.grad is not None else np.asarray("None")
            print(f"{k}/{v:<17d} |grad| max {np.abs(t.grad.numpy()).max() if t.grad is not None else None}")
    path = os.path.join(REPO, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    emit("v1_views_grad_phong")
    emit("v1_views_grad_phong_ds_quartic", double_sided=True, use_quartic=True)
