"""Generate tests/golden/v1_views_grad_*.npz: the gradients of a BATCH of views, from the reference torch backend running
under autograd on the CPU as its own callers run it -- one scene dict, and per batch element ``assign disk.pos /
lights.pos / eye / at, then render()`` (diffrend/torch/GAN/gan.py:325-378), with ONE summed loss

    loss = sum_v ( sum image_v * g_i[v] + sum_hit depth_v * g_d[v] )

and one backward.  This is what ``render_views(scene, cameras, overrides=...)`` under autograd must reproduce: a leaf all
views share gets the sum over the views, a per-view leaf the gradient of its own view.

Scene: oracle/golden_g9_g11.build_scene() MINUS objects.sphere (the reference's sphere gradients are NaN,
tests/test_aux_grad_golden_cpu.py), viewport 72 x 22.  Four views with their own eye / at; the last one looks away from
the scene (eye z = 30, at z = 60) and hits nothing.  Per view: disk.pos and lights.pos = the base values plus a seeded
offset in x, y, z, and seeded upstream gradients.  Everything else is shared.  Camera tensors do not require grad, so the
reference runs without any shim.

Stored (data only): the scene, cameras/{eye,at} (4,4), view/{disk.pos,lights.pos} (4,...), grad_in/{image,depth} (4,...),
ref/{image,depth,nearest} (4,...), grad/<leaf> for shared leaves, grad/<leaf>/<v> for per-view ones, kwargs.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by
hand -- no test reads the reference.
"""
import json

import numpy as np
import torch

from oracle import ref_harness as R
from oracle.golden_g9_g11 import build_scene
from oracle.golden_io import pack_scene
from oracle.ref_harness import f32

H, W = 22, 72
EYES = f32([[0.3, 1.0, 10.0, 1.0], [2.5, -0.5, 9.0, 1.0], [-3.0, 2.0, 8.5, 1.0], [0.0, 0.5, 30.0, 1.0]])
ATS = f32([[0.0, 0.0, 0.0, 1.0], [0.5, 0.2, 0.0, 1.0], [-0.5, 0.3, -1.0, 1.0], [0.0, 0.5, 60.0, 1.0]])
PER_VIEW = ("disk.pos", "lights.pos")


def emit(name, **kw):
    if not R.wanted(name):
        return
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
    ups = R.upstream((n, H, W), rng=rng)

    tsc, shared = R.torch_scene(sc)                    # camera tensors are no leaves; eye / at are assigned per view
    for k in PER_VIEW:                                 # ... as are the per-view leaves, which replace the builder's
        del shared[k]
    own = {k: [torch.tensor(view[k][v].astype(np.float32), requires_grad=True) for v in range(n)] for k in PER_VIEW}

    loss = 0.0
    ref = {"image": [], "depth": [], "nearest": []}
    for v in range(n):
        # the reference's batch loop: assign the element's leaves and camera, then render
        tsc["objects"]["disk"]["pos"] = own["disk.pos"][v]
        tsc["lights"]["pos"] = own["lights.pos"][v]
        tsc["camera"]["eye"] = torch.tensor(EYES[v], dtype=torch.float32)
        tsc["camera"]["at"] = torch.tensor(ATS[v], dtype=torch.float32)
        res = R.render(tsc, **kw)
        hit = res["depth"] <= sc["camera"]["far"]
        loss = loss + R.masked_loss(res, {k: g[v] for k, g in ups.items()}, hit)
        for k in ref:
            ref[k].append(res[k].detach().numpy())
        print(f"view {v}: hit fraction {float(hit.float().mean()):.3f}")
    loss.backward()

    out = pack_scene(sc)
    out["cameras/eye"], out["cameras/at"] = EYES, ATS
    for k in PER_VIEW:
        out["view/" + k] = view[k].astype(np.float32)
    out["grad_in/image"] = ups["image"].astype(np.float32)
    out["grad_in/depth"] = ups["depth"].astype(np.float32)
    out["ref/image"] = np.stack(ref["image"]).astype(np.float32)
    out["ref/depth"] = np.stack(ref["depth"]).astype(np.float32)
    out["ref/nearest"] = np.stack(ref["nearest"]).astype(np.int32)
    out["kwargs"] = np.asarray(json.dumps(kw))
    R.pack_grads(out, shared)
    for k in PER_VIEW:
        for v, t in enumerate(own[k]):
            out[f"grad/{k}/{v}"] = t.grad.numpy() if t.grad is not None else np.asarray("None")
            print(f"{k}/{v:<17d} |grad| max {np.abs(t.grad.numpy()).max() if t.grad is not None else None}")
    R.write(name, out)


def main():
    emit("v1_views_grad_phong")
    emit("v1_views_grad_phong_ds_quartic", double_sided=True, use_quartic=True)
