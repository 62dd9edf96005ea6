#!/usr/bin/env python3
"""Generate tests/golden/c1_camera_grad_*.npz and c2_camera_descent.npz: gradients with respect to the CAMERA (eye, at,
up) beside all scene leaves, from the reference torch backend running under autograd on the CPU.  Modelled on
tools/gen_golden_aux_grad.py: the same scene MINUS objects.sphere, the same four upstream gradients, the same loss

    loss = sum image * g_i + sum_hit depth * g_d + sum_hit normal . g_n + sum_hit pos . g_p

The shim.  The reference's perspective generate_rays normalises its ray directions in place (``ray_dir /= ...``,
torch/utils.py:476), and current torch refuses to differentiate that ("modified by an inplace operation").  The
reference's code runs WITHOUT EDITS while ``torch.Tensor.__itruediv__`` is replaced by ``lambda self, other: self /
other`` for the duration of the call: Python then rebinds the name to the quotient instead of writing in place, i.e.
the statement is read as d = v / |v|.  The orthographic branch has no in-place step and gives the same result with and
without the shim.

Why no spheres.  With objects.sphere in the scene every camera gradient of the reference is NaN (the masked sqrt of
the sphere intersection, the same NaN that makes tests/test_hip_aux_grad.py skip grad/sphere.*).

Stored per c1 fixture: the scene, the upstream gradients, ref/{image, depth, nearest, normal, pos}, grad/<leaf> for every
scene leaf and grad/camera.{eye,at,up} (float32, as the reference computes), and grad64/camera.* from the same code run
in float64 (``diffrend.torch.utils.FloatTensor = torch.DoubleTensor``, float64 leaves).

c2_camera_descent.npz: ten Adam steps (lr 0.03) on eye and at, perturbed by (0.6, -0.4, 0.5) and (0.3, 0.2, 0), towards
the frame rendered at the fixture camera; loss = mean((image - target)^2) + 0.05 mean(where(hit, depth -
target_depth, 0)^2).  Stored: the float64 run's loss, eye and at per step, the float32 run's likewise, and ``spread`` =
the largest distance between the two runs' eye / at components after step 10 (the tests' margin is 10 x that, floored).

Test infrastructure; needs the reference checkout (located as oracle/gen_golden_grad_tch.py locates it) and is run by
hand -- no test reads the reference.
usage: tools/gen_golden_camera_grad.py
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

import diffrend.torch.utils as ref_utils  # noqa: E402

H, W = 36, 48


@contextlib.contextmanager
def itruediv_shim():
    """``x /= y`` on tensors rebinds x to x / y instead of dividing in place (see the module docstring)."""
    saved = torch.Tensor.__itruediv__
    torch.Tensor.__itruediv__ = lambda self, other: self / other
    try:
        yield
    finally:
        torch.Tensor.__itruediv__ = saved


@contextlib.contextmanager
def precision(dtype):
    saved = ref_utils.FloatTensor
    ref_utils.FloatTensor = torch.DoubleTensor if dtype == torch.float64 else torch.FloatTensor
    try:
        yield
    finally:
        ref_utils.FloatTensor = saved


def scene_without_spheres(camera=None):
    sc = build_scene()
    del sc["objects"]["sphere"]
    if camera:
        sc["camera"].update(camera)
    return sc


def torch_scene(sc, dtype, camera_values=None):
    """The reference's scene dict with every differentiable input a leaf of ``dtype``; returns (scene, leaves)."""
    def leaf(a):
        return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64), dtype=dtype, requires_grad=True)

    leaves = {}
    tsc = {"camera": dict(sc["camera"], proj_type=sc["camera"].get("proj_type", "perspective")),
           "tonemap": {"type": "gamma", "gamma": torch.tensor([0.8], dtype=dtype)}}
    for k in ("eye", "at", "up"):
        val = (camera_values or {}).get(k, sc["camera"][k])
        tsc["camera"][k] = leaves["camera." + k] = leaf(val)
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
    return tsc, leaves


def ref_render(tsc, dtype, **kw):
    with contextlib.redirect_stdout(io.StringIO()), itruediv_shim(), precision(dtype):
        return ref_tch.render(tsc, tiled=False, shadow=False, **kw)


def run(sc, dtype, ups, **kw):
    tsc, leaves = torch_scene(sc, dtype)
    res = ref_render(tsc, dtype, **kw)
    image, depth, normal, pos = res["image"], res["depth"], res["normal"], res["pos"]
    hit = depth <= sc["camera"]["far"]
    hit3 = hit[:, :, None].expand(H, W, 3)

    def masked(x, g, m):
        return torch.sum(torch.where(m, x * torch.tensor(g, dtype=dtype), torch.zeros_like(x)))

    loss = torch.sum(image * torch.tensor(ups["image"], dtype=dtype)) + masked(depth, ups["depth"], hit) + \
        masked(normal, ups["normal"], hit3) + masked(pos, ups["pos"], hit3)
    loss.backward()
    return res, hit, leaves


def emit(name, camera=None, **kw):
    sc = scene_without_spheres(camera)
    rng = np.random.RandomState(7)                     # the g10 / g11 / n1 upstream gradients
    ups = {"image": f32(rng.uniform(-1, 1, size=(H, W, 3))), "depth": f32(rng.uniform(-1, 1, size=(H, W)))}
    rng = np.random.RandomState(11)
    ups["normal"] = f32(rng.uniform(-1, 1, size=(H, W, 3)))
    ups["pos"] = f32(rng.uniform(-1, 1, size=(H, W, 3)))

    res, hit, leaves = run(sc, torch.float32, ups, **kw)
    res64, _, leaves64 = run(sc, torch.float64, ups, **kw)

    out = pack_scene(sc)
    for k, g in ups.items():
        out["grad_in/" + k] = g
    for k in ("image", "depth", "normal", "pos"):
        out["ref/" + k] = res[k].detach().numpy()
    out["ref/nearest"] = res["nearest"].detach().numpy().astype(np.int64)
    out["kwargs"] = np.asarray(json.dumps(kw))
    same = int((res["nearest"] == res64["nearest"]).sum())
    for k, v in leaves.items():
        out["grad/" + k] = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), dtype=np.float32)
        print(f"{k:22s} |grad| max {np.abs(out['grad/' + k]).max():.4g}")
    for k in ("camera.eye", "camera.at", "camera.up"):
        out["grad64/" + k] = leaves64[k].grad.numpy()
        g32, g64 = out["grad/" + k].astype(np.float64), out["grad64/" + k]
        print(f"{k:22s} fp32 {g32}  fp64 {g64}  diff / max {np.abs(g32 - g64).max() / np.abs(g64).max():.3g}")
    path = os.path.join(REPO, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print("hit fraction", float(hit.float().mean()), "same winners fp32/fp64", same, "of", H * W, "->", path)


def descent(dtype, sc, target, steps=10):
    start = {"eye": np.asarray(sc["camera"]["eye"], dtype=np.float64) + np.array([0.6, -0.4, 0.5, 0.0]),
             "at": np.asarray(sc["camera"]["at"], dtype=np.float64) + np.array([0.3, 0.2, 0.0, 0.0])}
    tsc, leaves = torch_scene(sc, dtype, start)
    for k, v in leaves.items():
        if k not in ("camera.eye", "camera.at"):
            v.requires_grad_(False)
    eye, at = leaves["camera.eye"], leaves["camera.at"]
    opt = torch.optim.Adam([eye, at], lr=0.03)
    t_img, t_dep = (torch.tensor(target[k], dtype=dtype) for k in ("image", "depth"))
    losses, eyes, ats = [], [], []
    for _ in range(steps):
        opt.zero_grad()
        res = ref_render(tsc, dtype)
        hit = res["depth"] <= sc["camera"]["far"]
        loss = torch.mean((res["image"] - t_img) ** 2) + \
            0.05 * torch.mean(torch.where(hit, res["depth"] - t_dep, torch.zeros_like(t_dep)) ** 2)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        eyes.append(eye.detach().numpy().astype(np.float64).copy())
        ats.append(at.detach().numpy().astype(np.float64).copy())
    return np.asarray(losses), np.asarray(eyes), np.asarray(ats), start


def emit_descent(name):
    sc = scene_without_spheres()
    tsc, _ = torch_scene(sc, torch.float64)
    with torch.no_grad():
        res = ref_render(tsc, torch.float64)
    target = {"image": res["image"].numpy(), "depth": res["depth"].numpy()}
    l64, e64, a64, start = descent(torch.float64, sc, target)
    l32, e32, a32, _ = descent(torch.float32, sc, target)
    spread = max(np.abs(e64[-1] - e32[-1]).max(), np.abs(a64[-1] - a32[-1]).max())
    out = pack_scene(sc)
    out.update({"target/image": target["image"].astype(np.float32), "target/depth": target["depth"].astype(np.float32),
                "start/eye": start["eye"], "start/at": start["at"], "loss": l64, "eye": e64, "at": a64,
                "loss32": l32, "eye32": e32, "at32": a32, "spread": np.asarray(spread), "lr": np.asarray(0.03)})
    path = os.path.join(REPO, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print("descent loss", l64[0], "->", l64[-1], "fp32/fp64 spread after step 10:", spread, "->", path)


if __name__ == "__main__":
    emit("c1_camera_grad_phong")
    emit("c1_camera_grad_phong_ds_quartic", double_sided=True, use_quartic=True)
    emit("c1_camera_grad_ortho", camera={"proj_type": "ortho", "fovy": float(np.deg2rad(100.0)), "focal_length": 4.0})
    emit_descent("c2_camera_descent")
