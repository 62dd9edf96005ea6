"""Generate tests/golden/c1_camera_grad_*.npz and c2_camera_descent.npz: gradients with respect to the CAMERA (eye, at,
up) beside all scene leaves, from the reference torch backend running under autograd on the CPU.  Modelled on
oracle/golden_n1.py: the same scene MINUS objects.sphere, the same four upstream gradients, the same loss

    loss = sum image * g_i + sum_hit depth * g_d + sum_hit normal . g_n + sum_hit pos . g_p

The shim.  Camera leaves need the reference's in-place ray normalisation read as an out-of-place one; the reference's
code runs WITHOUT EDITS under ``oracle.ref_harness.itruediv_shim``, whose docstring has the why and the how.

Why no spheres.  With objects.sphere in the scene every camera gradient of the reference is NaN (the masked sqrt of
the sphere intersection, the same NaN that makes tests/test_hip_aux_grad.py skip grad/sphere.*).

Stored per c1 fixture: the scene, the upstream gradients, ref/{image, depth, nearest, normal, pos}, grad/<leaf> for every
scene leaf and grad/camera.{eye,at,up} (float32, as the reference computes), and grad64/camera.* from the same code run
in float64 (``oracle.ref_harness.precision``: ``diffrend.torch.utils.FloatTensor = torch.DoubleTensor``, float64 leaves).

c2_camera_descent.npz: ten Adam steps (lr 0.03) on eye and at, perturbed by (0.6, -0.4, 0.5) and (0.3, 0.2, 0), towards
the frame rendered at the fixture camera; loss = mean((image - target)^2) + 0.05 mean(where(hit, depth -
target_depth, 0)^2).  Stored: the float64 run's loss, eye and at per step, the float32 run's likewise, and ``spread`` =
the largest distance between the two runs' eye / at components after step 10 (the tests' margin is 10 x that, floored).

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by
hand -- no test reads the reference.
"""
import numpy as np
import torch

from oracle import ref_harness as R
from oracle.golden_g9_g11 import ORTHO, H, W, build_scene
from oracle.golden_io import pack_scene


def scene_without_spheres(camera=None):
    sc = build_scene()
    del sc["objects"]["sphere"]
    if camera:
        sc["camera"].update(camera)
    return sc


def ref_render(tsc, dtype, **kw):
    with R.itruediv_shim(), R.precision(dtype):
        return R.render(tsc, **kw)


def run(sc, dtype, ups, **kw):
    tsc, leaves = R.torch_scene(sc, dtype, camera_leaves=True)
    res = ref_render(tsc, dtype, **kw)
    hit = res["depth"] <= sc["camera"]["far"]
    R.masked_loss(res, ups, hit).backward()
    return res, hit, leaves


def emit(name, camera=None, **kw):
    if not R.wanted(name):
        return
    sc = scene_without_spheres(camera)
    ups = R.upstream((H, W), aux=True)                 # the g10 / g11 / n1 upstream gradients
    res, hit, leaves = run(sc, torch.float32, ups, **kw)
    res64, _, leaves64 = run(sc, torch.float64, ups, **kw)

    out = R.pack_run(sc, ups, res, leaves, kw)
    same = int((res["nearest"] == res64["nearest"]).sum())
    for k in ("camera.eye", "camera.at", "camera.up"):
        out["grad64/" + k] = leaves64[k].grad.numpy()
        g32, g64 = out["grad/" + k].astype(np.float64), out["grad64/" + k]
        print(f"{k:22s} fp32 {g32}  fp64 {g64}  diff / max {np.abs(g32 - g64).max() / np.abs(g64).max():.3g}")
    R.write(name, out)
    print("hit fraction", float(hit.float().mean()), "same winners fp32/fp64", same, "of", H * W)


def descent(dtype, sc, target, steps=10):
    start = {"eye": np.asarray(sc["camera"]["eye"], dtype=np.float64) + np.array([0.6, -0.4, 0.5, 0.0]),
             "at": np.asarray(sc["camera"]["at"], dtype=np.float64) + np.array([0.3, 0.2, 0.0, 0.0])}
    tsc, leaves = R.torch_scene(dict(sc, camera=dict(sc["camera"], **start)), dtype, camera_leaves=True)
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
    if not R.wanted(name):
        return
    sc = scene_without_spheres()
    tsc, _ = R.torch_scene(sc, torch.float64, camera_leaves=True)
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
    R.write(name, out)
    print("descent loss", l64[0], "->", l64[-1], "fp32/fp64 spread after step 10:", spread)


def main():
    emit("c1_camera_grad_phong")
    emit("c1_camera_grad_phong_ds_quartic", double_sided=True, use_quartic=True)
    emit("c1_camera_grad_ortho", camera=ORTHO)
    emit_descent("c2_camera_descent")
