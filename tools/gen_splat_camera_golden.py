#!/usr/bin/env python3
"""Generate tests/golden/splat_camera/sc1_*.npz: the camera gradients of the reference's OWN render_splats_along_ray and
render_splats_NDC (diffrend/torch/renderer.py:537-751, 358-474), running UNMODIFIED on the CPU under autograd with
camera.eye / at / up as leaves (oracle.ref_harness.torch_scene(camera_leaves=True)), in float64
(oracle.ref_harness.precision) and in float32, one view at a time for the batched cases, so that a shared leaf's
gradient is the sum over the views and a per-view eye's the stack.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  The along-ray cases are the base_scene family of oracle/golden_p1.py, the NDC ones the seeded cases of
tests/splats_ndc_cases.py (and one more draw of the same kind at 36 x 48).  The loss is sum(image * g_image): the camera
enters only through the lights, so the other outputs carry nothing of it.  Stored per fixture: kind, in/* (float32
inputs, camera scalars as float64), kwargs, grad_in/image, grad64/camera.{eye, at, up}, grad32/camera.{eye, at, up} and
meta: max |grad32 - grad64| per leaf with its tolerance.  Before anything is written the generator asserts the cases'
kink margins (splat_oracle.decision_margin >= 1e-6 for the along-ray family, splats_ndc_cases.MARGIN for NDC), that
every camera gradient is non-zero, and that the reference's own float32-float64 disagreement on every camera gradient is
at most a quarter of the float32 tolerance the GPU tests use, 3e-3 max(max|want|, 1e-6)."""
import contextlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402
from oracle.golden_p1 import base_scene, given_normals  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import splat_camera_oracle as oracle  # noqa: E402
import splat_oracle  # noqa: E402
import splats_ndc_cases as ndc_cases  # noqa: E402

ALONG_RAY_MARGIN = 1e-6


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def along_ray_batch(W, H, B):
    """B views of the base_scene family: per-view depths, eye and lights.pos, given normals and light_vis."""
    views = [base_scene(H, W, seed=3 + b) for b in range(B)]
    sc = views[0]
    rng = np.random.RandomState(17)
    disk = {"pos": np.stack([v["objects"]["disk"]["pos"] for v in views]),
            "normal": np.stack([given_normals(H, W, 5 + b) for b in range(B)]),
            "light_vis": _f32(rng.uniform(0.25, 1.0, (B, 2, H * W))),
            "material_idx": sc["objects"]["disk"]["material_idx"]}
    eye = _f32([sc["camera"]["eye"] + np.array([0.25 * b, -0.5 * b, 0.125 * b, 0.0]) for b in range(B)])
    lpos = _f32([sc["lights"]["pos"] + np.array([[-1.0 * b, 0.0, 0.0, 0.0], [0.5 * b, 1.0 * b, 0.0, 0.0]]) for b in range(B)])
    return dict(sc, camera=dict(sc["camera"], eye=eye), lights=dict(sc["lights"], pos=lpos), objects={"disk": disk})


def along_ray_cases():
    def light_w(sc):          # l_w = 0.5 and l_w = 0: the fourth column of the matrix gradient is g . l_w, not g
        lp = sc["lights"]["pos"].copy()
        lp[0, 3], lp[1, 3] = 0.5, 0.0
        return dict(sc, lights=dict(sc["lights"], pos=lp))
    yield "ar_2x2", base_scene(2, 2), {}
    yield "ar_3x5", base_scene(5, 3), {}
    yield "ar_3x5_lw", light_w(base_scene(5, 3)), {}
    yield "ar_12x16_s2", base_scene(16, 12), {"samples": 2}
    yield "ar_17x9_b3_quartic", along_ray_batch(17, 9, 3), {"use_quartic": True}
    yield "ar_36x48", base_scene(48, 36), {}


def ndc_cases_():
    for name in ("1x1", "2x2", "3x5_ds_quartic", "3x5_l1", "17x9_b3"):      # 3x5_l1: one light with l_w = 0.5
        c = ndc_cases.case(name)
        yield "ndc_" + name, c["scene"], c["kwargs"], c["upstream"]["image"]
    ndc_cases._SPEC["36x48"] = (36, 48, 0, {})                             # one more draw of the same kind
    for seed in range(5000, 5200):
        c = ndc_cases._draw("36x48", seed)
        if all(m[0] >= ndc_cases.DRAW_MARGIN for m in ndc_cases.margins(c["scene"]).values()):
            yield "ndc_36x48", c["scene"], c["kwargs"], c["upstream"]["image"]
            return
    raise RuntimeError("36x48: no draw satisfies the margins")


@contextlib.contextmanager
def float32_constants():
    """The renderers turn their numpy constants -- the pixel grid of render_splats_along_ray above all -- into tensors
    with tch_var_f, i.e. into float32 values in the reference's own precision.  Under precision(float64) the same call
    would keep the float64 linspace, another grid by 6e-8 of a pixel coordinate and another function by up to 7e-7 of
    a camera gradient.  While the float64 run lasts, the name tch_var_f in the renderer module rounds through float32
    first, as ref_harness.torch_scene does for the scene's values: both precisions render the same grid.  Only arrays
    that vary are rounded, i.e. the two grids: the one constant array, the rays' z = -focal_length, stays the float64
    it is in the kernels (which take focal_length as a double, where the float32 reference rounds it).  The reference's
    code runs without edits."""
    saved = R.ref_tch.tch_var_f

    def rounded(x):
        a = np.asarray(x)
        return saved(a.astype(np.float32).astype(np.float64) if a.ndim and np.ptp(a) > 0 else x)
    R.ref_tch.tch_var_f = rounded
    try:
        yield
    finally:
        R.ref_tch.tch_var_f = saved


def reference(kind, scene, kw, g_image, dtype):
    """{camera leaf: gradient} of the reference for the (possibly batched) scene in `dtype`."""
    B = oracle.n_views(kind, scene)
    runs = []
    for b in range(max(B, 1)):
        sc = oracle.view(kind, scene, b) if B else scene
        tsc, leaves = R.torch_scene(sc, dtype=dtype, camera_leaves=True)
        with R.precision(dtype), R.quiet(), float32_constants():
            if kind == "ndc":
                res = R.ref_tch.render_splats_NDC(tsc, **kw)
            else:
                res = R.ref_tch.render_splats_along_ray(tsc, normal_estimation_method="plane", **kw)
            g = g_image[b] if B else g_image
            assert res["image"].dtype == dtype and tuple(res["image"].shape) == g.shape, (res["image"].dtype, g.shape)
            torch.sum(res["image"] * torch.tensor(g, dtype=dtype)).backward()
        runs.append({k: leaves[k].grad.numpy().astype(np.float64) for k in oracle.CAMERA_LEAVES})
    if not B:
        return runs[0]
    return {k: (np.stack([r[k] for r in runs]) if np.ndim(scene["camera"][k.split(".")[1]]) == 2
                else sum(r[k] for r in runs)) for k in oracle.CAMERA_LEAVES}


def record(name, kind, scene, kw, g_image):
    B = oracle.n_views(kind, scene)
    for b in range(max(B, 1)):
        sc = oracle.view(kind, scene, b) if B else scene
        if kind == "ndc":
            m = ndc_cases.margins(sc, **kw)
            assert all(v[0] >= ndc_cases.MARGIN for v in m.values()), (name, m)
        else:
            m = splat_oracle.decision_margin(sc, **kw)
            assert all(v[0] >= ALONG_RAY_MARGIN and not len(v[1]) for v in m.values()), (name, m)
    grad64 = reference(kind, scene, kw, g_image, torch.float64)
    grad32 = reference(kind, scene, kw, g_image, torch.float32)
    out = oracle.pack(kind, scene)
    out["kwargs"] = np.asarray(json.dumps(kw))
    out["grad_in/image"] = g_image
    meta = {}
    for k in oracle.CAMERA_LEAVES:
        out["grad64/" + k], out["grad32/" + k] = grad64[k], grad32[k]
        big = float(np.abs(grad64[k]).max())
        assert big > 0, (name, k)
        err, tol = float(np.abs(grad32[k] - grad64[k]).max()), 3e-3 * max(big, 1e-6)
        meta[k] = {"err": err, "tol": tol, "max": big}
        assert err <= tol / 4, (name, k, err, tol)
        print(f"{name:22s} {k:10s} max {big:.4g}  fp32 - fp64 {err:.3g}  ({err / big:.2g} of max)")
    out["meta"] = np.asarray(json.dumps(meta, sort_keys=True))
    for k, v in out.items():
        assert v.dtype.kind not in "fc" or np.all(np.isfinite(v)), (name, k)
    R.write("sc1_" + name, out)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("splat_camera")
    for name, scene, kw in along_ray_cases():
        B = oracle.n_views("along_ray", scene)
        vp = scene["camera"]["viewport"]
        K = kw.get("samples", 1)
        shape = ((B,) if B else ()) + (K * vp[3], K * vp[2], 3)
        record(name, "along_ray", scene, kw, _f32(np.random.RandomState(29).uniform(-1, 1, shape)))
    for name, scene, kw, g_image in ndc_cases_():
        record(name, "ndc", scene, kw, g_image)
