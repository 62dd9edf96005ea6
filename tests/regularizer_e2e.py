"""The end-to-end case of the regulariser tests: render_splats_along_ray_batch at 8 x 8 base pixels, samples = 2, two
views, estimated normals, then the seven regularisers, then backward to objects.disk.pos.  Shared by the GPU test and
by the CPU check of its kink condition (tests/test_regularizer_oracle_cpu.py)."""
import copy

import numpy as np
import torch

import regularizer_oracle as ro
import splat_oracle

B, H, W, K = 2, 8, 8, 2
Z_MIN, Z_MAX = 3.9, 4.3
# normal_consistency is weighted 0: between the sub-pixels of one splat u_k . n is zero by construction (see
# tests/test_regularizer_oracle_cpu.py), so |u_k . n| has no gradient to compare there.  Its VALUE is compared.
WEIGHTS = np.array([1.5, 0.7, 0.0, -1.2, 2.0e-3, 0.9, 1.1])


def scene():
    rng = np.random.RandomState(23)       # 21 and 22 leave a pos difference within 1e-5 of zero (see the CPU test)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    z = np.stack([-(4.0 + 0.5 * np.sin(2 * xx + b) * np.cos(1.5 * yy) + 0.3 * (b + 1) * xx * yy) for b in range(B)])
    z = (z + 0.02 * rng.standard_normal(z.shape)).reshape(B, H * W)
    return {
        "camera": {"viewport": [0, 0, W, H], "fovy": float(np.deg2rad(45.0)), "focal_length": 0.8,
                   "eye": np.stack([[0.5 + 0.3 * b, 1.0 - 0.2 * b, 6.0, 1.0] for b in range(B)]).astype(np.float32),
                   "at": np.array([0.1, -0.2, 0.0, 1.0]), "up": np.array([0.2, 1.0, 0.3, 0.0]), "far": 100.0},
        "lights": {"pos": np.stack([[[3.0 - b, 4.0, 8.0, 1.0], [-4.0, 1.0 + b, 5.0, 1.0]] for b in range(B)]).astype(np.float32),
                   "color_idx": np.array([1, 2]),
                   "attenuation": np.array([[1.0, 0.0, 0.0], [0.6, 0.04, 0.003]], np.float32),
                   "ambient": np.array([0.05, 0.04, 0.06], np.float32)},
        "colors": np.array([[0, 0, 0], [0.9, 0.8, 0.7], [0.3, 0.5, 0.9]], np.float32),
        "materials": {"albedo": np.array([[0.7, 0.6, 0.5], [0.3, 0.8, 0.4]], np.float32),
                      "coeffs": np.array([[0.8, 0.2, 5.0], [0.6, 0.4, 12.0]], np.float32)},
        "objects": {"disk": {"pos": z.astype(np.float32),
                             "material_idx": (rng.uniform(size=H * W) < 0.4).astype(np.int64)}},
    }


def view(sc, b):
    one = copy.deepcopy(sc)
    one["camera"]["eye"] = sc["camera"]["eye"][b]
    one["lights"]["pos"] = sc["lights"]["pos"][b]
    one["objects"]["disk"]["pos"] = sc["objects"]["disk"]["pos"][b]
    return one


def oracle_view(b, requires_grad=True):
    """(render outputs, leaves) of view b from tests/splat_oracle.py in fp64."""
    one = view(scene(), b)
    leaves = splat_oracle.make_leaves(one, requires_grad=requires_grad)
    return splat_oracle.render(one, leaves, samples=K), leaves


def expected():
    """({term: (B,)}, d loss / d objects.disk.pos (B, N)) for loss = sum_views sum_k WEIGHTS[k] term_k, in fp64."""
    values, grads = {k: [] for k in ro.TERMS}, []
    for b in range(B):
        out, leaves = oracle_view(b)
        t = ro.terms(out["pos"], out["normal"], out["image"], out["depth"], Z_MIN, Z_MAX)
        sum(float(w) * t[k] for w, k in zip(WEIGHTS, ro.TERMS)).backward()
        grads.append(leaves["disk.pos"].grad.numpy())
        for k in ro.TERMS:
            values[k].append(float(t[k].detach()))
    return {k: np.asarray(v) for k, v in values.items()}, np.stack(grads)
