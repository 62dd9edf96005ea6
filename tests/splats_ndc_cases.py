"""Seeded inputs for the NDC splat renderer (tests/golden/splats_ndc/sn1_*.npz, tools/gen_splats_ndc_golden.py).

Every value is fp32-representable.  A case is redrawn (next seed) until no decision quantity of any of its views lies
within DRAW_MARGIN of its kink; the tests and the generator hold the committed cases to MARGIN.  The decision quantities
(splats_ndc_oracle.decisions): each diffuse dot, each specular dot, cam_dir . n under double_sided, each channel of the
light sum before the last relu, depth - far under norm_depth_image_only.  Between them the cases take every one of these
branches on both sides (coverage), so a comparison on the GPU leaves no element out.  All positions lie within the view
frustum with |z| <= 1."""
from typing import Any, Dict

import numpy as np

import splats_ndc_oracle as oracle

MARGIN = 1e-6
DRAW_MARGIN = 1e-4
NAMES = ("1x1", "2x2", "3x5", "17x9", "16x17", "3x5_w4", "3x5_ds_quartic", "3x5_l1", "17x9_b3", "17x9_b3_shared",
         "3x5_norm_depth")
#        W   H   B  options
_SPEC = {"1x1": (1, 1, 0, {}), "2x2": (2, 2, 0, {}), "3x5": (3, 5, 0, {}), "17x9": (17, 9, 0, {}),
         "16x17": (16, 17, 0, {}), "3x5_w4": (3, 5, 0, {"w4": True}),
         "3x5_ds_quartic": (3, 5, 0, {"two_sided": True}), "3x5_l1": (3, 5, 0, {"one_light": True}),
         "17x9_b3": (17, 9, 3, {}), "17x9_b3_shared": (17, 9, 3, {"shared": True}),
         "3x5_norm_depth": (3, 5, 0, {"norm_depth": True})}
_KWARGS = {"3x5_ds_quartic": {"double_sided": True, "use_quartic": True}, "3x5_norm_depth": {"norm_depth_image_only": True}}
BRANCHES = ("diffuse", "specular", "light sum", "cam_dir . n", "depth - far")


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def _draw(name: str, seed: int) -> Dict[str, Any]:
    W, H, B, opt = _SPEC[name]
    rng = np.random.RandomState(seed)
    N, V = W * H, max(B, 1)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    cx = ((jj.reshape(-1) + 0.5) / W * 2 - 1) * 0.9                  # pixel centres in NDC, row-major, y down the rows
    cy = (1 - (ii.reshape(-1) + 0.5) / H * 2) * 0.9
    x = cx + rng.uniform(-0.05, 0.05, (V, N))
    y = cy + rng.uniform(-0.05, 0.05, (V, N))
    z = rng.uniform(-0.9, 0.9, (V, N))
    if opt.get("norm_depth"):
        z[:, 0], z[:, N - 1] = 1.0, 1.0                              # off-axis on the far plane: depth > far
        z[:, N // 2] = -0.95                                         # the unique minimum, next to the axis
    pos = np.stack((x, y, z), axis=-1)
    if opt.get("w4"):
        w = rng.uniform(0.5, 2.0, (V, N))
        pos = np.concatenate((pos * np.array([1.0, 1.0, 0.5]) * w[..., None], w[..., None]), axis=-1)
    n = np.stack((rng.uniform(-0.6, 0.6, (V, N)), rng.uniform(-0.6, 0.6, (V, N)), rng.uniform(0.5, 1.0, (V, N))), -1)
    if opt.get("two_sided"):                                         # unnormalised, facing both ways
        n *= rng.uniform(0.5, 2.0, (V, N, 1)) * np.where(rng.uniform(size=(V, N, 1)) < 0.5, -1.0, 1.0)
    else:
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
    if opt.get("w4"):
        n = np.concatenate((n, rng.uniform(-1, 1, (V, N, 1))), axis=-1)
    eye = np.stack([[0.5 + 0.25 * b, 1.0 - 0.5 * b, 6.0 + 0.125 * b, 1.0] for b in range(V)])
    if opt.get("one_light"):
        lpos = np.stack([[[1.5 - b, 2.0, 4.0, 0.5]] for b in range(V)])
        lights = {"color_idx": np.array([1]), "attenuation": np.array([[0.0, 0.0, 0.0]]),
                  "ambient": np.array([0.0625, 0.03125, 0.0625])}
        coeffs = np.array([[0.75, 0.25, 0.0], [0.5, 0.5, 1.0]])
    else:
        lpos = np.stack([[[3.0 - b, 4.0, 8.0, 1.0], [-4.0 + 0.5 * b, 1.0 + b, 1.0, 1.0]] for b in range(V)])
        lights = {"color_idx": np.array([1, 2]), "attenuation": np.array([[1.0, 0.0, 0.0], [0.625, 0.0625, 0.00390625]]),
                  "ambient": np.array([0.046875, -0.0078125, 0.0625])}   # one channel of the light sum goes negative
        coeffs = np.array([[0.75, 0.25, 5.0], [0.625, 0.375, 12.0]])
    lpos = lpos + rng.uniform(-0.25, 0.25, lpos.shape) * np.array([1.0, 1.0, 1.0, 0.0])
    shared = bool(opt.get("shared"))
    scene = {
        "camera": {"viewport": [0, 0, W, H], "fovy": 0.75, "near": 1.0, "far": 10.0,
                   "eye": _f32(eye if (B and not shared) else eye[0]), "at": _f32([0.125, -0.25, 0.0, 1.0]),
                   "up": _f32([0.25, 1.0, 0.375, 0.0])},
        "lights": dict(lights, pos=_f32(lpos if (B and not shared) else lpos[0]),
                       attenuation=_f32(lights["attenuation"]), ambient=_f32(lights["ambient"])),
        "colors": _f32([[0, 0, 0], [0.875, 0.75, 0.6875], [0.3125, 0.5, 0.875]]),
        "materials": {"albedo": _f32([[0.75, 0.625, 0.5], [0.25, 0.8125, 0.375]]), "coeffs": _f32(coeffs)},
        "objects": {"disk": {"pos": _f32(pos if B else pos[0]), "normal": _f32(n if (B and not shared) else n[0]),
                             "material_idx": (rng.uniform(size=N) < 0.4).astype(np.int64)}},
    }
    kw = dict(_KWARGS.get(name, {}))
    up_rng = np.random.RandomState(1000 + seed)
    lead = (B,) if B else ()
    if opt.get("norm_depth"):
        shapes = {"image": (H, W), "depth": (H, W), "normal": (N, 3), "pos": (N, 4)}
    else:
        shapes = {"image": (H, W, 3), "depth": (H, W), "normal": (H, W, 3), "pos": (H, W, 3)}
    upstream = {k: _f32(up_rng.uniform(-1, 1, lead + shapes[k])) for k in oracle.OUTPUTS}
    return {"name": name, "scene": scene, "kwargs": kw, "upstream": upstream}


def views(scene: Dict[str, Any]):
    B = oracle.n_views(scene)
    return [oracle.view(scene, b) for b in range(B)] if B else [scene]


def margins(scene: Dict[str, Any], **kw) -> Dict[str, Any]:
    """{branch: (smallest |value|, any below 0, any above 0)} over every view of the scene."""
    out = {}
    for sc in views(scene):
        for k, v in oracle.decisions(sc, **kw).items():
            lo, neg, pos = out.get(k, (np.inf, False, False))
            out[k] = (min(lo, float(np.abs(v).min())), neg or bool((v < 0).any()), pos or bool((v > 0).any()))
    return out


def check_special(c: Dict[str, Any]) -> None:
    """What single cases promise beyond the margins."""
    if c["name"] == "3x5_norm_depth":
        d = oracle.render(c["scene"], oracle.make_leaves(c["scene"], False), **c["kwargs"])["depth"].numpy().reshape(-1)
        assert int((d >= c["scene"]["camera"]["far"]).sum()) == 2
        s = np.sort(d)
        assert s[1] - s[0] > 1e-3 and s[-1] - s[-2] > 1e-3                # a unique minimum and a unique maximum
    if c["name"] == "3x5_ds_quartic":
        n = c["scene"]["objects"]["disk"]["normal"]
        assert np.abs(np.linalg.norm(n, axis=-1) - 1).min() > 1e-3 and (n[:, 2] > 0).any() and (n[:, 2] < 0).any()


def case(name: str) -> Dict[str, Any]:
    """{'name', 'scene', 'kwargs', 'upstream'}: the first draw (seeds 0, 1, ...) whose margins hold."""
    base = 100 * NAMES.index(name)
    for attempt in range(200):
        c = _draw(name, base + attempt)
        if all(m[0] >= DRAW_MARGIN for m in margins(c["scene"], **c["kwargs"]).values()):
            try:
                check_special(c)
            except AssertionError:
                continue
            return c
    raise RuntimeError(f"{name}: no draw satisfies the margins")


def coverage(all_margins) -> Dict[str, bool]:
    """{branch: some case takes it on both sides}, from the margins() of every case."""
    return {b: any(b in m and m[b][1] and m[b][2] for m in all_margins) for b in BRANCHES}
