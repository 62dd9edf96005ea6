"""Splat scenes that leave the everyday operating point of render_splats_along_ray (smooth z near -5, two lights with
w = 1, positive colours, shininess 5 or 12, at most 3 samples, grids of 12 x 16 and up, every optional array present) and
reach the branches of csrc/srh_splat.h that such inputs never take:

  Z = min(z, 0) and the [z < 0] gate on the z gradient (k_splat_bwd and k_splat_gather), `dl > 0` at an origin splat,
  reflect_idx on a side of length 2 (two stencil slots of one splat on the same neighbour), grid_x / grid_y with W == 1
  or H == 1, sub_shift for K = 4 .. 8, the light_vis read-modify-write over up to 64 sub-pixels, dead lanes of a partial
  wave or workgroup, splat_pow's 0 ** 0 = 1 and the cf[2] != 0 guard, the im > 0 mask of the relu over the light sum,
  lights with w != 1, pos_cols == 3, the material reduction's uniform path per wave (m0 of the wave, live lanes only),
  den_ok false at a light with attenuation (0, 0, 0), g_rn = -g_t t / rn at ray . n near -0.1.

Every builder is deterministic (fixed seeds) and returns (scene, kwargs, notes): a numpy scene dict in the format
splat_oracle.unpack produces, the keywords of the call, and what the CPU test needs to know about the case.  The base
depth field, camera, lights and materials are those of oracle/golden_p1.py.

tests/test_splat_edge_scenes_cpu.py asserts with the oracle alone that each case reaches the branch it is named for;
tests/test_hip_splats_edges.py then compares the kernels with the oracle on them, and tests/test_hip_splat_entries.py
holds every entry to its own bound (the last four cases are pinned by tests/test_splat_entry_bounds_cpu.py)."""
import functools

import numpy as np

import splat_oracle


def surface(H, W, seed):
    """Camera-space depths of a smooth bumpy surface in front of the camera (z near -5), (H W,) float32."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    z = -(5.0 + 0.6 * np.sin(2.1 * xx + 0.4) * np.cos(1.7 * yy) + 0.8 * xx * yy + 0.3 * yy)
    z += 0.02 * rng.standard_normal((H, W))
    return z.astype(np.float32).reshape(-1)


def given_normals(H, W, seed):
    rng = np.random.RandomState(seed)
    n = np.stack([rng.uniform(-0.4, 0.4, H * W), rng.uniform(-0.4, 0.4, H * W), rng.uniform(0.7, 1.2, H * W)], 1)
    return n.astype(np.float32)                     # deliberately not unit: the renderer takes them as they are


def base_scene(H, W, seed, given=False, light_vis=False):
    rng = np.random.RandomState(seed)
    scene = {
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
        "objects": {"disk": {"pos": surface(H, W, seed),
                             "material_idx": (rng.uniform(size=H * W) < 0.4).astype(np.int64)}},
    }
    if given:
        scene["objects"]["disk"]["normal"] = given_normals(H, W, seed + 100)
    if light_vis:
        L = scene["lights"]["pos"].shape[0]
        scene["objects"]["disk"]["light_vis"] = np.random.RandomState(seed + 200).uniform(0.1, 1.0, (L, H * W)) \
            .astype(np.float32)
    return scene


def _samples(K, given):
    def build():
        scene = base_scene(5, 7, seed=20 + K, given=given, light_vis=True)
        return scene, {"samples": K}, {"grid": (5, 7), "given": given}
    return build


def _grid(H, W, seed, given, K=1, **notes):
    def build():
        kw = {"samples": K} if K > 1 else {}
        return base_scene(H, W, seed, given=given), kw, dict({"grid": (H, W), "given": given}, **notes)
    return build


def _lights(L):
    """L lights on a 6 x 6 grid.  L = 1: the light has w = 0 (its position is a direction from the eye: the camera
    translation drops out).  L = 5: w = (1, 0, 0.5, 2, 1).  Every light has an attenuation of its own."""
    def build():
        scene = base_scene(6, 6, seed=30 + L, given=(L == 1))
        pos = np.array([[3.0, 4.0, 8.0, 1.0], [-4.0, 1.0, 5.0, 0.0], [2.0, -3.0, 4.0, 0.5], [-1.0, 6.0, 7.0, 2.0],
                        [0.5, 0.5, 3.0, 1.0]], np.float32)
        att = np.array([[1.0, 0.0, 0.0], [0.6, 0.04, 0.003], [0.3, 0.1, 0.0], [1.5, 0.0, 0.01], [0.8, 0.02, 0.02]],
                       np.float32)
        pick = [1] if L == 1 else list(range(L))
        scene["lights"].update(pos=pos[pick], attenuation=att[pick], color_idx=np.array([2, 1, 3, 1, 2])[:L])
        scene["colors"] = np.array([[0, 0, 0], [0.9, 0.8, 0.7], [0.3, 0.5, 0.9], [0.6, 0.2, 0.4]], np.float32)
        return scene, {}, {"grid": (6, 6), "given": L == 1, "w": [float(v) for v in pos[pick, 3]]}
    return build


def _shininess_0_1():
    """Materials with shininess 0 (rd ** 0 = 1 also at rd = 0, no gradient to rd) and 1.  The third light stands far to
    the side of the surface, so that its reflection misses the camera on part of the frame (rd clipped to 0)."""
    scene = base_scene(9, 11, seed=41)
    scene["materials"]["coeffs"] = np.array([[0.8, 0.2, 0.0], [0.6, 0.4, 1.0]], np.float32)
    scene["lights"].update(pos=np.array([[3.0, 4.0, 8.0, 1.0], [-4.0, 1.0, 5.0, 1.0], [9.0, 1.0, 1.2, 1.0]], np.float32),
                           color_idx=np.array([1, 2, 1]),
                           attenuation=np.array([[1.0, 0.0, 0.0], [0.6, 0.04, 0.003], [0.5, 0.0, 0.01]], np.float32))
    return scene, {}, {"grid": (9, 11), "given": False}


NEGATIVE_SEED = 43


def _negative_colours():
    """Colours and ambient with negative channels: the light sum is negative on part of the frame and the relu clips."""
    scene = base_scene(9, 11, seed=NEGATIVE_SEED, given=True)
    scene["colors"] = np.array([[0, 0, 0], [0.9, -0.8, 0.7], [-0.3, 0.5, -0.9]], np.float32)
    scene["lights"]["ambient"] = np.array([-0.05, 0.04, -0.02], np.float32)
    return scene, {"samples": 2}, {"grid": (9, 11), "given": True}


CLAMP_SEED = 1


def clamped_rows(H=9, W=11):
    """The seeded clamped set: 10 of the 99 splats, five at z = 0.0 and five at z = +0.75."""
    idx = np.random.RandomState(CLAMP_SEED).permutation(H * W)[:10]
    return idx[:5], idx[5:]


def _clamped(given, K):
    def build():
        scene = base_scene(9, 11, seed=44, given=given)
        zero, behind = clamped_rows()
        z = scene["objects"]["disk"]["pos"]
        z[zero] = 0.0
        z[behind] = 0.75
        kw = {"samples": K} if K > 1 else {}
        return scene, kw, {"grid": (9, 11), "given": given, "clamped": np.sort(np.concatenate([zero, behind]))}
    return build


def _zpos_cols3():
    scene = base_scene(6, 5, seed=45, given=True)
    z = scene["objects"]["disk"]["pos"]
    xy = np.random.RandomState(46).uniform(-9, 9, (z.size, 2)).astype(np.float32)
    scene["objects"]["disk"]["pos"] = np.concatenate([xy, z[:, None]], 1)       # [N, 3]: only column 2 is read
    return scene, {}, {"grid": (6, 5), "given": True}


def _quartic_k2():
    return base_scene(5, 7, seed=47), {"samples": 2, "use_quartic": True}, {"grid": (5, 7), "given": False}


def _three_materials(scene):
    scene["materials"] = {"albedo": np.array([[0.7, 0.6, 0.5], [0.3, 0.8, 0.4], [0.5, 0.5, 0.9]], np.float32),
                          "coeffs": np.array([[0.8, 0.2, 5.0], [0.6, 0.4, 12.0], [0.7, 0.3, 3.0]], np.float32)}


def _materials_by_wave():
    """2 x 64: row 0 (wave 0) is material 0, row 1 (wave 1) material 1 -- every wave takes k_splat_bwd's uniform path, to a
    row of its own (m0 is the wave's, not the workgroup's).  Material 2 is used by nobody."""
    scene = base_scene(2, 64, seed=58)
    _three_materials(scene)
    scene["objects"]["disk"]["material_idx"] = np.repeat(np.array([0, 1], np.int64), 64)
    return scene, {}, {"grid": (2, 64), "given": False}


def _materials_mixed_tail():
    """1 x 70: material 1 only in the six live lanes of the last wave, material 0 in wave 0 and at pixel 0, as which the
    58 dead lanes of the last wave run: that wave is uniform over its LIVE lanes only, with m0 = 1.  The row is 70 times
    as wide as high, so its right-hand end is seen at 88 degrees: the six normals there are turned towards the eye and a
    third light stands beside it, which gives material 1 a specular term."""
    scene = base_scene(1, 70, seed=59, given=True)
    _three_materials(scene)
    scene["objects"]["disk"]["normal"][64:] = (np.array([-0.9, 0.1, 0.3]) + np.random.RandomState(65).uniform(-0.05, 0.05, (6, 3))) \
        .astype(np.float32)
    scene["lights"].update(pos=np.array([[3.0, 4.0, 8.0, 1.0], [-4.0, 1.0, 5.0, 1.0], [1.1, 1.7, 6.0, 1.0]], np.float32),
                           color_idx=np.array([1, 2, 1]),
                           attenuation=np.array([[1.0, 0.0, 0.0], [0.6, 0.04, 0.003], [0.8, 0.02, 0.02]], np.float32))
    scene["objects"]["disk"]["material_idx"] = (np.arange(70) >= 64).astype(np.int64)
    return scene, {"samples": 2}, {"grid": (1, 70), "given": True}


def _zero_attenuation():
    """6 x 6, three lights, the second with attenuation (0, 0, 0): den = 0, so afac = 1 (den_ok false) and the light's
    attenuation gradient is exactly 0 while it still lights the frame."""
    scene = base_scene(6, 6, seed=62)
    scene["lights"].update(pos=np.array([[3.0, 4.0, 8.0, 1.0], [-4.0, 1.0, 5.0, 1.0], [2.0, -3.0, 6.0, 1.0]], np.float32),
                           color_idx=np.array([1, 2, 1]),
                           attenuation=np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.6, 0.04, 0.003]], np.float32))
    return scene, {}, {"grid": (6, 6), "given": False}


def _steep_given_k2():
    """5 x 7, K = 2, given normals tilted 52 degrees towards -x: ray . n runs from about -0.1 at the left edge to -1 at the
    right, so that g_rn = -g_t t / rn dominates the normal gradient on the left columns."""
    scene = base_scene(5, 7, seed=63, given=True)
    rng = np.random.RandomState(64)
    th = np.deg2rad(52.0)
    n = np.array([-np.sin(th), 0.0, np.cos(th)]) + rng.uniform(-0.02, 0.02, (35, 3))
    scene["objects"]["disk"]["normal"] = n.astype(np.float32)
    return scene, {"samples": 2}, {"grid": (5, 7), "given": True}


def sub_ray_dot_normal(scene, kwargs):
    """ray . n of every sub-pixel, (KH, KW), from the oracle's outputs: pos = t ray and the rays point to -z, so
    ray = -sign(pos_z) unit(pos)."""
    out = splat_oracle.render(scene, splat_oracle.make_leaves(scene, requires_grad=False), **kwargs)
    pos, n = out["pos"].numpy(), out["normal"].numpy()
    ray = pos / np.linalg.norm(pos, axis=-1, keepdims=True) * -np.sign(pos[..., 2:3])
    return np.sum(ray * n, -1)


BUILDERS = {
    "k4_given": _samples(4, True), "k4_est": _samples(4, False),
    "k8_given": _samples(8, True), "k8_est": _samples(8, False),
    "grid_2x2": _grid(2, 2, 50, False), "grid_2x3_k2": _grid(2, 3, 51, False, K=2), "grid_3x2": _grid(3, 2, 52, False),
    "row_1x9": _grid(1, 9, 53, True), "col_9x1_k3": _grid(9, 1, 54, True, K=3),
    # N = 65, 257 and 221: one live lane in the last wave (65), in the last workgroup (257), 29 of 64 (221)
    "wave_5x13": _grid(5, 13, 55, True), "block_1x257": _grid(1, 257, 56, True), "odd_17x13": _grid(17, 13, 57, False),
    "lights_1": _lights(1), "lights_5": _lights(5),
    "shininess_0_1": _shininess_0_1,
    "negative_colours": _negative_colours,
    "clamped_est": _clamped(False, 1), "clamped_given_k2": _clamped(True, 2),
    "zpos_cols3": _zpos_cols3,
    "quartic_k2": _quartic_k2,
    "materials_by_wave": _materials_by_wave, "materials_mixed_tail": _materials_mixed_tail,
    "zero_attenuation": _zero_attenuation,
    "steep_given_k2": _steep_given_k2,
}
CASES = tuple(BUILDERS)


def build(name):
    return BUILDERS[name]()


def upstream(scene, kwargs, seed=11):
    """Upstream gradients of the four outputs, uniform in [-1, 1]."""
    vp = scene["camera"]["viewport"]
    K = int(kwargs.get("samples", 1))
    KH, KW = K * (vp[3] - vp[1]), K * (vp[2] - vp[0])
    rng = np.random.RandomState(seed)
    shapes = {"image": (KH, KW, 3), "depth": (KH, KW), "normal": (KH, KW, 3), "pos": (KH, KW, 3)}
    return {k: rng.uniform(-1, 1, shapes[k]).astype(np.float32) for k in splat_oracle.OUTPUTS}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(scene, kwargs, notes, upstream, oracle outputs, oracle gradients) of a case, computed once per process; the
    arrays are shared between tests and must not be written to."""
    scene, kwargs, notes = build(name)
    up = upstream(scene, kwargs)
    out, grads = splat_oracle.gradients(scene, up, **kwargs)
    for a in list(out.values()) + list(grads.values()) + list(up.values()):
        a.setflags(write=False)
    return scene, kwargs, notes, up, out, grads


@functools.lru_cache(maxsize=None)
def terms(name):
    """(total, absolute) of splat_oracle.gradient_terms for a case under reference(name)'s upstream, computed once per
    process; the arrays must not be written to."""
    scene, kwargs, notes, up, out, grads = reference(name)
    total, absolute = splat_oracle.gradient_terms(scene, up, **kwargs)
    for a in list(total.values()) + list(absolute.values()):
        a.setflags(write=False)
    return total, absolute


def shininess_rd(scene, kwargs):
    """relu(rd) of the oracle's formula per (light, pixel), recomputed from the oracle's outputs: (L, KH, KW)."""
    out = splat_oracle.render(scene, splat_oracle.make_leaves(scene, requires_grad=False), **kwargs)
    pos, N = out["pos"].numpy(), out["normal"].numpy()
    R, eye = splat_oracle.camera_basis(scene["camera"]["eye"], scene["camera"]["at"], scene["camera"]["up"])
    R, eye = R.numpy(), eye.numpy()
    lp = np.asarray(scene["lights"]["pos"], dtype=np.float64)
    lcc = (lp[:, :3] - lp[:, 3:4] * eye[None, :]) @ R
    cdir = -pos / np.sqrt(np.sum(pos * pos + 1e-10, -1, keepdims=True))
    rd = []
    for l in range(lp.shape[0]):
        v = lcc[l] - pos
        lh = v / np.sqrt(np.sum(v * v, -1, keepdims=True))
        ldn = np.sum(lh * N, -1)
        rd.append(np.maximum(np.sum(cdir * (2 * ldn[..., None] * N - lh), -1), 0.0))
    return np.stack(rd)
