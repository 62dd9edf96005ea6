"""Seeded inputs for the re-projection tests (tests/test_hip_projection.py on the GPU, tests/
test_projection_oracle_cpu.py here) and for tools/gen_projection_golden.py, which records the reference on them.

A case is a dict: `surfels` [B, N, 3], `rgb` and (where the case merges) `rotated_image` as [B, H, W, D] or [B, N, D],
all fp32-representable; `camera` (eye / at / up [B, 3] or [B, 4], viewport, fovy, focal_length); `blur_size`; `flags`
(the call's keyword switches); `upstream` {output: fp32 gradient [B, H, W, .]}.  Names are H x W, the smallest shapes at
which each piece can go wrong:
    2x2          D = 1; blur_size 3.0: the half-width 3 exceeds the frame, padding dominates
    3x5          D = 4, odd and non-square; blur_size 1.2: half-width 1 from H (3 from W, which would be wrong)
    12x16        B = 2, two cameras; blur_size 0.5 (half-width 3), rotated image, compute_new_depth; the second view
                 is squeezed to half its width, so its mask passes 1 in the middle
    17x9         B = 3, [B, N, D] layout, homogeneous camera vectors; surfels off every edge, a few behind the camera
    cluster_8x8  all 64 surfels in one cell, every other cell empty: the longest list, and pixels whose mask is 0
    36x48        1728 surfels, default blur_size (half-width 2): the lists cross workgroup boundaries
VARIANTS are the flag variants of 12x16, one per switch.

Surfels are drawn in the target camera's frame -- a pixel coordinate near each pixel's centre and a depth -- and lifted
to world coordinates, so the cases cover the frame the way a re-projected depth map does.

Kink condition (projection_oracle.decision_margin >= 1, in fp64, under every flag set the case is used with): every
component of `pixel coordinate - 0.5` at least 1e-4 from an integer, |Z| >= 1e-3, every blurred mask exactly 0 or at
least 1e-4 from 0 and, with a rotated image, at least 1e-4 from 1.  A draw that violates it is redrawn from the next
seed; tests/test_projection_oracle_cpu.py asserts it for every case, so no comparison leaves an element out."""
import functools

import numpy as np

import projection_oracle as po

NAMES = ("2x2", "3x5", "12x16", "17x9", "cluster_8x8", "36x48")
_SPEC = {  # B, H, W, D, blur_size, rotated, flat layout, jitter (pixels)
    "2x2": (1, 2, 2, 1, 3.0, False, False, 0.9),
    "3x5": (1, 3, 5, 4, 1.2, False, False, 1.2),
    "12x16": (2, 12, 16, 3, 0.5, True, False, 1.2),
    "17x9": (3, 17, 9, 2, 0.4, False, True, 3.0),
    "cluster_8x8": (1, 8, 8, 3, 0.7, False, False, 0.0),
    "36x48": (1, 36, 48, 3, 0.15, False, False, 1.2),
}
_FLAGS = {"12x16": {"compute_new_depth": True}, "17x9": {"compute_new_depth": True}}
VARIANTS = {"no_depth": {"use_depth": False}, "no_center_dist": {"use_center_dist": False},
            "raw_rotated": {"blur_rotated_image": False}, "detach_mask": {"detach_mask": True},
            "detach_mask2": {"detach_mask2": True}, "detach_depth_merge": {"detach_depth_merge": True}}
VARIANT_OF = "12x16"
FOVY, FOCAL = np.deg2rad(40.0), 0.5


def f32(a):
    return np.asarray(a, dtype=np.float32)


def draw_camera(rng, B, side=0.0, spread=0.5):
    """eye, at, up [B, 3] fp32 of B cameras above the origin, `side` to its right."""
    eye = f32(rng.uniform(-spread, spread, (B, 3)) + [side, 0.5, 4.0])
    at = f32(rng.uniform(-0.3, 0.3, (B, 3)) + [0.25 * side, 0.0, 0.0])
    up = f32(rng.uniform(-0.2, 0.2, (B, 3)) + [0.0, 1.0, 0.0])
    return eye, at, up


def pixel_centres(B, H, W):
    """(px, py) [B, H W]: the pixel coordinates of the frame's pixel centres, row by row."""
    gy, gx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    return np.broadcast_to(gx.reshape(1, H * W), (B, H * W)), np.broadcast_to(gy.reshape(1, H * W), (B, H * W))


def jittered_grid(rng, B, H, W, jitter):
    """(px, py) [B, H W]: a pixel coordinate within `jitter` pixels of each pixel's centre (px is drawn first)."""
    cx, cy = pixel_centres(B, H, W)
    return cx + rng.uniform(-jitter, jitter, (B, H * W)), cy + rng.uniform(-jitter, jitter, (B, H * W))


def rays(px, py, eye, at, up, W, H, fovy, focal):
    """Per pixel coordinate (px, py) [B, N] the direction r [B, N, 3] with world point = eye - depth * r.  Along an axis
    of one pixel the coordinate carries nothing: the ray goes through the centre."""
    h = np.tan(fovy / 2) * 2 * focal
    w = h * W / H
    a = (px - W / 2.0) / (-(W - 1) / w) / focal if W > 1 else np.zeros_like(px)
    b = (py - H / 2.0) / ((H - 1) / h) / focal if H > 1 else np.zeros_like(py)
    zc = eye.astype(np.float64) - at
    zc /= np.linalg.norm(zc, axis=-1, keepdims=True)
    xc = np.cross(up.astype(np.float64), zc)
    xc /= np.linalg.norm(xc, axis=-1, keepdims=True)
    return a[..., None] * xc[:, None] + b[..., None] * np.cross(zc, xc)[:, None] + zc[:, None]


def lift(px, py, z, eye, at, up, W, H, fovy=FOVY, focal=FOCAL):
    """World positions [B, N, 3] (fp64) of the points that the cameras (eye, at, up: [B, 3]) see at pixel coordinates
    (px, py) and depth z, each [B, N]."""
    return eye[:, None].astype(np.float64) - z[..., None] * rays(px, py, eye, at, up, W, H, fovy, focal)


def _draw(name, seed):
    B, H, W, D, blur_size, rotated, flat, jitter = _SPEC[name]
    rng = np.random.RandomState(seed)
    N = H * W
    eye, at, up = draw_camera(rng, B)
    px, py = jittered_grid(rng, B, H, W, jitter)           # the pixel coordinate and the depth each surfel is aimed at
    z = rng.uniform(1.5, 3.0, (B, N))
    if name == "cluster_8x8":
        px, py = 3.5 + rng.uniform(0.15, 0.85, (B, N)), 3.5 + rng.uniform(0.15, 0.85, (B, N))     # cell (3, 3)
    if name == "12x16":
        # the second view squeezed to half its width about the centre: most cells are occupied there, so the mask passes 1
        # (the merge's other branch) in the middle
        px[1] = W / 2.0 + 0.5 * (px[1] - W / 2.0)
    if name == "17x9":
        z[:, rng.permutation(N)[:4]] = -rng.uniform(0.5, 1.5, (B, 4))                             # behind the camera
    world = lift(px, py, z, eye, at, up, W, H)
    shape = (B, N, D) if flat else (B, H, W, D)
    hom = name == "17x9"
    case = {"surfels": f32(world), "rgb": f32(rng.uniform(0, 1, shape)),
            "rotated_image": f32(rng.uniform(0, 1, shape)) if rotated else None,
            "camera": {"eye": np.concatenate((eye, np.ones((B, 1), np.float32)), -1) if hom else eye,
                       "at": np.concatenate((at, np.ones((B, 1), np.float32)), -1) if hom else at,
                       "up": np.concatenate((up, np.zeros((B, 1), np.float32)), -1) if hom else up,
                       "viewport": [0, 0, W, H], "fovy": float(FOVY), "focal_length": FOCAL},
            "blur_size": blur_size, "flags": dict(_FLAGS.get(name, {})), "shape": (B, H, W, D)}
    case["upstream"] = {k: f32(rng.uniform(-1, 1, (B, H, W, D if k in ("out", "image1") else 1))) for k in po.OUTPUTS
                        if k != "depth" or case["flags"].get("compute_new_depth")}
    return case


def flag_sets(name):
    """Every flag set a case is used with: its own, and for 12x16 each variant's."""
    base = _FLAGS.get(name, {})
    return [base] + ([dict(base, **v) for v in VARIANTS.values()] if name == VARIANT_OF else [])


def margin(c, name):
    return min(po.decision_margin(c["surfels"], c["rgb"], c["camera"], c["rotated_image"], c["blur_size"], **f)
               for f in flag_sets(name))


@functools.lru_cache(maxsize=None)
def case(name, variant=None):
    if variant is not None:
        c = dict(case(VARIANT_OF))
        c["flags"] = dict(c["flags"], **VARIANTS[variant])
        return c
    for seed in range(1000 * NAMES.index(name), 1000 * NAMES.index(name) + 50):
        c = _draw(name, seed)
        if margin(c, name) >= 1.0:
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} is clear of every kink")


def inputs(c):
    return {k: c[k] for k in po.INPUTS}


ALL = [(n, None) for n in NAMES] + [(VARIANT_OF, v) for v in VARIANTS]


def tag(name, variant=None):
    return name if variant is None else f"{name}_{variant}"


@functools.lru_cache(maxsize=None)
def expected(name, variant=None, wrt=po.INPUTS, only=None):
    """(values {output: [B, H, W, .]}, gradients {input: like the input}) from the fp64 oracle, computed once; `only`
    restricts the loss to one output."""
    c = case(name, variant)
    ups = c["upstream"] if only is None else {only: c["upstream"][only]}
    return po.gradients(inputs(c), c["camera"], ups, c["blur_size"], wrt=wrt, **c["flags"])
