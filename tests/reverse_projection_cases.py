"""Seeded inputs for the reverse re-projection tests (tests/test_hip_reverse_projection.py on the GPU, tests/
test_reverse_projection_oracle_cpu.py here) and for tools/gen_reverse_projection_golden.py, which records the reference
on them.

A case is a dict: `rgb` and (where the case merges) `rotated_image` [B, H, W, D], `in_pos_wc` and `out_pos_wc`
[B, H W, 3], all fp32-representable; `camera1` (the source camera, which out_pos_wc is projected into) and `camera2`
(the target camera, for in_pos_wc): eye / at / up [B, 3] or [B, 4], viewport, and a fovy and focal_length that differ
between the two; `flags` (compute_new_depth, depth_epsilon); `upstream` {output: fp32 gradient [B, H, W, .]}; `wrt` (the
inputs that require grad) and `only` (None, or the one output the loss reads).  Names are H x W, the smallest shapes at
which each piece can go wrong:
    1x1          D = 1, rotated image: every coordinate is exactly 1/2, which fails the 0.5-pixel frame test, so mask = 0
                 and out = rotated_image, while image1 is still sampled (with weight 1 on the one texel)
    2x2          D = 1, no rotated image: the frame border dominates
    3x5          D = 4, non-square: W / H swaps in the aspect ratio, the normalisation and the mask bounds
    12x16        B = 2, two camera pairs, rotated image, compute_new_depth; in_pos_wc and out_pos_wc are what the two
                 cameras see, pixel centre by pixel centre, of ONE two-layer surface (a raised square over a plane, both
                 with a shallow relief), so the depth test rejects real occlusions
    17x9         B = 3, homogeneous camera vectors; samples off every edge, a few points behind each camera
    cluster_8x8  all 64 output pixels sample one source cell: the longest backward list, and texels whose gradient is 0
    36x48        1728 pixels: the lists cross workgroup boundaries
VARIANTS are the variants of 12x16, one per switch: depth_epsilon = 0, no rotated image, no new depth, each input
alone requiring grad, a loss on each output alone.  FUNCTION_VARIANTS are those that change the function's values;
they have fixtures.

Except in 12x16, positions are drawn in the camera's frame that projects them -- a pixel coordinate near each pixel's
centre and a depth -- and lifted to world coordinates.

Conditions (reverse_projection_oracle.decision_margin >= 1, in fp64, under every depth_epsilon the case is used with):
for both projections every component of `pixel coordinate - 0.5` at least 1e-4 from an integer (except along an axis of
one pixel, where the coordinate is exactly 1/2 by construction) and |Z| >= 1e-3; |d - d_out - depth_epsilon| >= 1e-4.
In 12x16 each of the two mask values holds at least 10 % of the pixels, at depth_epsilon 0.1 and at 0.  A draw that
violates one is redrawn from the next seed; tests/test_reverse_projection_oracle_cpu.py asserts them for every case, so
no comparison leaves an element out."""
import functools

import numpy as np

import reverse_projection_oracle as ro
from projection_cases import draw_camera, f32, jittered_grid, lift, pixel_centres, rays
from projection_checks import one_view

NAMES = ("1x1", "2x2", "3x5", "12x16", "17x9", "cluster_8x8", "36x48")
_SPEC = {  # B, H, W, D, rotated, compute_new_depth, jitter (pixels)
    "1x1": (1, 1, 1, 1, True, True, 0.4),
    "2x2": (1, 2, 2, 1, False, False, 0.45),
    "3x5": (1, 3, 5, 4, True, True, 1.2),
    "12x16": (2, 12, 16, 3, True, True, 0.0),
    "17x9": (3, 17, 9, 2, False, True, 3.0),
    "cluster_8x8": (1, 8, 8, 3, False, False, 0.3),
    "36x48": (1, 36, 48, 3, True, True, 1.2),
}
FUNCTION_VARIANTS = {"eps0": {"flags": {"depth_epsilon": 0.0}}, "no_rotated": {"rotated_image": None},
                     "no_depth": {"flags": {"compute_new_depth": False}}}
VARIANTS = dict(FUNCTION_VARIANTS,
                **{"wrt_" + k: {"wrt": (k,)} for k in ro.INPUTS}, **{"only_" + k: {"only": k} for k in ro.OUTPUTS})
VARIANT_OF = "12x16"
CAMERAS = ((np.deg2rad(40.0), 0.5), (np.deg2rad(50.0), 0.8))        # (fovy, focal_length) of camera1, camera2


# the two-layer surface: the plane z = 0, and z = RAISED over |x|, |y| < SQUARE; on both a relief of amplitude RELIEF,
# well under the default depth_epsilon and a few pixels long, so that no pixel's depth agrees with its twice-resampled
# depth to 1e-4 (on a plane the two differ by the interpolation error alone, which passes through 0)
SQUARE, RAISED, RELIEF = 0.7, 1.0, 0.04


def seen(eye, at, up, W, H, fovy, focal):
    """What each pixel centre of the cameras sees of the two-layer surface: world positions [B, H W, 3]."""
    r = rays(*pixel_centres(eye.shape[0], H, W), eye, at, up, W, H, fovy, focal)
    e = eye[:, None].astype(np.float64)
    top = e - ((e[..., 2:] - RAISED) / r[..., 2:]) * r
    ground = e - (e[..., 2:] / r[..., 2:]) * r
    hit = (np.abs(top[..., :1]) < SQUARE) & (np.abs(top[..., 1:2]) < SQUARE)
    p = np.where(hit, top, ground)
    p[..., 2] += RELIEF * np.sin(9.0 * p[..., 0] + 1.0) * np.sin(9.0 * p[..., 1] + 2.0)
    return p


def _draw(name, seed):
    B, H, W, D, rotated, new_depth, jitter = _SPEC[name]
    rng = np.random.RandomState(seed)
    N = H * W
    cams = [draw_camera(rng, B, side) for side in ((-0.9, 0.9) if name == "12x16" else (0.0, 0.0))]
    if name == "12x16":
        pos = [seen(*cams[k], W, H, *CAMERAS[k]) for k in (0, 1)]       # in_pos by camera1, out_pos by camera2
        pos = {"in_pos_wc": pos[0], "out_pos_wc": pos[1]}
    else:
        pos = {}
        for key, k in (("out_pos_wc", 0), ("in_pos_wc", 1)):             # out_pos is projected by camera1, in_pos by 2
            px, py = jittered_grid(rng, B, H, W, jitter)
            z = rng.uniform(1.5, 3.0, (B, N))
            if name == "cluster_8x8" and k == 0:
                px, py = 3.5 + rng.uniform(0.15, 0.85, (B, N)), 3.5 + rng.uniform(0.15, 0.85, (B, N))   # cell (3, 3)
                z = 2.0 + rng.uniform(-0.02, 0.02, (B, N))           # near one depth: the mask is not all 0
            if name == "17x9":
                z[:, rng.permutation(N)[:4]] = -rng.uniform(0.5, 1.5, (B, 4))                           # behind the camera
            pos[key] = lift(px, py, z, *cams[k], W, H, *CAMERAS[k])
    hom = name == "17x9"

    def camera(k):
        eye, at, up = cams[k]
        one, zero = np.ones((B, 1), np.float32), np.zeros((B, 1), np.float32)
        return {"eye": np.concatenate((eye, one), -1) if hom else eye, "at": np.concatenate((at, one), -1) if hom else at,
                "up": np.concatenate((up, zero), -1) if hom else up, "viewport": [0, 0, W, H],
                "fovy": float(CAMERAS[k][0]), "focal_length": CAMERAS[k][1]}

    case = {"rgb": f32(rng.uniform(0, 1, (B, H, W, D))), "in_pos_wc": f32(pos["in_pos_wc"]),
            "out_pos_wc": f32(pos["out_pos_wc"]),
            "rotated_image": f32(rng.uniform(0, 1, (B, H, W, D))) if rotated else None,
            "camera1": camera(0), "camera2": camera(1),
            "flags": {"compute_new_depth": new_depth, "depth_epsilon": 0.1}, "shape": (B, H, W, D),
            "wrt": ro.INPUTS, "only": None}
    case["upstream"] = {k: f32(rng.uniform(-1, 1, (B, H, W, D if k in ("out", "image1") else 1))) for k in ro.OUTPUTS
                        if k != "depth" or new_depth}
    return case


def epsilons(name):
    """Every depth_epsilon a case is used with."""
    return (0.1, 0.0) if name == VARIANT_OF else (0.1,)


def margin(c, name):
    return min(ro.decision_margin(c["in_pos_wc"], c["out_pos_wc"], c["camera1"], c["camera2"], e) for e in epsilons(name))


def mask_shares(c, name):
    """Per depth_epsilon the case is used with, the share of pixels whose mask is 1 (fp64 oracle)."""
    import torch
    t = {k: torch.as_tensor(np.asarray(c[k], dtype=np.float64)) for k in ("rgb", "in_pos_wc", "out_pos_wc")}
    return [float(ro.project(t["rgb"], t["in_pos_wc"], t["out_pos_wc"], c["camera1"], c["camera2"],
                             depth_epsilon=e)["mask"].mean()) for e in epsilons(name)]


def clear(c, name):
    if margin(c, name) < 1.0:
        return False
    return name != VARIANT_OF or all(0.1 <= s <= 0.9 for s in mask_shares(c, name))


@functools.lru_cache(maxsize=None)
def case(name, variant=None):
    if variant is not None:
        c = dict(case(VARIANT_OF))
        for k, v in VARIANTS[variant].items():
            c[k] = dict(c[k], **v) if k == "flags" else v
        if not c["flags"]["compute_new_depth"]:
            c["upstream"] = {k: u for k, u in c["upstream"].items() if k != "depth"}
        return c
    for seed in range(1000 * NAMES.index(name), 1000 * NAMES.index(name) + 50):
        c = _draw(name, seed)
        if clear(c, name):
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} meets the conditions")


def inputs(c):
    return {k: c[k] for k in ro.INPUTS}


def view(c, b):
    """View b of a case as a case of its own."""
    return one_view(c, b, ro.INPUTS, ("camera1", "camera2"))


ALL = [(n, None) for n in NAMES] + [(VARIANT_OF, v) for v in VARIANTS]
FIXTURES = [(n, None) for n in NAMES] + [(VARIANT_OF, v) for v in FUNCTION_VARIANTS]


def tag(name, variant=None):
    return name if variant is None else f"{name}_{variant}"


def gradients(c):
    """(values, gradients) of a case from the fp64 oracle, under the case's own `wrt` and `only`."""
    ups = c["upstream"] if c["only"] is None else {c["only"]: c["upstream"][c["only"]]}
    return ro.gradients(inputs(c), c["camera1"], c["camera2"], ups, wrt=c["wrt"], **c["flags"])


@functools.lru_cache(maxsize=None)
def expected(name, variant=None):
    """gradients(case(name, variant)), computed once."""
    return gradients(case(name, variant))
