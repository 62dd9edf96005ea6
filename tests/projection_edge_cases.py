"""Deterministic edge inputs for the surfel re-projection layer (tests/test_hip_projection_edges.py on the GPU, tests/
test_projection_edge_cases_cpu.py here, tools/gen_projection_golden.py for the RECORDED ones): what the seeded cases of
tests/projection_cases.py are redrawn to avoid, or never reach.  Same dict layout as projection_cases; `named` holds the
indices of the surfels a case places by hand.  Names are H x W; every case computes the new depth.

    half0_5x7         D = 4, rotated image, default blur_size 0.15: half = floor(0.075 H) = 0, one tap.  2 D + 1 = 9
                      blurred channels, the most there can be
    half0_raw_5x7     the same inputs with blur_rotated_image=False: `out` is the rotated image bit for bit where mask = 0
    half64_16x4       D = 1, rotated image, blur_size 8.01: half = 64, the cap, in a frame 16 rows tall
    row_1x9, col_9x1, one_1x1   D = 2, 2, 1, rotated image, half 0: along an axis of one pixel the scale (W - 1) / w is
                      exactly 0, so u = W / 2 - 1 / 2 = 0 and fx = 0 for every surfel.  one_1x1 is drawn at depth 5 to 6,
                      where the lone pixel's mask a / (a + 1e-8) is 1e-3 below 1 and not 1e-6
    block_16x16       N = 256, one whole workgroup; D = 1, rotated image, blur_size 0.4 (half 3)
    lane_1x257        N = 257: a second workgroup of one lane; D = 2, rotated image, half 0
    all_dropped_3x5   every surfel off the frame, a third behind the camera as well; rotated image.  Every range stays
                      [0, 0), the mask is 0 everywhere
    all_dropped_b2    B = 2: view 0 all dropped, view 1 ordinary
    exact_5x7         axis camera (eye 0, at (0, 0, -1), up (0, 1, 0)).  Surfel 0 on the axis in front and 2 at the origin:
                      u = 3, v = 2, fx = fy = 0, three betas exactly 0.  Surfel 1 at (0.001, 0.002, 0): Z exactly 0
                      (divided by 1), in the frame.  Surfel 3 has x = 0 only (fx = 0), surfel 4 y = 0 only (fy = 0)
    corner_first_8x8  all 64 surfels in cell (-1, -1): only corner (1, 1) is in the frame, at pixel 0
    corner_last_8x8   all 64 in cell (W - 1, H - 1): only corner (0, 0) is in the frame, at pixel N - 1
    nonfinite_4x6     axis camera.  Surfels 0..7 hold NaN, +-inf, 1e30 and 3e38 components; surfel 8 is finite, off the
                      frame and 400 units behind the camera (its depth weight exp(800) is inf).  Surfel 0 carries NaN rgb

Conditions (margin() >= 1): projection_oracle.decision_margin's, with the integer-distance condition left out along an
axis of one pixel (the coordinate is exactly 0 there in every precision, as in reverse_projection_oracle) and the integer-
distance and |Z| conditions left out for the surfels a case names.  A draw that violates one is redrawn from the next
seed of the case's own range."""
import functools

import numpy as np
import torch

import projection_cases as pc
import projection_oracle as po

NAMES = ("half0_5x7", "half0_raw_5x7", "half64_16x4", "row_1x9", "col_9x1", "one_1x1", "block_16x16", "lane_1x257",
         "all_dropped_3x5", "all_dropped_b2", "exact_5x7", "corner_first_8x8", "corner_last_8x8", "nonfinite_4x6")
RECORDED = ("half0_5x7", "row_1x9", "col_9x1", "exact_5x7", "all_dropped_3x5")     # tests/golden/projection/pr2_<name>.npz
_SPEC = {  # B, H, W, D, blur_size, rotated, axis camera
    "half0_5x7": (1, 5, 7, 4, 0.15, True, False), "half64_16x4": (1, 16, 4, 1, 8.01, True, False),
    "row_1x9": (1, 1, 9, 2, 0.15, True, False), "col_9x1": (1, 9, 1, 2, 0.15, True, False),
    "one_1x1": (1, 1, 1, 1, 0.15, True, False), "block_16x16": (1, 16, 16, 1, 0.4, True, False),
    "lane_1x257": (1, 1, 257, 2, 0.15, True, False), "all_dropped_3x5": (1, 3, 5, 2, 0.15, True, False),
    "all_dropped_b2": (2, 3, 5, 2, 0.15, True, False), "exact_5x7": (1, 5, 7, 3, 0.5, False, True),
    "corner_first_8x8": (1, 8, 8, 3, 0.4, False, False), "corner_last_8x8": (1, 8, 8, 3, 0.4, False, False),
    "nonfinite_4x6": (1, 4, 6, 3, 0.5, False, True),
}
HALF = {"half0_5x7": 0, "half0_raw_5x7": 0, "half64_16x4": 64, "row_1x9": 0, "col_9x1": 0, "one_1x1": 0,
        "block_16x16": 3, "lane_1x257": 0, "all_dropped_3x5": 0, "all_dropped_b2": 0, "exact_5x7": 1,
        "corner_first_8x8": 1, "corner_last_8x8": 1, "nonfinite_4x6": 1}
ON_AXIS, Z_ZERO, FX_ZERO, FY_ZERO = (0, 2), 1, 3, 4          # the named surfels of exact_5x7
FAR = (900.0, 700.0, -2.0)                                   # where nonfinite_4x6's named surfels go for the gradients


def pixels(c):
    """[B, N, 3] fp64: the pixel coordinates (and -Z) of a case's surfels."""
    return po.pixel_coordinates(torch.as_tensor(c["surfels"].astype(np.float64)), c["camera"]).numpy()


def cells(c):
    """([B, N, 2] cell, [B, N, 2] fractions) of a case's surfels, fp64; NaN where the coordinate is."""
    uv = pixels(c)[..., :2] - 0.5
    with np.errstate(invalid="ignore"):                    # inf - inf of an infinite coordinate
        return np.floor(uv), uv - np.floor(uv)


def live(c):
    """[B, N] bool: at least one corner of the surfel's cell can be in the frame (a NaN fails every comparison)."""
    B, H, W, D = c["shape"]
    cell, _ = cells(c)
    return (cell[..., 0] >= -1) & (cell[..., 0] <= W - 1) & (cell[..., 1] >= -1) & (cell[..., 1] <= H - 1)


def margin(c):
    """projection_oracle.decision_margin with the two conditions left out that the module's docstring names."""
    B, H, W, D = c["shape"]
    t = {k: torch.as_tensor(c[k].astype(np.float64)) for k in ("surfels", "rgb")}
    _, mask, _, px = po.scattered(t["surfels"], t["rgb"], c["camera"], c["flags"].get("use_depth", True),
                                  c["flags"].get("use_center_dist", True))
    mask = po.blur(mask, c["blur_size"])
    keep = np.setdiff1d(np.arange(H * W), np.asarray(c["named"], dtype=np.int64))
    px = px[:, keep]
    worst = [float(px[..., 2].abs().min()) / 1e-3]
    for axis, size in ((0, W), (1, H)):
        if size > 1:
            uv = px[..., axis] - 0.5
            worst.append(float((uv - torch.round(uv)).abs().min()) / 1e-4)
    if not bool(torch.isfinite(mask).all()):
        return 0.0
    if bool((mask != 0).any()):
        worst.append(float(mask[mask != 0].abs().min()) / 1e-4)
    if c["rotated_image"] is not None:
        worst.append(float((mask - 1).abs().min()) / 1e-4)
    return min(worst)


def _draw(name, seed):
    B, H, W, D, blur_size, rotated, axis = _SPEC[name]
    rng = np.random.RandomState(seed)
    N = H * W
    if axis:
        eye, at, up = pc.f32([[0, 0, 0]]), pc.f32([[0, 0, -1]]), pc.f32([[0, 1, 0]])
    else:
        eye, at, up = pc.draw_camera(rng, B)
    px, py = pc.jittered_grid(rng, B, H, W, 1.2)
    z = rng.uniform(5.0, 6.0, (B, N)) if name == "one_1x1" else rng.uniform(1.5, 3.0, (B, N))
    named = ()
    if name == "exact_5x7":                                # the coordinate of 3 and 4 that is not exact: inside the frame
        py[0, FX_ZERO], px[0, FY_ZERO] = rng.uniform(1.1, H - 1.1), rng.uniform(1.1, W - 1.1)
    if name.startswith("all_dropped"):
        side = rng.randint(0, 4, N)
        off = rng.uniform(1.0, 3.0, N)
        px[0] = np.where(side == 0, -off, np.where(side == 1, W + off, px[0]))
        py[0] = np.where(side == 2, -off, np.where(side == 3, H + off, py[0]))
        z[0, ::3] = -rng.uniform(0.5, 1.5, len(z[0, ::3]))                                      # and behind the camera
    if name == "corner_first_8x8":                         # u = px - 1/2 in (-1, 0)
        px, py = -0.5 + rng.uniform(0.15, 0.85, (B, N)), -0.5 + rng.uniform(0.15, 0.85, (B, N))
    if name == "corner_last_8x8":                          # u in (W - 1, W)
        px, py = W - 0.5 + rng.uniform(0.15, 0.85, (B, N)), H - 0.5 + rng.uniform(0.15, 0.85, (B, N))
    surfels = pc.f32(pc.lift(px, py, z, eye, at, up, W, H))
    rgb = pc.f32(rng.uniform(0, 1, (B, H, W, D)))
    rot = pc.f32(rng.uniform(0, 1, (B, H, W, D))) if rotated else None
    if name == "exact_5x7":
        named = (0, 1, 2, 3, 4)
        surfels[0, 0], surfels[0, Z_ZERO], surfels[0, 2] = (0, 0, -2), (0.001, 0.002, 0), (0, 0, 0)
        surfels[0, FX_ZERO, 0] = 0.0
        surfels[0, FY_ZERO, 1] = 0.0
    if name == "nonfinite_4x6":
        named = tuple(range(9))
        nan, inf = np.nan, np.inf
        surfels[0, :9] = [(nan, 0, -2), (0.1, inf, -2), (-inf, 0.1, -2), (0.1, 0.1, nan), (0.1, 0.1, inf),
                          (1e30, 0.1, -2), (0.1, -3e38, -2), (3e38, 3e38, -1e-30), (800.0, 0.1, 400.0)]
        rgb[0].reshape(N, D)[0] = nan
    case = {"surfels": surfels, "rgb": rgb, "rotated_image": rot, "named": named,
            "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY),
                       "focal_length": pc.FOCAL},
            "blur_size": blur_size, "flags": {"compute_new_depth": True}, "shape": (B, H, W, D)}
    case["upstream"] = {k: pc.f32(rng.uniform(-1, 1, (B, H, W, D if k in ("out", "image1") else 1))) for k in po.OUTPUTS}
    return case


def sanitized(c):
    """nonfinite_4x6 with its named surfels at FAR (finite, off the frame, in front) and the NaN rgb row 0: the same
    function of every other input, and the case the gradients are taken on -- scatter_add hands a NaN in the dump slot
    to the gradient of every surfel that shares the slot, in the restatement and in the reference alike."""
    s, rgb = c["surfels"].copy(), c["rgb"].copy()
    s[0, list(c["named"])] = FAR
    rgb[0].reshape(-1, rgb.shape[-1])[0] = 0.0
    return dict(c, surfels=s, rgb=rgb)


def _fits(name, c):
    if margin(c) < 1.0:
        return False
    if name == "exact_5x7":                                # the free coordinate of 3 and 4, and their depth, are clear
        p = pixels(c)[0]
        free = np.array([p[FX_ZERO, 1], p[FY_ZERO, 0]]) - 0.5
        if np.abs(free - np.round(free)).min() < 1e-4 or np.abs(p[[FX_ZERO, FY_ZERO], 2]).min() < 1e-3:
            return False
    if name == "nonfinite_4x6" and margin(sanitized(c)) < 1.0:
        return False
    return True


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "half0_raw_5x7":
        c = dict(case("half0_5x7"))
        c["flags"] = dict(c["flags"], blur_rotated_image=False)
        return c
    first = 11000 + 100 * NAMES.index(name)
    for seed in range(first, first + 50):
        c = _draw(name, seed)
        if _fits(name, c):
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} fits")


def inputs(c):
    return {k: c[k] for k in po.INPUTS}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(values {output: [B, H, W, .]}, gradients {input: like the input}) from the fp64 oracle, computed once.  For
    nonfinite_4x6 the values are those of the case as it is and the gradients those of sanitized(case)."""
    c = case(name)
    val, grad = po.gradients(inputs(c), c["camera"], c["upstream"], c["blur_size"], **c["flags"])
    if name == "nonfinite_4x6":
        s = sanitized(c)
        _, grad = po.gradients(inputs(s), s["camera"], s["upstream"], s["blur_size"], **s["flags"])
    return val, grad
