"""Seeded inputs for the dense re-projection tests (tests/test_hip_dense_projection.py on the GPU, tests/
test_dense_projection_oracle_cpu.py here) and for tools/gen_dense_projection_golden.py, which records the reference on
them.

A case is a dict: `surfels` [B, N, 3], `rgb` and (where the case merges) `rotated_image` as [B, H, W, D] ("grid") or
[B, N, D] ("flat"), all fp32-representable; `camera` (eye / at / up [B, 3], viewport, fovy, focal_length); `blur_size`;
`upstream` {'out': like rgb, 'mask': [..., 1]} fp32.  Frames are H x W, the smallest at which each piece can go wrong:
    2x2      D = 1: one tile, one partial chunk
    3x5      D = 4, odd and non-square: sigma from W (1.0) differs from sigma from H (0.6)
    12x16    B = 2, two cameras; 192 surfels = three whole chunks of 64, one whole strip of 16 columns
    17x9     B = 3; surfels up to three pixels (several sigma) off every edge and four per view behind the camera
    36x48    B = 2; 2 x 2 pixel tiles of 32 with remainders 4 and 16, 27 chunks, three strips
    35x37    2 x 2 tiles with remainders 3 and 5, 1295 surfels = 20 chunks and 15 more (and 20 backward workgroups and 15
             lanes more), three strips the last of 5 columns: every tiled dimension more than once, with a remainder
Every frame is used in both layouts, with and without a rotated image: the same surfels and values, reshaped.  blur_size
is chosen per frame so that sigma for the grid layout, blur_size * W / 6, is between 0.6 and 1.5 pixels; the flat layout
then has sigma = blur_size * N / 6, H times as much (the reference's quirk).

The layer's one kink is Z = 0: a draw with any |Z| < 1e-3 (fp64) is redrawn from the next seed, and tests/
test_dense_projection_oracle_cpu.py asserts the margin, so no comparison leaves an element out."""
import functools

import numpy as np

import dense_projection_oracle as do
from projection_cases import FOCAL, FOVY, draw_camera, f32, jittered_grid, lift

FRAMES = ("2x2", "3x5", "12x16", "17x9", "36x48", "35x37")
_SPEC = {  # B, H, W, D, sigma of the grid layout (pixels), jitter (pixels)
    "2x2": (1, 2, 2, 1, 0.6, 0.9),
    "3x5": (1, 3, 5, 4, 1.0, 1.2),
    "12x16": (2, 12, 16, 3, 1.2, 1.2),
    "17x9": (3, 17, 9, 2, 0.9, 3.0),
    "36x48": (2, 36, 48, 3, 1.5, 1.2),
    "35x37": (1, 35, 37, 3, 0.8, 1.2),
}
LAYOUTS = ("grid", "flat")
Z_MARGIN = 1e-3
ALL = [(f, layout, rotated) for f in FRAMES for layout in LAYOUTS for rotated in (False, True)]
# what the reference is recorded on (it cannot run with a rotated image): every frame as a grid, the small ones flat too
RECORDED = [(f, "grid") for f in FRAMES] + [(f, "flat") for f in FRAMES[:4]]


def _draw(frame, seed):
    B, H, W, D, sigma, jitter = _SPEC[frame]
    rng = np.random.RandomState(seed)
    N = H * W
    eye, at, up = draw_camera(rng, B)
    px, py = jittered_grid(rng, B, H, W, jitter)
    z = rng.uniform(1.5, 3.0, (B, N))
    if frame == "17x9":
        z[:, rng.permutation(N)[:4]] = -rng.uniform(0.5, 1.5, (B, 4))          # behind the camera
    return {"surfels": f32(lift(px, py, z, eye, at, up, W, H)), "rgb": f32(rng.uniform(0, 1, (B, H, W, D))),
            "rotated_image": f32(rng.uniform(0, 1, (B, H, W, D))),
            "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(FOVY), "focal_length": FOCAL},
            "blur_size": float(np.float32(6 * sigma / W)), "shape": (B, H, W, D),
            "upstream": {"out": f32(rng.uniform(-1, 1, (B, H, W, D))), "mask": f32(rng.uniform(-1, 1, (B, H, W, 1)))}}


@functools.lru_cache(maxsize=None)
def _frame(frame):
    for seed in range(1000 * FRAMES.index(frame), 1000 * FRAMES.index(frame) + 50):
        c = _draw(frame, seed)
        if do.z_margin(c["surfels"], c["camera"]) >= Z_MARGIN:
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {frame} is clear of Z = 0")


@functools.lru_cache(maxsize=None)
def case(frame, layout="grid", rotated=False):
    c = dict(_frame(frame))
    B, H, W, D = c["shape"]
    lead = (B, H, W) if layout == "grid" else (B, H * W)
    c["rgb"] = c["rgb"].reshape(*lead, D)
    c["rotated_image"] = c["rotated_image"].reshape(*lead, D) if rotated else None
    c["upstream"] = {"out": c["upstream"]["out"].reshape(*lead, D), "mask": c["upstream"]["mask"].reshape(*lead, 1)}
    c["layout"] = layout
    return c


def sigma(c):
    return do.sigma_of(c["rgb"].shape, c["blur_size"])


def inputs(c):
    return {k: c[k] for k in do.INPUTS}


def tag(frame, layout="grid", rotated=False):
    return f"{frame}_{layout}" + ("_rot" if rotated else "")


@functools.lru_cache(maxsize=None)
def expected(frame, layout="grid", rotated=False, wrt=do.INPUTS, only=None):
    """(values {output: array}, gradients {input: like the input}) from the fp64 oracle, computed once; `only`
    restricts the loss to one output."""
    c = case(frame, layout, rotated)
    ups = c["upstream"] if only is None else {only: c["upstream"][only]}
    return do.gradients(inputs(c), c["camera"], ups, c["blur_size"], wrt=wrt)
