"""Seeded inputs for the hard-projection tests (tests/test_hip_hard_projection.py on the GPU, tests/
test_hard_projection_oracle_cpu.py here) and for tools/gen_hard_projection_golden.py, which records the reference on them.

A case is a dict: `surfels` [B, N, 3], `rgb` as [B, H, W, D] or [B, N, D], fp32; `camera` (eye / at / up [B, 3] or
[B, 4], viewport, fovy, focal_length); `shape` (B, H, W, D); `upstream` {'out': fp32 gradient like rgb}.  Surfels are
drawn like projection_cases._draw: a jittered pixel coordinate and a depth, lifted with projection_cases.lift.  Names are
H x W, the smallest shapes at which each piece can go wrong:
    1x1          one surfel, one pixel
    2x2          D = 1
    3x5          D = 4, odd and non-square
    12x16        B = 2, two cameras
    17x9         B = 3, [B, N, D] layout, homogeneous camera vectors; surfels off every edge, a few behind the camera
    cluster_8x8  all 64 surfels in one pixel, 63 pixels empty: the longest run
    36x48        1728 surfels: the runs cross workgroup boundaries

Kink condition (hard_projection_oracle.kink_margin >= 1, in fp64): every pixel-coordinate component at least 1e-4 from an
integer -- where round(coordinate - 1/2) ties -- and |Z| >= 1e-3.  A draw that violates it is redrawn from the next seed;
tests/test_hard_projection_oracle_cpu.py asserts it for every case, so no comparison leaves an element out."""
import functools

import numpy as np

import hard_projection_oracle as ho
import projection_cases as pc

NAMES = ("1x1", "2x2", "3x5", "12x16", "17x9", "cluster_8x8", "36x48")
_SPEC = {  # B, H, W, D, flat layout, jitter (pixels)
    "1x1": (1, 1, 1, 3, False, 0.4),
    "2x2": (1, 2, 2, 1, False, 0.9),
    "3x5": (1, 3, 5, 4, False, 1.2),
    "12x16": (2, 12, 16, 3, False, 1.2),
    "17x9": (3, 17, 9, 2, True, 3.0),
    "cluster_8x8": (1, 8, 8, 3, False, 0.0),
    "36x48": (1, 36, 48, 3, False, 1.2),
}


def _draw(name, seed):
    B, H, W, D, flat, jitter = _SPEC[name]
    rng = np.random.RandomState(seed)
    N = H * W
    eye, at, up = pc.draw_camera(rng, B)
    px, py = pc.jittered_grid(rng, B, H, W, jitter)
    z = rng.uniform(1.5, 3.0, (B, N))
    if name == "cluster_8x8":
        px, py = 3.0 + rng.uniform(0.1, 0.9, (B, N)), 3.0 + rng.uniform(0.1, 0.9, (B, N))         # pixel (3, 3)
    if name == "17x9":
        z[:, rng.permutation(N)[:4]] = -rng.uniform(0.5, 1.5, (B, 4))                             # behind the camera
    shape = (B, N, D) if flat else (B, H, W, D)
    hom = name == "17x9"
    return {"surfels": pc.f32(pc.lift(px, py, z, eye, at, up, W, H)), "rgb": pc.f32(rng.uniform(0, 1, shape)),
            "camera": {"eye": np.concatenate((eye, np.ones((B, 1), np.float32)), -1) if hom else eye,
                       "at": np.concatenate((at, np.ones((B, 1), np.float32)), -1) if hom else at,
                       "up": np.concatenate((up, np.zeros((B, 1), np.float32)), -1) if hom else up,
                       "viewport": [0, 0, W, H], "fovy": float(pc.FOVY), "focal_length": pc.FOCAL},
            "shape": (B, H, W, D), "upstream": {"out": pc.f32(rng.uniform(-1, 1, shape))}}


@functools.lru_cache(maxsize=None)
def case(name):
    for seed in range(5000 + 100 * NAMES.index(name), 5000 + 100 * NAMES.index(name) + 50):
        c = _draw(name, seed)
        if ho.kink_margin(c["surfels"], c["camera"]) >= 1.0:
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} is clear of every kink")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(values {'out', 'mask', 'count', 'index'}, gradients {'rgb'}) from the fp64 oracle, computed once."""
    c = case(name)
    return ho.gradients({"surfels": c["surfels"], "rgb": c["rgb"]}, c["camera"], c["upstream"])


@functools.lru_cache(maxsize=None)
def magnitudes(name):
    """({'out'}, {'rgb'}): the oracle's sums of |terms| per entry (tests/entry_checks.py), computed once."""
    c = case(name)
    return ho.magnitudes({"surfels": c["surfels"], "rgb": c["rgb"]}, c["camera"], c["upstream"])
