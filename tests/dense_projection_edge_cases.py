"""Deterministic edge inputs for the dense re-projection (tests/test_hip_dense_projection_edges.py on the GPU, tests/
test_dense_projection_edge_cases_cpu.py here, tools/gen_dense_projection_golden.py for the RECORDED ones): what the
seeded frames of tests/dense_projection_cases.py never reach.  Same dict layout and the same four uses per frame (grid
and flat, with and without a rotated image) as dense_projection_cases; `named` holds the indices of the surfels a case
places by hand.  Names are H x W; `sigma` is that of the grid layout in pixels, the flat layout's is H times as much.

    row_1x5, col_5x1, one_1x1   D = 2, 2, 1, sigma 0.8: along an axis of one pixel the scale (W - 1) / w is exactly 0 and
                      every surfel has u = 0; the row pitch of the backward's strips is 16 for one column
    far_9x7           D = 3, sigma 0.9.  Surfels 0..11 are lifted from pixel coordinates 1e3, 1e6 and 1e12 pixels beyond
                      the left, right, top and bottom side, at ordinary depth: finite in fp32, weight exactly 0 on every
                      pixel in fp64.  In k_dproj_fwd's recurrence their outward factor overflows to inf and the entry it
                      would give is NaN; the result is clean because no such entry is ever written
    sigma_0p1_9x7, sigma_0p03_9x7   D = 3: q = exp(-1 / sigma^2) is 4e-44 and 0, most weights are denormal or 0, and the
                      normalised `out` divides by m + 1e-10 with m far below 1e-10 on most pixels
    sigma_12_9x7      D = 3: every surfel weighs on every pixel, the mask is about 60
    tile_33x33        D = 1, sigma 0.8: the first frame with a second tile in both directions, each one pixel wide

Every case keeps |Z| >= Z_MARGIN (dense_projection_oracle.z_margin), the layer's one kink; a draw that does not is
redrawn from the next seed of the case's own range.  No non-finite input: an inf coordinate projects to NaN, and by the
layer's definition a NaN reaches every pixel."""
import functools

import numpy as np
import torch

import dense_projection_oracle as do
from dense_projection_cases import LAYOUTS, Z_MARGIN
from projection_cases import FOCAL, FOVY, draw_camera, f32, jittered_grid, lift

NAMES = ("row_1x5", "col_5x1", "one_1x1", "far_9x7", "sigma_0p1_9x7", "sigma_0p03_9x7", "sigma_12_9x7", "tile_33x33")
_SPEC = {  # B, H, W, D, sigma of the grid layout (pixels)
    "row_1x5": (1, 1, 5, 2, 0.8), "col_5x1": (1, 5, 1, 2, 0.8), "one_1x1": (1, 1, 1, 1, 0.8),
    "far_9x7": (1, 9, 7, 3, 0.9), "sigma_0p1_9x7": (1, 9, 7, 3, 0.1), "sigma_0p03_9x7": (1, 9, 7, 3, 0.03),
    "sigma_12_9x7": (1, 9, 7, 3, 12.0), "tile_33x33": (1, 33, 33, 1, 0.8),
}
ALL = [(n, layout, rotated) for n in NAMES for layout in LAYOUTS for rotated in (False, True)]
# tests/golden/dense_projection/dp2_<name>_grid.npz: without a rotated image, which the reference cannot run with
RECORDED = (("row_1x5", "grid"), ("far_9x7", "grid"))
FAR = tuple(range(12))                 # far_9x7: (left, right, top, bottom) x (1e3, 1e6, 1e12)
FAR_DISTANCES = (1e3, 1e6, 1e12)


def _draw(name, seed):
    B, H, W, D, sigma = _SPEC[name]
    rng = np.random.RandomState(seed)
    N = H * W
    eye, at, up = draw_camera(rng, B)
    px, py = jittered_grid(rng, B, H, W, 1.2)
    z = rng.uniform(1.5, 3.0, (B, N))
    named = ()
    if name == "far_9x7":
        named = FAR
        for i, dist in enumerate(FAR_DISTANCES):
            px[0, i], px[0, 3 + i], py[0, 6 + i], py[0, 9 + i] = -dist, W + dist, -dist, H + dist
    return {"surfels": f32(lift(px, py, z, eye, at, up, W, H)), "rgb": f32(rng.uniform(0, 1, (B, H, W, D))),
            "rotated_image": f32(rng.uniform(0, 1, (B, H, W, D))), "named": named,
            "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(FOVY), "focal_length": FOCAL},
            "blur_size": float(np.float32(6 * sigma / W)), "shape": (B, H, W, D),
            "upstream": {"out": f32(rng.uniform(-1, 1, (B, H, W, D))), "mask": f32(rng.uniform(-1, 1, (B, H, W, 1)))}}


@functools.lru_cache(maxsize=None)
def _frame(name):
    first = 12500 + 100 * NAMES.index(name)
    for seed in range(first, first + 50):
        c = _draw(name, seed)
        if np.isfinite(c["surfels"]).all() and do.z_margin(c["surfels"], c["camera"]) >= Z_MARGIN:
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} is clear of Z = 0")


@functools.lru_cache(maxsize=None)
def case(name, layout="grid", rotated=False):
    c = dict(_frame(name))
    B, H, W, D = c["shape"]
    lead = (B, H, W) if layout == "grid" else (B, H * W)
    c["rgb"] = c["rgb"].reshape(*lead, D)
    c["rotated_image"] = c["rotated_image"].reshape(*lead, D) if rotated else None
    c["upstream"] = {"out": c["upstream"]["out"].reshape(*lead, D), "mask": c["upstream"]["mask"].reshape(*lead, 1)}
    c["layout"] = layout
    return c


def sigma(c):
    return do.sigma_of(c["rgb"].shape, c["blur_size"])


def pixels(c):
    """[B, N, 3] fp64: the pixel coordinates (and -Z) of a case's surfels."""
    return do.pixel_coordinates(torch.as_tensor(c["surfels"].astype(np.float64)), c["camera"]).numpy()


def inputs(c):
    return {k: c[k] for k in do.INPUTS}


def tag(name, layout="grid", rotated=False):
    return f"{name}_{layout}" + ("_rot" if rotated else "")


@functools.lru_cache(maxsize=None)
def expected(name, layout="grid", rotated=False, fn=do.project):
    """(values {output: array}, gradients {input: like the input}) from the fp64 oracle, computed once; `fn`: the
    oracle's dense form, or project_separable."""
    c = case(name, layout, rotated)
    return do.gradients(inputs(c), c["camera"], c["upstream"], c["blur_size"], fn=fn)
