"""Deterministic edge inputs for the depth lift (tests/test_hip_surfels_edges.py on the GPU, tests/
test_surfels_edge_cases_cpu.py here): what the seeded cases of tests/surfels_cases.py keep away from.  The relu is a
decision on the exact fp32 input, so every value below is a case, not a hazard.  Same dict layout as surfels_cases.

    special_3x3, special_3x3_camera   one depth per pixel (SPECIAL, in pixel order), world and camera frame:
        0  +0.0             d = 0: the eye (world) / 0 (camera), gradient exactly 0
        1  -0.0             the same
        2  1e-45            the smallest subnormal: > 0, so the full gradient
        3  1.1754944e-38    the smallest normal
        4  +inf             the centre pixel of an odd grid: x = y = 0, so inf * 0 = NaN; the gradient is finite
        5  -inf             d = 0
        6  1e30
        7  NaN              a NaN stays a NaN; the gradient is passed through (threshold_backward)
        8  2.0              an ordinary pixel
      NONFINITE names the pixels whose output is non-finite in every component: fixed by the case, not by a result.
    row_1x300, column_300x1           B = 2; a linspace of ONE sample along one axis and 300 pixels along the other: two
                                      workgroups of 256 lanes, the second partly empty.  Depths as in surfels_cases: an
                                      eighth exactly 0 or negative, the others in 1.5..3
    b5_1x1                            five views of one pixel: the launch grid is (1, 5); views 1 and 3 have depth 0 and -1
"""
import functools

import numpy as np

import projection_cases as pc
import surfels_oracle as so

NAMES = ("special_3x3", "special_3x3_camera", "row_1x300", "column_300x1", "b5_1x1")
SPECIAL = np.array([0.0, -0.0, 1e-45, 1.1754944e-38, np.inf, -np.inf, 1e30, np.nan, 2.0], dtype=np.float32)
NONFINITE = (4, 7)                 # +inf on the centre pixel, NaN
DEAD = (0, 1, 5)                   # depth <= 0
_SPEC = {  # B, H, W, frame
    "special_3x3": (1, 3, 3, "world"), "special_3x3_camera": (1, 3, 3, "camera"), "row_1x300": (2, 1, 300, "world"),
    "column_300x1": (2, 300, 1, "world"), "b5_1x1": (5, 1, 1, "world"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    B, H, W, frame = _SPEC[name]
    N = H * W
    rng = np.random.RandomState(7100 + NAMES.index(name))
    eye, at, up = pc.draw_camera(rng, B)
    if name.startswith("special"):
        depth = SPECIAL.reshape(1, N).copy()
    else:
        depth = rng.uniform(1.5, 3.0, (B, N))
        if name == "b5_1x1":
            depth[1, 0], depth[3, 0] = 0.0, -1.0
        else:
            for b in range(B):
                bad = rng.permutation(N)[:-(-N // 8)]
                depth[b, bad[0::2]] = 0.0
                depth[b, bad[1::2]] = -rng.uniform(0.5, 1.5, len(bad[1::2]))
            depth[:, N - 1] = 2.5 - np.arange(B)            # the last lane of the partly empty workgroup is alive
        depth = pc.f32(depth)
    return {"depth": depth, "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY),
                                       "focal_length": pc.FOCAL},
            "frame": frame, "shape": (B, H, W), "upstream": {"pos": pc.f32(rng.uniform(-1, 1, (B, N, 3)))}}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(values {'pos': [B, N, 3]}, gradients {'depth': like the input}) from the fp64 oracle, computed once."""
    c = case(name)
    return so.gradients({"depth": c["depth"]}, c["camera"], c["upstream"], c["frame"])


def full_gradient(c):
    """[B, N] fp64: the gradient every pixel would get were its depth positive, g . dP/dd with dP_cc/dd = (x_j / f,
    y_i / f, -1) -- written out here, without autograd and without the relu."""
    B, H, W = c["shape"]
    f = float(c["camera"]["focal_length"])
    gx, gy = so.pixel_grid(c["camera"])
    d = np.stack((np.tile(gx, H) / f, np.repeat(gy, W) / f, -np.ones(H * W)), axis=-1)               # [N, 3]
    if c["frame"] == "world":
        R, _ = so.camera_to_world(c["camera"])
        d = np.einsum("brc,nc->bnr", R.numpy(), d)
    else:
        d = np.broadcast_to(d, (B, H * W, 3))
    return np.sum(d * c["upstream"]["pos"].astype(np.float64), axis=-1)
