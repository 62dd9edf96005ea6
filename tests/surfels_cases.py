"""Seeded inputs for the depth-lift tests (tests/test_hip_surfels.py on the GPU, tests/test_surfels_oracle_cpu.py here)
and for tools/gen_surfels_golden.py, which records the reference on them.

A case is a dict: `depth` fp32 in one of the three accepted shapes; `camera` (eye / at / up [B, 3] or [B, 4], viewport,
fovy, focal_length); `frame`; `shape` (B, H, W); `upstream` {'pos': fp32 gradient [B, N, 3]}.  Names are H x W, the
smallest shapes at which each piece can go wrong:
    1x1          a linspace of one sample along both axes: the point is on the optical axis
    1x4, 4x1     a linspace of one sample along one axis
    2x2          the grid is its end points only
    3x5          odd and non-square, depth as [B, H, W]
    12x16        B = 2, two cameras, depth as [B, H, W, 1]
    17x9         B = 3, homogeneous camera vectors
    36x48        1728 pixels: several workgroups, the last one partly empty
The variant `camera` of 12x16 returns camera coordinates.

In every case with more than one pixel at least one eighth of the depths (and at least two) are exactly 0 or negative,
alternately: the relu branch, where the point is the eye and the gradient exactly 0.  Every other depth is in 1.5..3, so
|depth| >= 1e-3 throughout and no input sits near the kink at 0."""
import functools

import numpy as np

import projection_cases as pc
import surfels_oracle as so

NAMES = ("1x1", "1x4", "4x1", "2x2", "3x5", "12x16", "17x9", "36x48")
_SPEC = {  # B, H, W, depth layout
    "1x1": (1, 1, 1, "flat"), "1x4": (1, 1, 4, "flat"), "4x1": (1, 4, 1, "image"), "2x2": (1, 2, 2, "flat"),
    "3x5": (1, 3, 5, "image"), "12x16": (2, 12, 16, "image1"), "17x9": (3, 17, 9, "flat"), "36x48": (1, 36, 48, "image"),
}
VARIANTS = {"camera": {"frame": "camera"}}
VARIANT_OF = "12x16"
ALL = [(n, None) for n in NAMES] + [(VARIANT_OF, v) for v in VARIANTS]


def shaped(depth, B, H, W, layout):
    return depth.reshape({"flat": (B, H * W), "image": (B, H, W), "image1": (B, H, W, 1)}[layout])


@functools.lru_cache(maxsize=None)
def case(name, variant=None):
    if variant is not None:
        return dict(case(VARIANT_OF), **VARIANTS[variant])
    B, H, W, layout = _SPEC[name]
    N = H * W
    rng = np.random.RandomState(7000 + NAMES.index(name))
    eye, at, up = pc.draw_camera(rng, B)
    depth = rng.uniform(1.5, 3.0, (B, N))
    if N > 1:
        for b in range(B):
            bad = rng.permutation(N)[:max(2, -(-N // 8))]
            depth[b, bad[0::2]] = 0.0
            depth[b, bad[1::2]] = -rng.uniform(0.5, 1.5, len(bad[1::2]))
    hom = name == "17x9"
    return {"depth": shaped(pc.f32(depth), B, H, W, layout),
            "camera": {"eye": np.concatenate((eye, np.ones((B, 1), np.float32)), -1) if hom else eye,
                       "at": np.concatenate((at, np.ones((B, 1), np.float32)), -1) if hom else at,
                       "up": np.concatenate((up, np.zeros((B, 1), np.float32)), -1) if hom else up,
                       "viewport": [0, 0, W, H], "fovy": float(pc.FOVY), "focal_length": pc.FOCAL},
            "frame": "world", "shape": (B, H, W), "upstream": {"pos": pc.f32(rng.uniform(-1, 1, (B, N, 3)))}}


def tag(name, variant=None):
    return name if variant is None else f"{name}_{variant}"


@functools.lru_cache(maxsize=None)
def expected(name, variant=None, grid="numpy"):
    """(values {'pos': [B, N, 3]}, gradients {'depth': like the input}) from the fp64 oracle, computed once."""
    c = case(name, variant)
    return so.gradients({"depth": c["depth"]}, c["camera"], c["upstream"], c["frame"], grid)


@functools.lru_cache(maxsize=None)
def magnitudes(name, variant=None, grid="numpy"):
    """({'pos'}, {'depth'}, {eye, at, up}): the oracle's sums of |terms| per entry (tests/entry_checks.py), computed
    once."""
    c = case(name, variant)
    return so.magnitudes({"depth": c["depth"]}, c["camera"], c["upstream"], c["frame"], grid)
