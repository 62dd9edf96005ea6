"""Seeded inputs for the plane-fit tests (tests/test_hip_normals.py on the GPU, tests/test_normals_oracle_cpu.py here)
and for tools/gen_normals_golden.py, which records the reference on them.

A case is a dict: `pos` fp32 [B, H, W, 3] or [B, N, 3]; `camera` (eye / at / up [B, 3], viewport, fovy, focal_length: the
camera the points were lifted with; the layer reads eye / at / up for the world frame and the viewport for [B, N, 3]);
`frame`; `shape` (B, H, W); `upstream` {'normal': fp32 gradient in pos's shape}.  Names are H x W, the smallest shapes
at which each piece can go wrong:
    2x2          both reflected neighbours of a pixel are the same pixel, in both directions
    2x5, 5x2     the same in one direction
    3x5          odd and non-square; recorded through the reference's unbatched function too
    12x16        B = 2
    17x9         B = 3, one camera per view, world frame
    36x48        1728 points: several workgroups, the last one partly empty
The variant `flat` of 12x16 gives the points as [B, N, 3], the shape depth_to_surfels returns.

The points are what depth_to_surfels(frame='camera') makes of depth = 3 + a smooth term + uniform noise of at most 0.05
(tests/surfels_oracle.lift on numpy's pixel grid, in fp64, rounded once to fp32).  With that recipe the reference's own
float32 result stays within the stated tolerance of its float64 one, values and gradients
(test_the_float32_reference_meets_the_stated_tolerance); rougher points bring it closer to that tolerance, which is why
the noise stops at 0.05.

The upstream gradient is uniform in (-1, 1) in steps of 1/64, and the loss of 36x48 leaves rows 10..25 out: both keep
the largest fixture below the largest one of the sibling layers, and the second shows that a centre without an upstream
gradient contributes exactly 0."""
import functools

import numpy as np
import torch

import normals_oracle as no
import projection_cases as pc
import surfels_oracle as so

NAMES = ("2x2", "2x5", "5x2", "3x5", "12x16", "17x9", "36x48")
_SPEC = {  # B, H, W, frame
    "2x2": (1, 2, 2, "camera"), "2x5": (1, 2, 5, "camera"), "5x2": (1, 5, 2, "camera"), "3x5": (1, 3, 5, "camera"),
    "12x16": (2, 12, 16, "camera"), "17x9": (3, 17, 9, "world"), "36x48": (1, 36, 48, "camera"),
}
VARIANTS = ("flat",)
VARIANT_OF = "12x16"
UNBATCHED = "3x5"          # also recorded through estimate_surface_normals_plane_fit
NOISE = 0.05
UNSEEN_ROWS = {"36x48": (10, 26)}     # rows the case's loss leaves out: the gradient is exactly 0 from row 11 to row 24
ALL = [(n, None) for n in NAMES] + [(VARIANT_OF, v) for v in VARIANTS]


def lifted(depth, camera):
    """[B, H, W] depths -> [B, H, W, 3] fp32 camera-space points."""
    B, H, W = depth.shape
    pos = so.lift(torch.as_tensor(np.asarray(depth, dtype=np.float64)), camera, frame="camera")
    return pc.f32(pos.numpy().reshape(B, H, W, 3))


def draw_depth(rng, B, H, W, noise=NOISE):
    """3 + a smooth term + uniform noise of at most `noise`."""
    i, j = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing="ij")
    phase = rng.uniform(0, 2 * np.pi, (B, 2, 1, 1))
    smooth = 0.3 * np.sin(3.0 * i[None] + phase[:, 0]) + 0.2 * np.cos(2.0 * j[None] + phase[:, 1])
    return 3.0 + smooth + rng.uniform(-noise, noise, (B, H, W))


@functools.lru_cache(maxsize=None)
def case(name, variant=None):
    if variant is not None:
        assert variant == "flat", variant
        c = dict(case(VARIANT_OF))
        B, H, W = c["shape"]
        return dict(c, pos=c["pos"].reshape(B, H * W, 3), upstream={"normal": c["upstream"]["normal"].reshape(B, H * W, 3)})
    B, H, W, frame = _SPEC[name]
    rng = np.random.RandomState(9000 + NAMES.index(name))
    eye, at, up = pc.draw_camera(rng, B)
    camera = {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY), "focal_length": pc.FOCAL}
    pos = lifted(draw_depth(rng, B, H, W), camera)
    upstream = np.round(rng.uniform(-1, 1, (B, H, W, 3)) * 64) / 64
    if name in UNSEEN_ROWS:
        upstream[:, slice(*UNSEEN_ROWS[name])] = 0.0
    return {"pos": pos, "camera": camera, "frame": frame, "shape": (B, H, W), "upstream": {"normal": pc.f32(upstream)}}


def tag(name, variant=None):
    return name if variant is None else f"{name}_{variant}"


@functools.lru_cache(maxsize=None)
def expected(name, variant=None):
    """(values {'normal': like pos}, gradients {'pos': like pos}) from the fp64 oracle, computed once."""
    c = case(name, variant)
    return no.gradients({"pos": c["pos"]}, c["camera"], c["upstream"], c["frame"])


@functools.lru_cache(maxsize=None)
def turned(name, variant=None):
    """expected() from the map turned by 180 degrees (normals_oracle.turned_gradients), computed once."""
    c = case(name, variant)
    return no.turned_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], c["frame"], c["shape"])
