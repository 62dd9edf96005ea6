"""Deterministic edge inputs for the plane-fit layer (tests/test_hip_normals_edges.py on the GPU, tests/
test_normals_edge_cases_cpu.py here): what the seeded cases of tests/normals_cases.py keep away from.  Same dict layout
as normals_cases; `nonzero` is False where the gradient is exactly 0 by construction.

    two_2x3, two_3x2, two_2x2     sides of 2: both reflected neighbours along such a side are the same pixel, so a centre's
                                  stencil lands 2 (and at 2x2 diagonally 4) times on one point
    wide_2x300, tall_300x2        B = 2, 600 points: workgroups of 256 lanes straddle rows, the third is partly empty
    b5_2x2                        five views of 2 x 2: the launch grid is (1, 5)
    constant_4x4                  every point the same: u = 0 in every slot, D = 1e-12 exactly, n = (0, 0, s) with
                                  s = 1 / sqrt(1 + 3e-10), gradient exactly 0
    vertical_plane_5x6            P = (j, j, -i): every (ux, uy) is on the line ux = uy bit for bit, so a = b = d and
                                  a d - b^2 cancels to exactly 0; D = 1e-12, n = (0, 0, s).  The gradient is finite, of
                                  the order 1e12 (two divisions by D), and fixed to the last bit by products of equal
                                  operands -- there is no cancellation between unequal roundings
    duplicates_5x6                lifted points with columns 2 and 4 copies of columns 1 and 3: a zero-length difference,
                                  kept finite by the eps under the square root (u = 0, slope 1 / sqrt(3e-10)).  The
                                  border columns keep three distinct columns in reach, so no fit degenerates
    nan_7x7, inf_7x7, big_7x7     lifted points with the z of the centre point (3, 3) NaN, +inf and 1e30, and a NaN
                                  upstream gradient (z) on the far corner (0, 6).  Normals are non-finite on the centre's
                                  3 x 3 (NaN, inf; none for 1e30), gradients on its 5 x 5 and on the corner's 2 x 2
    world_shared_6x5, world_views_6x5   B = 2 in the world frame: one camera ([3] vectors) for both views, one per view
"""
import functools

import numpy as np

import normals_cases as nc
import normals_oracle as no
import projection_cases as pc

NAMES = ("two_2x3", "two_3x2", "two_2x2", "wide_2x300", "tall_300x2", "b5_2x2", "constant_4x4", "vertical_plane_5x6",
         "duplicates_5x6", "nan_7x7", "inf_7x7", "big_7x7", "world_shared_6x5", "world_views_6x5")
_SPEC = {  # B, H, W, frame
    "two_2x3": (1, 2, 3, "camera"), "two_3x2": (1, 3, 2, "camera"), "two_2x2": (1, 2, 2, "camera"),
    "wide_2x300": (2, 2, 300, "camera"), "tall_300x2": (2, 300, 2, "camera"), "b5_2x2": (5, 2, 2, "camera"),
    "constant_4x4": (1, 4, 4, "camera"), "vertical_plane_5x6": (1, 5, 6, "camera"), "duplicates_5x6": (1, 5, 6, "camera"),
    "nan_7x7": (1, 7, 7, "camera"), "inf_7x7": (1, 7, 7, "camera"), "big_7x7": (1, 7, 7, "camera"),
    "world_shared_6x5": (2, 6, 5, "world"), "world_views_6x5": (2, 6, 5, "world"),
}
SPECIAL = {"nan_7x7": np.nan, "inf_7x7": np.inf, "big_7x7": 1e30}
CENTRE, CORNER = (3, 3), (0, 6)


def reach(point, radius, H=7, W=7):
    """[H, W] bool: the pixels within `radius` of `point` along both axes."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (np.abs(i - point[0]) <= radius) & (np.abs(j - point[1]) <= radius)


@functools.lru_cache(maxsize=None)
def case(name):
    B, H, W, frame = _SPEC[name]
    rng = np.random.RandomState(9100 + NAMES.index(name))
    eye, at, up = pc.draw_camera(rng, B)
    camera = {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY), "focal_length": pc.FOCAL}
    pos = nc.lifted(nc.draw_depth(rng, B, H, W), camera)
    upstream = np.round(rng.uniform(-1, 1, (B, H, W, 3)) * 64) / 64
    nonzero = True
    if name == "constant_4x4":
        pos[:] = pos[0, 1, 2]
        nonzero = False
    elif name == "vertical_plane_5x6":
        i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pos = pc.f32(np.stack((j, j, -i), axis=-1)[None])
    elif name == "duplicates_5x6":
        pos[:, :, 2::2] = pos[:, :, 1:-1:2]
    elif name in SPECIAL:
        pos[0, CENTRE[0], CENTRE[1], 2] = SPECIAL[name]
        upstream[0, CORNER[0], CORNER[1], 2] = np.nan
    elif name == "world_shared_6x5":
        camera = dict(camera, eye=eye[0], at=at[0], up=up[0])
    return {"pos": pos, "camera": camera, "frame": frame, "shape": (B, H, W), "upstream": {"normal": pc.f32(upstream)},
            "nonzero": nonzero}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(values {'normal': like pos}, gradients {'pos': like pos}) from the fp64 oracle, computed once."""
    c = case(name)
    return no.gradients({"pos": c["pos"]}, c["camera"], c["upstream"], c["frame"])


@functools.lru_cache(maxsize=None)
def turned(name):
    """expected() from the map turned by 180 degrees (normals_oracle.turned_gradients), computed once."""
    c = case(name)
    return no.turned_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], c["frame"], c["shape"])
