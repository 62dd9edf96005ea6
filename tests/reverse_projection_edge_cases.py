"""Deterministic edge inputs for the reverse re-projection (tests/test_hip_reverse_projection_edges.py on the GPU, tests/
test_reverse_projection_edge_cases_cpu.py here, tools/gen_reverse_projection_golden.py for the RECORDED ones): what the
seeded cases of tests/reverse_projection_cases.py never reach.  Same dict layout as reverse_projection_cases; every case
has a rotated image and computes the new depth.  Names are H x W.

    row_1x5, col_5x1  D = 2.  Along the single axis the scale (H - 1) / h is exactly 0 and the coordinate exactly 1/2,
                      which fails the 0.5-pixel frame test: mask = 0 everywhere and out = rotated_image, while image1 is
                      still sampled (weight 1 on the one row or column)
    all_outside_3x5   D = 2.  Every out_pos_wc sample is at least one pixel off the frame: image1 = 0, depth = 0,
                      mask = 0, out = rotated_image; the gradients of rgb and out_pos_wc are exactly 0
    block_16x16       N = 256, one whole workgroup; D = 1
    lane_1x257        N = 257: a second workgroup of one lane; D = 2

Conditions are those of reverse_projection_cases (reverse_projection_oracle.decision_margin >= 1 at depth_epsilon 0.1);
a draw that violates one is redrawn from the next seed of the case's own range."""
import functools

import numpy as np

import reverse_projection_oracle as ro
from projection_cases import draw_camera, f32, jittered_grid, lift
from reverse_projection_cases import CAMERAS

NAMES = ("row_1x5", "col_5x1", "all_outside_3x5", "block_16x16", "lane_1x257")
RECORDED = ("row_1x5", "col_5x1")                       # tests/golden/reverse_projection/rp2_<name>.npz
_SPEC = {  # B, H, W, D
    "row_1x5": (1, 1, 5, 2), "col_5x1": (1, 5, 1, 2), "all_outside_3x5": (1, 3, 5, 2), "block_16x16": (1, 16, 16, 1),
    "lane_1x257": (1, 1, 257, 2),
}


def _draw(name, seed):
    B, H, W, D = _SPEC[name]
    rng = np.random.RandomState(seed)
    N = H * W
    cams = [draw_camera(rng, B) for _ in (0, 1)]
    pos = {}
    for key, k in (("out_pos_wc", 0), ("in_pos_wc", 1)):                 # out_pos is projected by camera1, in_pos by 2
        px, py = jittered_grid(rng, B, H, W, 1.2)
        z = rng.uniform(1.5, 3.0, (B, N))
        if name == "all_outside_3x5" and k == 0:
            side = rng.randint(0, 4, N)
            off = rng.uniform(1.0, 3.0, N)
            px[0] = np.where(side == 0, -off, np.where(side == 1, W + off, px[0]))
            py[0] = np.where(side == 2, -off, np.where(side == 3, H + off, py[0]))
        pos[key] = lift(px, py, z, *cams[k], W, H, *CAMERAS[k])

    def camera(k):
        eye, at, up = cams[k]
        return {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(CAMERAS[k][0]),
                "focal_length": CAMERAS[k][1]}

    case = {"rgb": f32(rng.uniform(0, 1, (B, H, W, D))), "in_pos_wc": f32(pos["in_pos_wc"]),
            "out_pos_wc": f32(pos["out_pos_wc"]), "rotated_image": f32(rng.uniform(0, 1, (B, H, W, D))),
            "camera1": camera(0), "camera2": camera(1), "flags": {"compute_new_depth": True, "depth_epsilon": 0.1},
            "shape": (B, H, W, D), "wrt": ro.INPUTS, "only": None}
    case["upstream"] = {k: f32(rng.uniform(-1, 1, (B, H, W, D if k in ("out", "image1") else 1))) for k in ro.OUTPUTS}
    return case


def margin(c):
    return ro.decision_margin(c["in_pos_wc"], c["out_pos_wc"], c["camera1"], c["camera2"], c["flags"]["depth_epsilon"])


@functools.lru_cache(maxsize=None)
def case(name):
    first = 13500 + 100 * NAMES.index(name)
    for seed in range(first, first + 50):
        c = _draw(name, seed)
        if margin(c) >= 1.0:
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} meets the conditions")


def inputs(c):
    return {k: c[k] for k in ro.INPUTS}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(values, gradients) of a case from the fp64 oracle, computed once."""
    c = case(name)
    return ro.gradients(inputs(c), c["camera1"], c["camera2"], c["upstream"], wrt=c["wrt"], **c["flags"])
