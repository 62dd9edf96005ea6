"""Seeded inputs for the regulariser tests (tests/test_hip_regularizers.py on the GPU, tests/
test_regularizer_oracle_cpu.py here) and for tools/gen_regularizer_golden.py, which records the reference on some of them.

A case is a dict: the four fp32-representable inputs (with the view axis unless `single`), z_min / z_max / z_scale /
unit_normal_scale, the upstream weights (B, 7) in TERMS order, and `flat` (H, W) bool or None marking the deliberately
degenerate pixels.  Shapes are H x W, the smallest at which the kernels can still go wrong:
    2x2           every neighbour is a reflection, multiplicity 2 on both axes
    3x5, 5x3      one interior row / column, non-square
    17x9_b3       one pixel past a 16-wide tile, three views with distinct weights
    9x17          one pixel past a 16-wide row
    70x33_b2      several 256-pixel workgroups per view, ragged last workgroup, rows that straddle workgroups
    36x48         the size of the largest recorded fixture (p1's)
    flat_patch    a 4 x 4 block with image exactly 0 and constant depth (sign(0) = 0), p_z exactly at z_min (relu'(0) =
                  0) and strictly inside [z_min, z_max]
    near_flat     a cloud within 1e-4 of (1, -2, -3): cancellation in the variance
    zero_weights  some upstream weights exactly 0
    single        one view without the leading axis

Kink condition: outside the flat pixels no decision quantity (regularizer_oracle.decision_margin) is within MARGIN of
zero in fp64; a draw that violates it is redrawn from the next seed.  tests/test_regularizer_oracle_cpu.py asserts it
for every case, so the GPU comparison leaves no element out."""
import functools

import numpy as np
import torch

import regularizer_oracle as ro

MARGIN = 1e-9
NAMES = ("2x2", "3x5", "5x3", "17x9_b3", "9x17", "70x33_b2", "36x48", "flat_patch", "near_flat", "zero_weights", "single")
_SHAPES = {"2x2": (1, 2, 2), "3x5": (1, 3, 5), "5x3": (1, 5, 3), "17x9_b3": (3, 17, 9), "9x17": (1, 9, 17),
           "70x33_b2": (2, 70, 33), "36x48": (1, 36, 48), "flat_patch": (1, 12, 10), "near_flat": (1, 16, 12),
           "zero_weights": (2, 5, 7), "single": (1, 6, 5)}


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _draw(name, seed):
    B, H, W = _SHAPES[name]
    rng = np.random.RandomState(seed)
    pos = np.stack([rng.uniform(-1, 1, (B, H, W)), rng.uniform(-1, 1, (B, H, W)), -rng.uniform(1.5, 4.5, (B, H, W))], -1)
    case = {"normal": _f32(rng.uniform(-1, 1, (B, H, W, 3))), "image": _f32(rng.uniform(0, 1, (B, H, W, 3))),
            "depth": _f32(rng.uniform(1, 5, (B, H, W))), "z_min": 2.0, "z_max": 4.0, "z_scale": 2.0,
            "unit_normal_scale": 10.0, "flat": None, "single": name == "single"}
    weights = rng.uniform(0.5, 2.0, (B, 7)) * rng.choice([-1.0, 1.0], (B, 7))
    if name == "near_flat":
        # distinct multiples of 2^-22 (fp32's spacing at 3) per component: no two pixels share a coordinate
        steps = np.stack([rng.permutation(800)[:B * H * W] - 400 for _ in range(3)], -1).reshape(B, H, W, 3)
        pos = np.array([1.0, -2.0, -3.0]) + steps * 2.0 ** -22
        case.update(z_min=2.5, z_max=3.00005, z_scale=10.0)
    if name == "flat_patch":
        flat = np.zeros((H, W), dtype=bool)
        flat[3:7, 2:6] = True
        case["image"][0, flat] = 0.0
        case["depth"][0, flat] = 2.25
        pos[0, 1, 1:4, 2] = -2.0                          # |p_z| exactly z_min
        pos[0, 9, 5:8, 2] = -4.0                          # |p_z| exactly z_max
        pos[0, 10, 1:6, 2] = [-2.25, -2.75, -3.0, -3.25, -3.75]      # strictly inside
        flat[1, 1:4] = flat[9, 5:8] = True
        case["flat"] = flat
    if name == "zero_weights":
        weights[0, [1, 3, 6]] = 0.0
        weights[1, [0, 2, 4, 5]] = 0.0
    case["pos"] = _f32(pos)
    case["weights"] = _f32(weights)
    return case


def margins(case):
    """decision_margin of every view of a case."""
    x = {k: torch.tensor(np.asarray(case[k], dtype=np.float64)) for k in ro.INPUTS}
    return [ro.decision_margin(*(x[k][b] for k in ro.INPUTS), case["z_min"], case["z_max"], flat=case["flat"])
            for b in range(x["depth"].shape[0])]


@functools.lru_cache(maxsize=None)
def case(name):
    for seed in range(1000 * NAMES.index(name), 1000 * NAMES.index(name) + 50):
        c = _draw(name, seed)
        if min(margins(c)) >= MARGIN:
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} keeps {MARGIN} clear of every kink")


def inputs(c):
    """The four inputs as the public call takes them: without the view axis for a `single` case."""
    return {k: (c[k][0] if c["single"] else c[k]) for k in ro.INPUTS}


@functools.lru_cache(maxsize=None)
def expected(name, wrt=ro.INPUTS):
    """(values {term: (B,)}, gradients {input: (B, ...)}) of a case from the fp64 oracle, computed once."""
    c = case(name)
    return ro.gradients({k: c[k] for k in ro.INPUTS}, c["weights"], c["z_min"], c["z_max"], c["z_scale"],
                        c["unit_normal_scale"], wrt=wrt)
