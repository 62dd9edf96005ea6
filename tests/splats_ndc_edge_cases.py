"""Deterministic edge inputs for the NDC splat renderer (tests/test_hip_splats_ndc_edges.py on the GPU, tests/
test_splats_ndc_edge_cases_cpu.py here, tools/gen_splats_ndc_golden.py for the recorded ones): the branches that the
seeded cases of tests/splats_ndc_cases.py cannot reach.  Built on splats_ndc_cases._draw, so cameras, lights, colours and
materials are those of the seeded cases; a case is {'name', 'scene', 'kwargs', 'upstream'} as there, plus 'at_kink': the
splats that sit on a kink on purpose.  Every other splat keeps the margins of splats_ndc_cases.margins.

The backward kernel reduces the material gradients per 64-lane wave: one wave_add into the wave's material when every
live lane has the same one (the uniform path), else one atomic per lane.  The seeded material_idx is drawn with
probability 0.4, so every full wave of the seeded cases is mixed.
    uniform_waves    16 x 12, three waves: material 1 on splats 0..63, 0 on 64..127, the seeded mixture on 128..191 -- the
                     uniform path with m0 != 0 over a full wave, next to a divergent wave in the same launch
    uniform_partial  16 x 5, 80 splats: wave 0 all material 1; wave 1 has 16 live lanes, all material 0, whose dead lanes
                     read splat 0 (material 1)
    uniform_b3       the same pattern, B = 3, every per-view leaf with its own view axis
    zero_normals     the committed 3x5 scene with the normals of two splats exactly (0, 0, 0): cam_dir . n and the diffuse
    (_ds, _l1,       dot are exactly 0, and so is the specular dot under double_sided (sgn = sign(0) = 0): sgn == 0,
     _l1_ds)         relu(0), and with the one-light coefficients of 3x5_l1 (exponent 0 for material 0) 0 ** 0 = 1.
                     _ds: double_sided; _l1: the scene of 3x5_l1
The dl > 0 guard of a splat at the origin is left out: sqrt at 0 makes autograd's answer NaN, and the guard's 0 is a
choice the sibling suite (tests/splat_edge_scenes.py) documents.

All of them are RECORDED (tests/golden/splats_ndc/sn2_<name>.npz): the reference accepts every one and returns finite
values and gradients, zero normals included.  The prefix is sn2_ because tests/test_splats_ndc_oracle_cpu.py holds the
sn1_ files to exactly the seeded cases.

abi_scene() is the 5 x 13 scene (65 splats: one workgroup, the second wave with one live lane) of the C ABI tests."""
import copy
import functools

import numpy as np

import splats_ndc_cases as cases
import splats_ndc_oracle as oracle

NAMES = ("uniform_waves", "uniform_partial", "uniform_b3", "zero_normals", "zero_normals_ds", "zero_normals_l1",
         "zero_normals_l1_ds")
RECORDED = NAMES
_GRID = {"uniform_waves": (16, 12, 0), "uniform_partial": (16, 5, 0), "uniform_b3": (16, 5, 3)}      # W, H, B
WAVE = 64


def _draw_grid(W, H, B, seed):
    """splats_ndc_cases._draw for a grid that is not one of its names (its two-light scene, no option)."""
    key = f"edge_{W}x{H}_b{B}"
    cases._SPEC[key] = (W, H, B, {})
    try:
        return cases._draw(key, seed)
    finally:
        del cases._SPEC[key]


def _uniform(name, seed):
    W, H, B = _GRID[name]
    c = _draw_grid(W, H, B, seed)
    mat = c["scene"]["objects"]["disk"]["material_idx"]
    mat[:WAVE] = 1
    mat[WAVE:2 * WAVE] = 0                               # 16 x 5: the 16 live lanes of wave 1
    return dict(c, name=name, at_kink=())


def _zero_normals(name):
    base = cases.case("3x5_l1" if "_l1" in name else "3x5")
    c = {"name": name, "scene": copy.deepcopy(base["scene"]), "upstream": base["upstream"],
         "kwargs": {"double_sided": True} if name.endswith("_ds") else {}}
    disk = c["scene"]["objects"]["disk"]
    mat = np.asarray(disk["material_idx"])
    at = (int(np.flatnonzero(mat == 0)[1]), int(np.flatnonzero(mat == 1)[1]))      # one splat of either material
    disk["normal"][list(at)] = 0.0
    return dict(c, at_kink=at)


def margins(c):
    """splats_ndc_cases.margins over the splats that are not at a kink on purpose: {branch: (smallest |value|, any below
    0, any above 0)}."""
    keep = np.setdiff1d(np.arange(c["scene"]["objects"]["disk"]["pos"].shape[-2]), np.asarray(c["at_kink"], dtype=np.int64))
    out = {}
    for sc in cases.views(c["scene"]):
        for k, v in oracle.decisions(sc, **c["kwargs"]).items():
            v = v[keep]
            lo, neg, pos = out.get(k, (np.inf, False, False))
            out[k] = (min(lo, float(np.abs(v).min())), neg or bool((v < 0).any()), pos or bool((v > 0).any()))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("zero_normals"):
        return _zero_normals(name)
    base = 9000 + 100 * NAMES.index(name)
    for seed in range(base, base + 200):
        c = _uniform(name, seed)
        if all(m[0] >= cases.DRAW_MARGIN for m in margins(c).values()):
            return c
    raise RuntimeError(f"{name}: no draw satisfies the margins")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(outputs, gradients) of the fp64 restatement in the batch's layout, computed once."""
    c = case(name)
    return oracle.batch_gradients(c["scene"], c["upstream"], **c["kwargs"])


@functools.lru_cache(maxsize=None)
def abi_scene():
    """({'scene', 'upstream'}) at 5 x 13 (H x W) for the calls through the C ABI."""
    for seed in range(9900, 10100):
        c = dict(_draw_grid(13, 5, 0, seed), at_kink=())
        if all(m[0] >= cases.DRAW_MARGIN for m in margins(c).values()):
            return c
    raise RuntimeError("abi_scene: no draw satisfies the margins")
