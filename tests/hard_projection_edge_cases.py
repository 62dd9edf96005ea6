"""Deterministic edge inputs for the hard projection (tests/test_hip_hard_projection_edges.py on the GPU, tests/
test_hard_projection_edge_cases_cpu.py here, tools/gen_hard_projection_golden.py for the two RECORDED ones): what the
seeded cases of tests/hard_projection_cases.py are redrawn to avoid.  Same dict layout as hard_projection_cases; `named`
holds the indices of the surfels a case places by hand.

The exact cases look down the axis: eye (0, 0, 0), at (0, 0, -1), up (0, 1, 0), so a surfel with x = 0 has camera X
exactly 0 and lands on u = W / 2 - 1 / 2 whatever its depth -- a rounding TIE when W is even (likewise y and H).

    tie_4x6, tie_6x4   (H x W, D = 3; recorded)  surfels 0..2 on the axis at Z < 0, Z > 0 and Z = 0 (both coordinates
                       tie), 3 with only x = 0 (u ties), 4 with only y = 0 (v ties).  4x6: u = 2.5 and v = 1.5 round to
                       the even 2 and 2, index 14; 6x4: u = 1.5, v = 2.5, index 10 -- one side ties downwards, the other
                       upwards.  The rest is the usual jittered draw, clear of every kink
    edges_5x7          surfels 0..7 land in the border pixels from OUTSIDE the span of the pixel centres: u in
                       (-0.5, 0) (rint gives -0.0) and in (W - 1, W - 0.5), likewise v; two per band
    nonfinite_4x6      surfels 0..7 hold NaN, +-inf, 1e30 and 3e38 components: all dropped.  Surfel 0 also carries NaN
                       rgb, and the upstream gradient is NaN on two pixels nothing lands on: no result may depend on them
    all_dropped_3x5    every surfel is off the frame, a third of them behind the camera as well: nothing but dropped keys
    all_dropped_b2     B = 2: view 0 all dropped, view 1 ordinary
    cluster_last_8x8   all 64 surfels in pixel N - 1: the run ends with the ordered list, not with another key
    cluster_first_8x8  all 64 in pixel 0
"""
import functools

import numpy as np
import torch

import hard_projection_oracle as ho
import projection_cases as pc
import projection_oracle as po

NAMES = ("tie_4x6", "tie_6x4", "edges_5x7", "nonfinite_4x6", "all_dropped_3x5", "all_dropped_b2", "cluster_last_8x8",
         "cluster_first_8x8")
RECORDED = ("tie_4x6", "tie_6x4")          # tests/golden/hard_projection/hp2_<name>.npz
_SPEC = {  # B, H, W, D, axis camera
    "tie_4x6": (1, 4, 6, 3, True), "tie_6x4": (1, 6, 4, 3, True), "edges_5x7": (1, 5, 7, 3, False),
    "nonfinite_4x6": (1, 4, 6, 3, True), "all_dropped_3x5": (1, 3, 5, 2, False), "all_dropped_b2": (2, 3, 5, 2, False),
    "cluster_last_8x8": (1, 8, 8, 3, False), "cluster_first_8x8": (1, 8, 8, 3, False),
}
TIE_BOTH, TIE_U, TIE_V = (0, 1, 2), (3,), (4,)
NONFINITE_UPSTREAM = (0, 23)               # the pixels of nonfinite_4x6 whose upstream gradient is NaN


def pixels(c):
    """[B, N, 3] fp64: the pixel coordinates (and -Z) of a case's surfels."""
    return po.pixel_coordinates(torch.as_tensor(c["surfels"].astype(np.float64)), c["camera"]).numpy()


def margin(c, skip=()):
    """hard_projection_oracle.kink_margin over the surfels not in `skip` (those deliberately at a kink)."""
    keep = np.setdiff1d(np.arange(c["surfels"].shape[1]), np.asarray(skip, dtype=np.int64))
    return ho.kink_margin(c["surfels"][:, keep], c["camera"])


def _draw(name, seed):
    B, H, W, D, axis = _SPEC[name]
    rng = np.random.RandomState(seed)
    N = H * W
    if axis:
        eye, at, up = pc.f32([[0, 0, 0]]), pc.f32([[0, 0, -1]]), pc.f32([[0, 1, 0]])
    else:
        eye, at, up = pc.draw_camera(rng, B)
    px, py = pc.jittered_grid(rng, B, H, W, 1.2)
    z = rng.uniform(1.5, 3.0, (B, N))
    named = ()
    if name.startswith("tie"):                             # the coordinate of 3 and 4 that does not tie: inside the frame
        py[0, 3], px[0, 4] = rng.uniform(1.1, H - 1.1), rng.uniform(1.1, W - 1.1)
    if name == "edges_5x7":
        named = tuple(range(8))
        px[0, 0:2], px[0, 2:4] = rng.uniform(0.05, 0.45, 2), W - rng.uniform(0.05, 0.45, 2)    # u = px - 1/2
        py[0, 4:6], py[0, 6:8] = rng.uniform(0.05, 0.45, 2), H - rng.uniform(0.05, 0.45, 2)
        px[0, 4:8], py[0, 0:4] = rng.uniform(1.1, W - 1.1, 4), rng.uniform(1.1, H - 1.1, 4)
    if name.startswith("all_dropped"):
        side = rng.randint(0, 4, N)
        off = rng.uniform(1.0, 3.0, N)
        px[0] = np.where(side == 0, -off, np.where(side == 1, W + off, px[0]))
        py[0] = np.where(side == 2, -off, np.where(side == 3, H + off, py[0]))
        z[0, ::3] = -rng.uniform(0.5, 1.5, len(z[0, ::3]))                                      # and behind the camera
    if name == "cluster_last_8x8":
        px, py = W - 1 + rng.uniform(0.1, 0.9, (B, N)), H - 1 + rng.uniform(0.1, 0.9, (B, N))
    if name == "cluster_first_8x8":
        px, py = rng.uniform(0.1, 0.9, (B, N)), rng.uniform(0.1, 0.9, (B, N))
    surfels = pc.f32(pc.lift(px, py, z, eye, at, up, W, H))
    rgb = pc.f32(rng.uniform(0, 1, (B, H, W, D)))
    upstream = pc.f32(rng.uniform(-1, 1, (B, H, W, D)))
    if name.startswith("tie"):
        named = TIE_BOTH + TIE_U + TIE_V
        surfels[0, 0], surfels[0, 1], surfels[0, 2] = (0, 0, -2), (0, 0, 3), (0, 0, 0)
        surfels[0, 3, 0] = 0.0
        surfels[0, 4, 1] = 0.0
    if name == "nonfinite_4x6":
        named = tuple(range(8))
        nan, inf = np.nan, np.inf
        surfels[0, :8] = [(nan, 0, -2), (0.1, inf, -2), (-inf, 0.1, -2), (0.1, 0.1, nan), (0.1, 0.1, inf),
                          (1e30, 0.1, -2), (0.1, -3e38, -2), (3e38, 3e38, -1e-30)]
        rgb[0].reshape(N, D)[0] = nan
    return {"surfels": surfels, "rgb": rgb, "named": named,
            "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY),
                       "focal_length": pc.FOCAL},
            "shape": (B, H, W, D), "upstream": {"out": upstream}}


def _fits(name, c):
    """What a draw must satisfy beyond its construction: every surfel that is not at a kink on purpose is clear of every
    kink, and the NaN upstream gradients of nonfinite_4x6 sit on pixels nothing lands on."""
    skip = c["named"] if name.startswith(("tie", "nonfinite")) else ()
    if margin(c, skip) < 1.0:
        return False
    if name.startswith("tie"):                             # the coordinate of 3 and 4 that does not tie is clear as well
        p = pixels(c)[0]
        free = np.array([p[3, 1], p[4, 0]])
        if np.abs(free - np.round(free)).min() < 1e-4 or np.abs(p[[3, 4], 2]).min() < 1e-3:
            return False
    if name == "nonfinite_4x6":
        idx, _ = ho.pixel_index(torch.as_tensor(c["surfels"].astype(np.float64)), c["camera"])
        if np.isin(NONFINITE_UPSTREAM, idx.numpy()).any():
            return False
    return True


@functools.lru_cache(maxsize=None)
def case(name):
    for seed in range(5800 + 100 * NAMES.index(name), 5800 + 100 * NAMES.index(name) + 50):
        c = _draw(name, seed)
        if _fits(name, c):
            if name == "nonfinite_4x6":
                B, H, W, D = c["shape"]
                c["upstream"]["out"].reshape(H * W, D)[list(NONFINITE_UPSTREAM)] = np.nan
            c["seed"] = seed
            return c
    raise RuntimeError(f"no draw of {name} fits")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(values {'out', 'mask', 'count', 'index'}, gradients {'rgb'}) from the fp64 oracle, computed once."""
    c = case(name)
    return ho.gradients({"surfels": c["surfels"], "rgb": c["rgb"]}, c["camera"], c["upstream"])
