"""Per-entry bounds for the splat renderer (csrc/srh_splat.h) against the fp64 oracle (tests/splat_oracle.py).  The whole
chain is fp64 and rounds to fp32 on the way out, so every figure is derived, except the fp64 floor C64.

  written values   every forward output element; disk.pos, disk.normal; disk.light_vis at K = 1.  One cast:
                     |got - want| <= (2^-24 |want| + C64 scale) (1 + 2^-20)
                   scale = the entry's `absolute` (splat_oracle.gradient_terms) for gradients, max|want| of the array for
                   forward outputs.
  light_vis, K>1   an fp32 read-modify-write chain over the K^2 sub-pixels:  K^2 2^-24 absolute (1 + 2^-20)
  atomic leaves    lights.pos, lights.attenuation, colors, lights.ambient, materials.albedo, materials.coeffs:
                     D 2^-24 absolute (1 + 2^-20),  D = 1 (the cast of the term) + 6 (wave_sum) + adds
                   `adds` = the atomic additions the entry receives, counted from the case alone (add_counts).
An entry whose `absolute` is 0 has bound 0: it must be exactly 0.

Batches (surf_renderer_amd/splats.py), B views:
  colors, lights.attenuation, lights.ambient, materials.*, and lights.pos when shared: the views ADD INTO ONE BUFFER, so
  `adds` is B times the view's (add_counts(views=B)) and `absolute` the sum of the views';
  disk.normal [N, 3] and disk.light_vis [L, N] when shared: each view's value is written as the single call writes it and
  splats.py reduces with g.sum(0): the views' bounds added, plus B - 1 fp32 additions of the sum of |the views' values|
  (shared_written_bound).

C64 is the fp64 chains' own error, the kernels against the oracle (both round, in different orders): measured on an
MI355X as the largest (|got - want| - 2^-24 |want|) / scale over all written entries of all cases
(tests/test_hip_splat_entries.py prints it; profiles/splat_entry_bounds.txt records it), times 4 -- fp64 chains of this
length vary with their operands by about as much.  C64_CAP = 2^-36 is a condition, not a tolerance: about a thousand fp64
roundings amplified by the largest shininess of the cases, 12, give 2^-39.
The measurement reads 0: over the 31 cases no written entry is further from the oracle than one fp32 rounding of the
oracle's value, the largest figure being that of the entries that are 0 on both sides (over the entries with want != 0
it is negative, profiles/splat_entry_bounds.txt).  So C64 = 4 x 0 = 0 and a written entry's bound is the cast alone."""
import numpy as np

import splat_oracle
from grad_cases import entry_bounds

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
C64_CAP = 2.0 ** -36
C64_MEASURED = 0.0           # MI355X: no written entry of any case is further from the oracle than one fp32 rounding
C64_FACTOR = 4
C64 = C64_FACTOR * C64_MEASURED

ATOMIC = ("lights.pos", "colors", "lights.attenuation", "lights.ambient", "materials.albedo", "materials.coeffs")
WRITTEN = ("disk.pos", "disk.normal")


def add_counts(scene, kwargs, views=1):
    """{atomic leaf: the atomic additions each entry receives}, shaped like (or broadcastable to) the leaf, from the case
    alone.  `views`: the views of a batch that add into the same buffer."""
    vp = [int(v) for v in np.asarray(scene["camera"]["viewport"]).reshape(-1)]
    n = (vp[2] - vp[0]) * (vp[3] - vp[1])
    K = int(kwargs.get("samples", 1))
    waves = -(-n // 64)
    cidx, mat = splat_oracle.clamped_color_idx(scene), splat_oracle.material_idx(scene, n)
    L, C, M = len(cidx), len(np.asarray(scene["colors"])), len(np.asarray(scene["materials"]["albedo"]))
    per_light = waves * K * K                                 # wave_add inside the sub-pixel and the light loop
    materials = np.zeros(M)
    for w in range(waves):
        live = mat[64 * w:64 * (w + 1)]
        if np.all(live == live[0]):
            materials[live[0]] += 1                           # one wave_add to the wave's row
        else:
            materials += np.bincount(live, minlength=M)       # one atomicAdd per live lane
    counts = {"lights.pos": np.full((L, 1), per_light), "lights.attenuation": np.full((L, 1), per_light),
              "colors": (per_light * np.bincount(cidx, minlength=C))[:, None],
              "lights.ambient": np.full((1,), waves), "materials.albedo": materials[:, None],
              "materials.coeffs": materials[:, None]}
    return {k: views * v.astype(np.float64) for k, v in counts.items()}


def atomic_bound(absolute, adds):
    """(bound, accumulation part) of an atomic leaf: D 2^-24 absolute (1 + 2^-20) with D = 1 + 6 + adds; the two are the
    same here (eps_term = 0).  grad_cases.entry_bounds counts 9 + atomics, hence adds - 2."""
    return entry_bounds(absolute, np.asarray(adds, dtype=np.float64) - 2.0, 0.0)


def written_bound(want, scale, c64=None):
    c64 = C64 if c64 is None else c64
    return (U * np.abs(np.asarray(want, dtype=np.float64)) + c64 * np.asarray(scale, dtype=np.float64)) * SLACK


def output_bound(want, c64=None):
    want = np.asarray(want, dtype=np.float64)
    return written_bound(want, np.abs(want).max(initial=0.0), c64)


def light_vis_bound(want, absolute, K, c64=None):
    """Written once at K = 1; an fp32 chain of K^2 roundings, in a fixed order, at K > 1."""
    if K == 1:
        return written_bound(want, absolute, c64)
    return K * K * U * np.asarray(absolute, dtype=np.float64) * SLACK


def leaf_bound(key, want, absolute, counts, K, c64=None):
    """The bound of every entry of a leaf of ONE view."""
    if key in ATOMIC:
        return atomic_bound(absolute, counts[key])[0]
    if key == "disk.light_vis":
        return light_vis_bound(want, absolute, K, c64)
    return written_bound(want, absolute, c64)


def shared_written_bound(wants, bounds):
    """disk.normal / disk.light_vis shared by the views of a batch: the views' own bounds, plus the B - 1 fp32 additions of
    g.sum(0), each within 2^-24 of the sum of |the views' values|."""
    B = len(wants)
    return sum(bounds) + (B - 1) * U * sum(np.abs(w) for w in wants) * SLACK


def written_excess(got, want, scale, nonzero=False):
    """The C64 measurement of one array: the largest (|got - want| - 2^-24 |want|) / scale over entries with scale > 0
    (nonzero: and want != 0 -- an entry that is 0 on both sides reads exactly 0)."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), want.shape)
    ok = (scale > 0) & np.isfinite(want) & ((want != 0) | (not nonzero))
    if not ok.any():
        return -np.inf if nonzero else 0.0
    return float(np.max((np.abs(got - want)[ok] - U * np.abs(want[ok])) / scale[ok]))
