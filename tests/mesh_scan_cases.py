"""Inputs that put r0 ON the CDF of the mesh sampler -- test infrastructure, numpy only.  tests/mesh_sampling_cases.py
keeps every r0 2^-30 away from every CDF value, so its cases cannot see the last ~20 bits of k_mesh_scan's result, its
tie rule, or whether a zero-weight face owns a sliver of the unit interval.  Two families close that
(tests/test_mesh_scan_cases_cpu.py asserts what is promised of them here):

  EXACT   One axis-aligned right triangle per face in z = 0 with legs (2^a, 2^b) and small integer origins: area2 is the
          single product 2^(a + b), every weight and every partial sum of weights is an integer below 2^53, so EVERY
          association order gives the same sums and cdf[i] = fl(prefix_i / total) whatever the scan's tree.  r0 may then
          sit on a CDF value and one ulp below it and `face` is still known exactly.  Zero-weight faces come in three
          kinds -- a duplicate vertex, the other winding under an eye on +z (the cull), a NaN vertex of its own -- in
          runs over a lane's 4 faces, a wave's 256, a whole tile, the tile seam and the tail, at face counts around the
          tile.  The views come in batches of three with per-view f; the batch's F is that of its largest view, the
          others padded with zero-weight faces, and a view alone keeps its own F.
  RANGED  The same triangles with legs (a, 1), a float32 drawn log-uniformly from 2^-15..2^15: area2 = a is still exact,
          the sums are not (over 2^-10..2^10 they still are: 24-bit terms down to 2^-33 under a total of 2^17 fit
          fp64's 53 bits, and a scan without the running maximum would pass).  About 30 % zero-weight faces.  Its probes are every double within 4 ulp of every exact CDF
          value (fractions.Fraction, rounded once).  A scan that sums F non-negative terms in any fixed order is within
          (F - 1) u relative of the exact prefix, likewise the total, and the division rounds once more: its CDF is
          within TOL = (2 F + 2) 2^-53 of the exact one.  Every positive share weight / total exceeds 2 TOL + 16 2^-53,
          so a probe can only be given to one of the two positive-weight faces around its boundary."""
import functools
from fractions import Fraction

import numpy as np

VIEWS = 3
TILE, WAVE, LANE = 1024, 256, 4            # srh_mesh.h: kMeshScanTile, a wave's share of it, kMeshScanItems
LAST = np.nextafter(1.0, 0.0)
EYE = np.array([0.5, 0.25, 2.0 ** 20])     # on +z: a face wound to face -z is culled
KINDS = ("duplicate", "flipped", "nan")    # of a zero-weight face; kind -1 is a positive-weight face
MAX_EXPONENT = 30                          # exact weights are 2^0 .. 2^30

# (name, F, share of scattered zero-weight faces, dead runs [lo, hi), alive: positive faces only inside [lo, hi))
EXACT = [
    ("f1023_head", 1023, 0.0, [(0, LANE)], None),
    ("f1024_wave", TILE, 0.1, [(WAVE, 2 * WAVE)], None),
    ("f1025_tail", 1025, 0.0, [(1019, 1025)], None),
    ("f2048_seam", 2 * TILE, 0.3, [(0, LANE), (TILE - 4, TILE + 5)], None),
    ("f2049_single", 2049, 0.0, [], (TILE, TILE + 1)),
    ("f2049_tile", 2049, 0.0, [(TILE, 2 * TILE)], None),
    ("f3077_last_tile", 3 * TILE + 5, 0.0, [], (3 * TILE, 3 * TILE + 5)),
    ("f3077_first_tile", 3 * TILE + 5, 0.1, [], (0, TILE)),
    ("f3077_mix", 3 * TILE + 5, 0.3, [(0, LANE), (WAVE, 2 * WAVE), (2 * TILE - 4, 2 * TILE + 5)], None),
]
EXACT_BATCHES = [(0, 1, 2), (3, 4, 5), (6, 7, 8)]
RANGED = [1025, 2053]                      # F of the two ranged batches; three seeds each
RANGED_LOG2 = 15.0                         # legs a in 2^-15 .. 2^15
ULPS = 4


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def tol(n_faces):
    """how far a fixed-order fp64 scan of n_faces weights, divided by its total, can be from the exact CDF"""
    return (2 * n_faces + 2) * 2.0 ** -53


def _triangles(legs, kind):
    """(v [3 F, 3] float32, f [F, 3] int64): face i has its own vertices 3 i .. 3 i + 2, the right angle at a small
    integer origin, legs[i] = (along x, along y), wound to face +z; kind[i] >= 0 makes it a zero-weight face."""
    n = len(legs)
    i = np.arange(n)
    v = np.zeros((n, 3, 3))
    v[:, :, 1] = (i % 5)[:, None]
    v[:, 1, 0] = legs[:, 0]
    v[:, 2, 1] += legs[:, 1]
    f = 3 * i[:, None] + np.arange(3)[None, :]
    f[kind == 0, 1] = f[kind == 0, 0]                                   # a duplicate vertex; 3 i + 1 is unreferenced
    f[kind == 1] = f[kind == 1][:, [0, 2, 1]]                           # wound the other way: culled from +z
    v[kind == 2, 1, 0] = np.nan                                         # a NaN vertex of its own
    v = v.reshape(-1, 3)
    assert np.array_equal(f32(v).astype(np.float64), v, equal_nan=True)   # every coordinate is a float32 as it stands
    return f32(v), f


def _kinds(dead, start=0):
    """the three kinds in turn over the zero-weight faces, -1 elsewhere"""
    kind = np.full(len(dead), -1)
    kind[dead] = (start + np.arange(dead.sum())) % len(KINDS)
    return kind


def exact_mesh(areas):
    """areas [F] of integers, 2^e with 0 <= e <= 30, or 0 for a zero-weight face: (v [3 F, 3] float32, f [F, 3] int64,
    kind [F]).  A zero-weight face of the flipped or the NaN kind keeps legs of its own (2^7, 2^8), so that a cull or a
    NaN test that fails adds weight."""
    areas = np.asarray(areas, np.int64)
    dead = areas == 0
    e = np.where(dead, 15, np.round(np.log2(np.where(dead, 1, areas)))).astype(np.int64)
    assert (np.where(dead, 0, 2 ** e) == areas).all() and e.max() <= MAX_EXPONENT
    legs = np.stack([2.0 ** (e // 2), 2.0 ** (e - e // 2)], axis=1)
    kind = _kinds(dead)
    return _triangles(legs, kind) + (kind,)


def exact_cdf(weight):
    """[F] float64: integer prefix sums in Python integers, one correctly rounded division each"""
    w = [int(x) for x in weight]
    assert all(float(a) == b for a, b in zip(w, weight)) and min(w) >= 0
    total, run, out = sum(w), 0, []
    assert 0 < total < 2 ** 53
    for a in w:
        run += a
        out.append(run / total)                                         # int / int is correctly rounded
    return np.array(out)


def fraction_cdf(weight):
    """[F] float64 of any finite non-negative weights: exact rational prefix sums over the exact total, rounded once"""
    w = [Fraction(float(x)) for x in weight]
    total, run, out = sum(w), Fraction(0), []
    for a in w:
        run += a
        out.append(float(run / total))                                  # Fraction.__float__ rounds once
    return np.array(out)


def _uniforms(r0, seed):
    rng = np.random.RandomState(seed)
    r0 = np.asarray(r0, np.float64)
    assert (r0 >= 0).all() and (r0 < 1).all()
    return np.concatenate([r0[:, None], rng.rand(len(r0), 2)], axis=1)


def boundary_probes(cdf, weight, seed=0):
    """uniforms [S, 3]: r0 = 0, nextafter(1, 0), every distinct CDF value below 1 and the double just below each (0
    stays 0); s and t seeded.  r0 = 1 is refused by the layer and is not among them."""
    assert len(cdf) == len(weight)
    values = np.unique(cdf[cdf < 1.0])
    return _uniforms(np.concatenate([[0.0, LAST], values, np.nextafter(values, 0.0)]), seed)


def ulp_probes(cdf, seed=0, ulps=ULPS):
    """uniforms [S, 3]: r0 = every double within `ulps` of every distinct CDF value, inside [0, 1), and 0 and
    nextafter(1, 0)"""
    values = np.unique(cdf)
    near = [values]
    up, down = values, values
    for _ in range(ulps):
        up, down = np.nextafter(up, 2.0), np.nextafter(down, -1.0)
        near += [up, down]
    r0 = np.concatenate(near + [[0.0, LAST]])
    return _uniforms(np.unique(r0[(r0 >= 0) & (r0 < 1)]), seed)


def ranged_mesh(n_faces, seed):
    """(v [3 F, 3] float32, f [F, 3] int64, kind [F]): legs (a, 1) with a float32 a log-uniform over 2^-15..2^15, about
    30 % zero-weight faces of the three kinds, one of them at an index that starts a lane's four"""
    rng = np.random.RandomState(seed)
    a = f32(2.0 ** rng.uniform(-RANGED_LOG2, RANGED_LOG2, n_faces)).astype(np.float64)
    dead = rng.uniform(size=n_faces) < 0.3
    dead[LANE * (1 + rng.randint(n_faces // LANE - 1))] = True
    dead[[0, n_faces - 1]] = False
    kind = _kinds(dead, seed)
    return _triangles(np.stack([a, np.ones(n_faces)], axis=1), kind) + (kind,)


def upstreams(shape, seed):
    """g_pos, g_normal float32 with 0.25 <= |g| < 1: no zero, so a zero gradient is the layer's"""
    rng = np.random.RandomState(88000 + seed)
    return [f32(rng.uniform(0.25, 1, shape) * rng.choice([-1, 1], shape)) for _ in range(2)]


def _exact_areas(k):
    name, n, share, runs, alive = EXACT[k]
    rng = np.random.RandomState(4100 + k)
    e = rng.randint(0, MAX_EXPONENT + 1, n)
    dead = rng.uniform(size=n) < share
    for lo, hi in runs:
        dead[lo:hi] = True
        dead[[i for i in (lo - 1, hi) if 0 <= i < n]] = False           # the run ends where it says
    if alive is not None:
        dead[:alive[0]] = True
        dead[alive[1]:] = True
        dead[[alive[0], alive[1] - 1]] = False
    live = np.flatnonzero(~dead)
    if len(live) >= 2:                                                  # the whole range of 2^30 in every such view
        e[live[len(live) // 3]], e[live[2 * len(live) // 3]] = 0, MAX_EXPONENT
    return np.where(dead, 0, 2 ** e.astype(np.int64))


def _pad(v, f, kind, n_faces):
    """the view with zero-weight faces of the three kinds behind it, up to n_faces"""
    extra = n_faces - len(f)
    if extra == 0:
        return v, f, kind
    pk = _kinds(np.ones(extra, bool), len(f))
    pv, pf = _triangles(np.full((extra, 2), 2.0 ** 6), pk)
    return np.concatenate([v, pv]), np.concatenate([f, pf + len(v)]), np.concatenate([kind, pk])


def _cycled(u, n):
    return u[np.arange(n) % len(u)]


def _frozen(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _batch(names, meshes, weights, cdfs, probes, seed):
    """pads three views (v, f, kind) to one F and their probes to one S (by repeating them in turn)"""
    n_faces, n_samples = max(len(m[1]) for m in meshes), max(len(u) for u in probes)
    padded = [_pad(*m, n_faces) for m in meshes]
    g_pos, g_normal = upstreams((VIEWS, n_samples, 3), seed)
    return _frozen({
        "names": names, "v": np.stack([p[0] for p in padded]), "f": np.stack([p[1] for p in padded]),
        "kind": np.stack([p[2] for p in padded]), "eye": EYE.copy(), "own_faces": np.array([len(m[1]) for m in meshes]),
        "weight": np.stack([np.concatenate([w, np.zeros(n_faces - len(w))]) for w in weights]),
        "cdf": np.stack([np.concatenate([c, np.ones(n_faces - len(c))]) for c in cdfs]),
        "uniforms": np.stack([_cycled(u, n_samples) for u in probes]), "g_pos": g_pos, "g_normal": g_normal})


@functools.lru_cache(maxsize=None)
def exact_batch(j):
    """Batch j of the exact views: {names, v [3, 3 F, 3] float32, f [3, F, 3] int64, kind [3, F], eye [3], own_faces [3]
    (F of each view before the padding), weight [3, F] (integers), cdf [3, F] (exact), uniforms [3, S, 3] (boundary
    probes, repeated in turn up to the batch's S), g_pos, g_normal [3, S, 3] float32}.  Read-only: it is cached."""
    names, meshes, weights, cdfs, probes = [], [], [], [], []
    for k in EXACT_BATCHES[j]:
        areas = _exact_areas(k)
        names.append(EXACT[k][0])
        meshes.append(exact_mesh(areas))
        weights.append(areas.astype(np.float64))
        cdfs.append(exact_cdf(weights[-1]))
        probes.append(boundary_probes(cdfs[-1], weights[-1], 5200 + k))
    return _batch(names, meshes, weights, cdfs, probes, 10 + j)


@functools.lru_cache(maxsize=None)
def ranged_batch(j):
    """Batch j of the ranged views, laid out as exact_batch's: F = RANGED[j] for all three, weight = the float32 legs,
    cdf = fraction_cdf(weight), uniforms = ulp_probes.  Read-only: it is cached."""
    n = RANGED[j]
    names, meshes, weights, cdfs, probes = [], [], [], [], []
    for b in range(VIEWS):
        v, f, kind = ranged_mesh(n, 6300 + 10 * j + b)
        names.append("ranged_f%d_%d" % (n, b))
        meshes.append((v, f, kind))
        weights.append(np.where(kind < 0, v[f[:, 1], 0].astype(np.float64), 0.0))
        cdfs.append(fraction_cdf(weights[-1]))
        probes.append(ulp_probes(cdfs[-1], 7400 + 10 * j + b))
    return _batch(names, meshes, weights, cdfs, probes, 20 + j)


def dead_view_batch():
    """a view without a positive weight (the three kinds in turn) between the two exact views of 2049 faces"""
    c = exact_batch(1)
    assert list(c["own_faces"][1:]) == [2049, 2049]
    out = {k: (np.array(a) if isinstance(a, np.ndarray) else a) for k, a in c.items()}
    kind = _kinds(np.ones(2049, bool))
    v, f = _triangles(np.full((2049, 2), 2.0 ** 6), kind)
    for k, a in (("v", v), ("f", f), ("kind", kind), ("weight", np.zeros(2049)), ("cdf", np.zeros(2049))):
        out[k][0] = a
    order = [1, 0, 2]                                                   # exact, dead, exact
    for k in ("v", "f", "kind", "weight", "cdf", "uniforms", "g_pos", "g_normal", "own_faces"):
        out[k] = out[k][order]
    out["names"] = [c["names"][1], "f2049_all_dead", c["names"][2]]
    return out


def expected_faces(cdf, r0):
    """numpy's choice(p=...): the number of CDF values <= r0"""
    return np.searchsorted(cdf, r0, side="right").astype(np.int64)


def acceptable_bounds(cdf, weight):
    """(live, lo, hi): the positive-weight faces and the exact interval [lo, hi) of r0 that selects each"""
    live = np.flatnonzero(np.asarray(weight) > 0)
    hi = cdf[live]
    return live, np.concatenate([[0.0], hi[:-1]]), hi
