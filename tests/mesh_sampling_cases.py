"""Seeded inputs of the mesh-sampling tests -- test infrastructure.  REGULAR cases are comparable with the reference and
have fixtures under tests/golden/mesh_sampling; their conditions (tests/test_mesh_sampling_cases_cpu.py asserts them):

  - every r0 is at least 2^-30 away from every CDF value, for numpy's CDF and for a plain left-to-right prefix sum: a
    correct scan in any fixed order is within about F 2^-52 of either, so `face` must equal the oracle's exactly.  The
    generator steps a view's seed until this holds;
  - with a camera |n . cam_dir| >= 1e-6 on every face, so the cull is the oracle's;
  - no face is a sliver: sum |cross-product terms| / |c| <= 2^10, so that the normal's bound is its store's half ulp;
  - every case with more than one face hits at least two faces in every view.
r0 ON the CDF -- its values, the doubles around them, the tie rule and zero-weight runs over a lane, a wave and a tile
-- is what this gap leaves out: tests/mesh_scan_cases.py and tests/test_hip_mesh_sampling_scan.py cover it.

Every case has three views with different vertices.  The shapes sit at the seams of srh_mesh.h: a wave's width in
faces (63, 64, 65), a wave's share of a scan tile (256 + 1), the tile (1024 + 1), several tiles (the bunny), and sample
counts around a workgroup (257, 1300, 2000).  EDGE inputs are built in tests/test_hip_mesh_sampling_edges.py from the
helpers here and checked against tests/mesh_sampling_oracle.py alone: the reference raises or gives NaN on them."""
import functools
import hashlib
import os

import numpy as np

import mesh_sampling_oracle as oracle

VIEWS = 3
SCAN_TILE, SCAN_WAVE = 1024, 256           # srh_mesh.h: kMeshScanTile, and a wave's kMeshScanItems * 64 faces of it
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets", "data")
GAP = 2.0 ** -30

# (name, mesh, F, S, f per view, eye: None | "shared" | "per_view")
REGULAR = [
    ("f1_s1", "grid", 1, 1, False, None),
    ("f2_s5_eye", "grid", 2, 5, False, "shared"),
    ("cube_s257", "cube", 12, 257, False, None),
    ("cube_s257_eyes", "cube", 12, 257, False, "per_view"),
    ("f63_s65_fviews", "grid", 63, 65, True, None),
    ("f64_s65_eye", "grid", 64, 65, False, "shared"),
    ("f65_s65_fviews_eyes", "grid", 65, 65, True, "per_view"),
    ("f%d_s300" % (SCAN_WAVE + 1), "grid", SCAN_WAVE + 1, 300, False, None),
    ("f%d_s1300_eyes" % (SCAN_TILE + 1), "grid", SCAN_TILE + 1, 1300, False, "per_view"),
    ("bunny_s2000_eyes", "bunny", 4968, 2000, False, "per_view"),
]


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def tag(k):
    return REGULAR[k][0]


@functools.lru_cache(maxsize=None)
def load_obj(name):
    """(v [V, 3] float64, f [F, 3] int64) of assets/data/<name>.obj: its `v` and `f` lines, 1-based `a/b/c` corners"""
    v, f = [], []
    with open(os.path.join(ASSETS, name + ".obj")) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p and p[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.asarray(v, np.float64), np.asarray(f, np.int64)


def grid_mesh(n_faces, rng, flip=0.0):
    """The first n_faces triangles of a jittered height field over a square grid, wound to face +z, a share `flip` of
    them wound the other way; only the referenced vertices are kept: (v [V, 3] float64, f [F, 3] int64)."""
    n = max(1, int(np.ceil(np.sqrt(n_faces / 2.0))))
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    xy = np.stack([ii, jj], -1).reshape(-1, 2) + rng.uniform(-0.25, 0.25, ((n + 1) ** 2, 2))
    z = 0.4 * np.sin(0.9 * xy[:, 0]) * np.cos(0.7 * xy[:, 1]) + rng.uniform(-0.15, 0.15, len(xy))
    v = np.concatenate([xy, z[:, None]], axis=1) / n
    at = lambda i, j: i * (n + 1) + j                                  # noqa: E731
    f = []
    for i in range(n):
        for j in range(n):
            f += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    f = np.asarray(f[:n_faces], np.int64)
    used = np.unique(f)
    f = np.searchsorted(used, f)
    turn = rng.uniform(size=len(f)) < flip
    f[turn] = f[turn][:, ::-1]
    return v[used], f


def _moved(v, rng):
    """a view's copy of an asset's vertices: rotated a little about z, scaled and shifted"""
    a, s = rng.uniform(-0.4, 0.4), rng.uniform(0.8, 1.25)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return s * v @ rot.T + rng.uniform(-0.3, 0.3, 3)


def gap_to(cdf, r0):
    """the smallest |r0 - cdf value| over all pairs"""
    at = np.searchsorted(cdf, r0)
    below, above = cdf[np.clip(at - 1, 0, len(cdf) - 1)], cdf[np.clip(at, 0, len(cdf) - 1)]
    return float(np.minimum(np.abs(r0 - below), np.abs(r0 - above)).min())


def draw(seed, n_samples):
    """[S, 3] = (r0, s, t) in the reference's order of consumption after np.random.seed(seed)"""
    rng = np.random.RandomState(seed)
    r0 = rng.random_sample(n_samples)
    return np.concatenate([r0[:, None], rng.rand(n_samples, 2)], axis=1)


def seeded_uniforms(weight, n_samples, seed):
    """(uniforms, seed): the first seed at or after `seed`, in steps of 1, whose r0 keep GAP from both CDFs"""
    cdfs = (oracle.cdf_numpy(weight), oracle.cdf_plain(weight))
    for step in range(1000):
        u = draw(seed + step, n_samples)
        if min(gap_to(c, u[:, 0]) for c in cdfs) >= GAP:
            return u, seed + step
    raise AssertionError("no seed keeps r0 away from the CDF")


@functools.lru_cache(maxsize=None)
def regular(k):
    """Case k: {name, v [3, V, 3] float32, f [F, 3] or [3, F, 3] int64, eye None | [3] | [3, 3] float64,
    uniforms [3, S, 3] float64, seeds [3], g_pos, g_normal [3, S, 3] float32 in (-1, 1)}.  Read-only: it is cached."""
    name, mesh, F, S, f_views, eye_kind = REGULAR[k]
    vs, fs = [], []
    for b in range(VIEWS):
        rng = np.random.RandomState(1000 * k + b)
        if mesh == "grid":
            # one connectivity for the case unless it is per view; the vertices differ per view either way
            frng = np.random.RandomState(500 + 1000 * k + (b if f_views else 0))
            flip = 0.3 if (eye_kind and F > 2) else 0.0
            v, f = grid_mesh(F, frng, flip)
            v = _moved(v + rng.uniform(-0.02, 0.02, v.shape) / max(1.0, np.sqrt(F / 2.0)), rng)
            if f_views:
                f = f[np.random.RandomState(900 + 1000 * k + b).permutation(F)]
        else:
            v, f = load_obj(mesh)
            v = _moved(v / np.abs(v).max(), rng)
        vs.append(f32(v))
        fs.append(f)
    v = np.stack(vs)
    f = np.stack(fs) if f_views else fs[0]
    eye = None
    if eye_kind:
        centre = v.reshape(-1, 3).astype(np.float64).mean(0)
        rng = np.random.RandomState(300 + k)
        if mesh == "grid":                                           # above the height field
            eyes = centre + np.array([0.0, 0.0, 4.0]) + rng.uniform(-0.5, 0.5, (VIEWS, 3))
        else:                                                        # around the object
            d = rng.standard_normal((VIEWS, 3))
            eyes = centre + 4.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
        eye = eyes if eye_kind == "per_view" else eyes[0]
    uniforms, seeds = [], []
    for b in range(VIEWS):
        q = oracle.face_quantities(v[b], f[b] if f_views else f, view_eye(eye, b))
        u, seed = seeded_uniforms(q["weight"], S, 7000 + 100 * k + 10 * b)
        uniforms.append(u)
        seeds.append(seed)
    rng = np.random.RandomState(77000 + k)
    out = {"name": name, "v": v, "f": f, "eye": eye, "uniforms": np.stack(uniforms), "seeds": np.asarray(seeds),
           "g_pos": f32(rng.uniform(-1, 1, (VIEWS, S, 3))), "g_normal": f32(rng.uniform(-1, 1, (VIEWS, S, 3)))}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def view_eye(eye, b):
    return None if eye is None else (eye if np.ndim(eye) == 1 else eye[b])


def view_faces(f, b):
    return f if np.ndim(f) == 2 else f[b]


def view_of(c, b):
    """(v, f, uniforms, eye) of view b of a case"""
    return c["v"][b], view_faces(c["f"], b), c["uniforms"][b], view_eye(c["eye"], b)


def checksum(c):
    h = hashlib.sha256()
    for k in ("v", "f", "eye", "uniforms", "g_pos", "g_normal"):
        if c[k] is not None:
            a = np.ascontiguousarray(c[k])
            h.update(k.encode() + str(a.shape).encode() + str(a.dtype).encode() + a.tobytes())
    return h.hexdigest()[:16]
