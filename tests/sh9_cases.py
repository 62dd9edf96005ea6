"""Seeded inputs of the SH9 lighting tests -- test infrastructure.  Every array is float32 (the values the kernels compute
on); tests/test_sh9_cases_cpu.py pins them by hash, tools/gen_sh_lighting_golden.py records the reference on them under
tests/golden/sh_lighting.

Projection cases, (H, W, C, views): probe values uniform in [0, 2], so that the coefficients of order >= 1 cancel
heavily and only a bound relative to the sum of |terms| means anything.  The shapes: even and square with the r = 0
pixel (16), the swapped-axis quirk (12 x 20), an odd side with one channel (15), fewer pixels inside the disc than a
wave with three views and four channels (5), seven workgroups per view (40), and the probe whose one pixel lies outside
(1 x 1, L exactly 0).  ORACLE_ONLY: 73 workgroups per view, more than the finish kernel's 64 rows, so the rows wrap.

Irradiance cases, (N, C, kind of M, M per view): N at one normal, around a wave (63, 64), past a workgroup (257) and
past four (1025); M made by RealSH9_ZonalMatrix from random coefficients, or a random non-symmetric matrix; one M per
view or one shared.  Three views.  In every view the even rows are unit normals and the odd rows are not normalised
(lengths 0.2 .. 3); the last row of the last view is exactly zero, where E = M[3, 3].  ORACLE_ONLY_N: 67 workgroups."""
import functools
import hashlib

import numpy as np

import sh9_oracle as oracle

PROJECTION = [(16, 16, 3, 2), (12, 20, 3, 2), (15, 15, 1, 1), (5, 5, 4, 3), (40, 40, 3, 2), (1, 1, 3, 1)]
ORACLE_ONLY = (136, 136, 3, 2)
GRID_DIMS = [(6, 6), (5, 8)]                  # where irrad_Z and reconstruct_SH9 are recorded

IRRADIANCE = [(1, 3, "zonal", True), (63, 1, "random", False), (64, 4, "zonal", False), (257, 3, "random", True),
              (1025, 4, "random", False), (1025, 1, "zonal", True), (257, 4, "zonal", True), (64, 3, "random", True)]
ORACLE_ONLY_N = (16900, 3, "random", True)
VIEWS = 3


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def projection_tag(k):
    return "p%dx%dx%d" % PROJECTION[k][:3]


def irradiance_tag(k):
    N, C, kind, per_view = IRRADIANCE[k]
    return "n%d_c%d_%s_%s" % (N, C, kind, "views" if per_view else "shared")


def _frozen(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def make_projection(shape, seed):
    H, W, C, B = shape
    rng = np.random.RandomState(seed)
    return _frozen({"envmap": f32(rng.uniform(0.0, 2.0, (B, H, W, C))), "g_L": f32(rng.uniform(-1, 1, (B, C, 9)))})


@functools.lru_cache(maxsize=None)
def projection(k):
    """{envmap [B, H, W, C], g_L [B, C, 9]} float32.  Read-only: it is cached."""
    return make_projection(PROJECTION[k], 4100 + k)


def make_irradiance(spec, seed):
    N, C, kind, per_view = spec
    rng = np.random.RandomState(seed)
    n_M = VIEWS if per_view else 1
    L = f32(rng.uniform(-1, 1, (n_M, C, 9)))
    if kind == "zonal":
        M = f32(np.stack([oracle.zonal_matrix(L[b].astype(np.float64)) for b in range(n_M)]))
    else:
        M = f32(rng.uniform(-1, 1, (n_M, 4, 4, C)))
    d = rng.standard_normal((VIEWS, N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d[:, 1::2] *= rng.uniform(0.2, 3.0, (VIEWS, N, 1))[:, 1::2]
    d[VIEWS - 1, N - 1] = 0.0
    out = {"L": L if per_view else L[0], "M": M if per_view else M[0], "normal": f32(d),
           "g_E": f32(rng.uniform(-1, 1, (VIEWS, N, C)))}
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def irradiance(k):
    """{L [3, C, 9] or [C, 9] (what a zonal M was made of), M [3, 4, 4, C] or [4, 4, C], normal [3, N, 3], g_E [3, N, C]}
    float32.  Read-only: it is cached."""
    return make_irradiance(IRRADIANCE[k], 5200 + k)


def view_M(c, b):
    return c["M"] if c["M"].ndim == 3 else c["M"][b]


def inside_share(H, W):
    return float(oracle.grid(H, W)["inside"].mean())


def lightprobe_bytes():
    """a 4 x 4 x 3 raw float file: little-endian float32, some values below zero so that the clip and the clamp act"""
    rng = np.random.RandomState(6300)
    return rng.uniform(-0.5, 3.0, (4, 4, 3)).astype("<f4").tobytes()


LIGHTPROBE_CALLS = [{}, {"flipud": False, "normalize": False, "clip_lb_thresh": 0.5}]


def checksum(c, keys):
    h = hashlib.sha256()
    for k in keys:
        a = np.ascontiguousarray(c[k])
        h.update(k.encode() + str(a.shape).encode() + str(a.dtype).encode() + a.tobytes())
    return h.hexdigest()[:16]
