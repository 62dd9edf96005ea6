"""Seeded inputs of the point-set tests -- test infrastructure.  REGULAR cases are comparable with the reference (margins
between the best and the second-best distance, no coincident pair: tests/test_pointsets_cases_cpu.py asserts them) and
have fixtures under tests/golden/pointsets; EDGE cases (ties, coincident points, NaN, inf, extreme magnitudes, a
1300-term fan-in) are checked against tests/pointsets_oracle.py alone, because the reference gives NaN or leaves ties
open on them."""
import hashlib

import numpy as np

VIEWS = 3
QUERIES_PER_WORKGROUP, UNROLL = 256, 8            # srh_pointsets.h: kPsQueries, kPsUnroll
# (N, M, D); the last is one query and one target past a workgroup and a round of the stream
REGULAR = [(1, 1, 3), (1, 5, 3), (5, 1, 3), (63, 65, 3), (64, 64, 1), (65, 63, 2), (257, 1025, 3), (1300, 700, 4),
           (QUERIES_PER_WORKGROUP + 1, UNROLL + 1, 3)]


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def tag(k):
    return "%dx%dx%d" % REGULAR[k]


def regular(k):
    """Case k: u [3, N, D], v [3, M, D] float32 -- view b from RandomState(1000 k + b): normal variates, v scaled 1.1 and
    shifted 0.2 -- with upstream gradients in (-1, 1): g [3, 3] for (sym, uv, vu), g_u [3, N], g_v [3, M] for the dists."""
    N, M, D = REGULAR[k]
    u, v = np.empty((VIEWS, N, D), np.float32), np.empty((VIEWS, M, D), np.float32)
    for b in range(VIEWS):
        rng = np.random.RandomState(1000 * k + b)
        u[b] = f32(rng.standard_normal((N, D)))
        v[b] = f32(rng.standard_normal((M, D)) * 1.1 + 0.2)
    rng = np.random.RandomState(77000 + k)
    up = {"g": f32(rng.uniform(-1, 1, (VIEWS, 3))), "g_u": f32(rng.uniform(-1, 1, (VIEWS, N))),
          "g_v": f32(rng.uniform(-1, 1, (VIEWS, M)))}
    return {"name": tag(k), "u": u, "v": v, **up}


def _with_upstreams(name, u, v, seed, **notes):
    u, v = f32(u), f32(v)
    rng = np.random.RandomState(88000 + seed)
    return {"name": name, "u": u, "v": v, "g_u": f32(rng.uniform(0.25, 1, len(u)) * rng.choice([-1, 1], len(u))),
            "g_v": f32(rng.uniform(0.25, 1, len(v)) * rng.choice([-1, 1], len(v))), **notes}


def edges():
    """One view each, u [N, D], v [M, D]; the upstream gradients have no zero, so a zero gradient is the layer's."""
    nan, inf = float("nan"), float("inf")
    rng = np.random.RandomState(4242)
    cloud_u, cloud_v = rng.standard_normal((40, 3)), rng.standard_normal((37, 3)) * 1.1 + 0.2
    out = []
    # exact ties: the lowest index wins
    out.append(_with_upstreams("tie_lattice", [[0.0], [2.0]], [[1.0], [1.0]], 0))
    dup = np.concatenate([cloud_v[:9], cloud_v[:9], cloud_v[3:6]])
    out.append(_with_upstreams("tie_duplicated_targets", cloud_u[:20], dup, 1))
    grid = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    out.append(_with_upstreams("tie_integer_grid", grid + 0.5, grid, 2))
    # coincident points: v[4] = u[7] wins for u[7]; the duplicate of it at v[30] never wins; and u = v
    co = cloud_v.copy()
    co[4], co[30] = cloud_u[7], cloud_u[7]
    out.append(_with_upstreams("coincident_pair", cloud_u, co, 3))
    out.append(_with_upstreams("identical_sets", cloud_u, cloud_u, 4))
    # non-finite coordinates
    bad = cloud_v.copy()
    bad[5, 1] = nan
    out.append(_with_upstreams("nan_target", cloud_u, bad, 5, dead_v=[5]))
    bad = cloud_u.copy()
    bad[3, 0] = nan
    out.append(_with_upstreams("nan_query", bad, cloud_v, 6, dead_u=[3]))
    bad_u, bad_v = cloud_u.copy(), cloud_v.copy()
    bad_u[2, 2], bad_v[6, 0], bad_v[8, 1] = inf, -inf, inf
    out.append(_with_upstreams("inf_coordinates", bad_u, bad_v, 7, dead_u=[2], dead_v=[6, 8]))
    out.append(_with_upstreams("all_nan_targets", cloud_u[:11], np.full((9, 3), nan), 8,
                               dead_u=list(range(11)), dead_v=list(range(9))))
    # 1e-40 (a float32 subnormal) and 3e38 together: fp64 neither underflows nor overflows on them
    tiny = np.array([[1e-40, 0, 0], [0, -2e-40, 0], [3e38, 3e38, -3e38], [-3e38, 1e-40, 3e38], [2.5e38, 3e38, -3e38]])
    out.append(_with_upstreams("extreme_magnitudes", tiny, tiny[[1, 4, 0, 3]] * np.array([0.5, 0.5, 1.0]), 9))
    # every query nearest to the one target: grad_v[0] is a 1300-term sum
    out.append(_with_upstreams("fan_in", np.random.RandomState(9).standard_normal((1300, 3)), [[0.1, -0.2, 0.3]], 10))
    return out


def checksum(c):
    h = hashlib.sha256()
    for k in ("u", "v", "g_u", "g_v") + (("g",) if "g" in c else ()):
        a = np.ascontiguousarray(c[k])
        h.update(k.encode() + str(a.shape).encode() + str(a.dtype).encode() + a.tobytes())
    return h.hexdigest()[:16]
