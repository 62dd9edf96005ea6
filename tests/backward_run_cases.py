"""Designed winner maps for the backward kernels' run and workgroup reductions (csrc/srh_backward.h: RunReduce,
scatter_primitive_grads), shared by tests/test_backward_run_cases_cpu.py (which pins them on the oracle's frames) and
tests/test_hip_backward_runs.py.

The backward kernels launch 64 x 4 workgroups: lane = column mod 64, wave = (row - row0) mod 4.  Every case is a small
scene of float32 values whose WINNER MAP is the design: a camera on the z axis looking down -z, screen-facing
primitives in a few depth layers 0.4 % apart (so a camera shifted sideways moves every layer by the same whole number
of columns, views_case), and every primitive edge a quarter of a pixel away from the nearest pixel centre:
  * hband    a long flat triangle whose short edge is vertical on a column boundary: rows [r0, r1) from that column to
             the frame's edge (left or right); the apex is only as far out as the quarter-pixel margin at the far edge
             of the frame needs, and vertex 0 -- the one vertex with a gradient -- is on the short edge;
  * vstrip   the same turned upright: columns [c0, c1) on every row;
  * pixel_*  a disc, sphere or small triangle of 0.3 pixels around one pixel centre: a run of length 1;
  * a background plane, or none (misses), a near-clipped band (a hole of misses inside one primitive's run), and
    planes tangent to a sphere around the eye (each wins one pixel of a one-column frame).
run_features names, per workgroup, the run and merge edges a frame or slab holds; atomic_counts counts the fp32 atomic
additions each gradient entry receives, both from the winner map and the slab's first row alone."""
import copy

import numpy as np

from oracle import np_oracle

EYE_Z = 10.0
Z_PLANE, Z_STRIP, Z_BAND, Z_A, Z_PIXEL = 0.0, 0.06, 0.10, 0.14, 0.20     # depth layers: 4e-3 relative apart and more
MARGIN = 0.25                                                             # pixels between an edge and a pixel centre
KINDS = ("plane", "triangle", "disk", "sphere")

LIGHTS = {"pos": [[4, 3, 12, 1], [-5, 2, 11, 1], [1, -6, 13, 1]], "color_idx": [1, 2, 1],
          "attenuation": [[1, 0.02, 0.001], [0.8, 0.01, 0.002], [1.2, 0.0, 0.003]], "ambient": [0.02, 0.03, 0.01]}
COLORS = [[0, 0, 0], [0.8, 0.7, 0.6], [0.3, 0.5, 0.9]]
ALBEDO = [[0.9, 0.8, 0.7], [0.4, 0.9, 0.5], [0.6, 0.3, 0.8], [0.7, 0.7, 0.2]]
COEFFS = [[0.8, 0.3, 8], [0.7, 0.2, 32], [0.9, 0.4, 2], [0.6, 0.5, 16]]


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


class Builder:
    """Primitives placed in pixel coordinates (u = column, v = row, pixel centres at integers) of a W x H frame."""

    def __init__(self, W, H, plane=True, ortho=False, near=1.0, pitch=None):
        self.W, self.H, self.ortho, self.near = W, H, ortho, near
        pitch = pitch or (0.25 if ortho else 0.025)          # row pitch on the image plane (focal length 1)
        self.h = pitch * max(H - 1, 4)
        self.w = self.h * W / H
        self.x0 = -self.w / 2
        self.y0 = self.h / 2
        self.px = self.w / (W - 1) if W > 1 else self.w
        self.py = self.h / (H - 1) if H > 1 else self.h
        self.prims = {k: [] for k in KINDS}
        if plane:
            self.plane([0, 0, Z_PLANE], [0, 0, 1], 0)

    def scale(self, z):
        return 1.0 if self.ortho else EYE_Z - z

    def xy(self, u, v, z):
        return (self.x0 + u * self.px) * self.scale(z), (self.y0 - v * self.py) * self.scale(z)

    def radius(self, z):
        return 0.3 * min(self.px, self.py) * self.scale(z)

    def plane(self, pos, normal, mat):
        self.prims["plane"].append(dict(pos=list(pos) + [1], normal=list(normal) + [0], material_idx=mat))

    def tri(self, uv, z, mat):
        """Triangle through the pixel-space points uv[0..2] at depth z; uv[0] stays vertex 0, the winding is made
        counter-clockwise about +z (the inside test's sign)."""
        p = [self.xy(u, v, z) for u, v in uv]
        area = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[2][0] - p[0][0]) * (p[1][1] - p[0][1])
        if area < 0:
            p = [p[0], p[2], p[1]]
        self.prims["triangle"].append(dict(face=[[x, y, z, 1] for x, y in p], normal=[0, 0, 1, 0], material_idx=mat))

    def hband(self, r0, r1, c, side, z, mat):
        """Rows [r0, r1) on columns >= c (side 'right') or < c (side 'left')."""
        half = (r1 - r0) / 2 + MARGIN
        reach = 2.2 * half * (self.W + 1)                    # half-height at the frame's far edge >= half - 0.5 + 0.05
        mid = (r0 + r1 - 1) / 2
        u = c - 0.5
        self.tri([(u, mid - half), (u, mid + half), (u + (reach if side == "right" else -reach), mid)], z, mat)

    def vstrip(self, c0, c1, z, mat):
        """Columns [c0, c1) on every row."""
        half = (c1 - c0) / 2 + MARGIN
        reach = 2.2 * half * (self.H + 1)
        mid = (c0 + c1 - 1) / 2
        v = self.H - 0.5 + MARGIN
        self.tri([(mid - half, v), (mid + half, v), (mid, v - reach)], z, mat)

    def pixel_disk(self, c, r, mat, z=Z_PIXEL):
        x, y = self.xy(c, r, z)
        self.prims["disk"].append(dict(pos=[x, y, z, 1], normal=[0, 0, 1, 0], radius=self.radius(z), material_idx=mat))

    def pixel_sphere(self, c, r, mat, z=Z_PIXEL):
        x, y = self.xy(c, r, z)
        self.prims["sphere"].append(dict(pos=[x, y, z, 1], radius=self.radius(z), material_idx=mat))

    def pixel_tri(self, c, r, mat, z=Z_PIXEL):
        self.tri([(c - 0.3, r + 0.3), (c + 0.3, r + 0.3), (c, r - 0.3)], z, mat)

    def scene(self, tonemap=True):
        cam = {"viewport": [0, 0, self.W, self.H], "fovy": float(2 * np.arctan(self.h / 2)), "focal_length": 1.0,
               "eye": _f32([0, 0, EYE_Z, 1]), "at": _f32([0, 0, 0, 1]), "up": _f32([0, 1, 0, 0]), "near": self.near,
               "far": 1000.0, "proj_type": "ortho" if self.ortho else "perspective"}
        objects = {}
        for kind in KINDS:
            if self.prims[kind]:
                objects[kind] = {k: (np.array([p[k] for p in self.prims[kind]], dtype=np.int64) if k == "material_idx"
                                     else _f32([p[k] for p in self.prims[kind]])) for k in self.prims[kind][0]}
        sc = {"camera": cam, "objects": objects, "colors": _f32(COLORS),
              "lights": {"pos": _f32(LIGHTS["pos"]), "color_idx": np.array(LIGHTS["color_idx"]),
                         "attenuation": _f32(LIGHTS["attenuation"]), "ambient": _f32(LIGHTS["ambient"])},
              "materials": {"albedo": _f32(ALBEDO), "coeffs": _f32(COEFFS)}}
        if tonemap:
            sc["tonemap"] = {"type": "gamma", "gamma": 0.8}
        return sc


def _main(ortho=False):
    """129 x 9.  Columns 0..63: rows 0-1 band B, rows 2-5 band A, rows 6-8 band C -- each a full wave per row, so the
    frame's workgroups (rows 0-3, 4-7, 8) hold two waves of one and two of the other, slab (2, 6) merges A, slabs
    (1, 9) and (3, 8) hold three waves of one and one of the other, and (0, 1), (2, 8), (2, 9) end in 3, 2 and 1 dead
    rows under full waves.  A runs on through columns 64..128 (a run across the wave boundary, one live lane in the
    right-edge workgroup) with one foreign disc at lane 0 of row 3.  Over the background plane in columns 64..128 of
    the other rows: single pixels at lanes 0, 63 and inside, a strip of 3, a run of 2 that crosses into column 128,
    and eight single-pixel discs, spheres and triangles."""
    b = Builder(129, 9, ortho=ortho)
    b.hband(0, 2, 64, "left", Z_BAND, 2)                     # B
    b.hband(2, 6, 0, "right", Z_A, 1)                        # A
    b.hband(6, 9, 64, "left", Z_BAND, 3)                     # C
    b.hband(7, 8, 126, "right", Z_STRIP, 2)                  # run of 2 in lanes 62-63, on into column 128
    b.vstrip(100, 103, Z_STRIP, 3)                           # a strip of 3 on rows 0, 1, 6, 7, 8 (behind A)
    b.pixel_disk(64, 0, 1)
    b.pixel_disk(127, 0, 2)
    b.pixel_disk(90, 0, 3)
    b.pixel_sphere(127, 1, 0)
    b.pixel_sphere(127, 6, 1)
    b.pixel_disk(64, 3, 0)                                   # the foreign pixel on A: lane 0 of wave 1 in slab (2, 6)
    for i in range(8):
        b.pixel_disk(66 + 2 * i, 6, i % 4)
        b.pixel_sphere(66 + 2 * i, 7, (i + 1) % 4)
        b.pixel_tri(66 + 2 * i, 8, (i + 2) % 4)
    b.pixel_disk(90, 8, 0)                                   # three kinds side by side
    b.pixel_sphere(91, 8, 1)
    b.pixel_tri(92, 8, 2)
    return b


def _f65x5():
    """65 x 5, no background.  Rows 0-3: A with one foreign disc at lane 31 of row 1; column 64 is a right-edge
    workgroup with one live lane, all A.  Row 4: a band on columns 0..39, misses, single pixels at lanes 50 and 63;
    column 64 of row 4 is a workgroup without a hit."""
    b = Builder(65, 5, plane=False)
    b.hband(0, 4, 0, "right", Z_A, 1)
    b.pixel_disk(31, 1, 2)
    b.hband(4, 5, 40, "left", Z_BAND, 3)
    b.pixel_sphere(50, 4, 0)
    b.pixel_tri(63, 4, 2)
    return b


def _f64x4(which):
    """64 x 4, one workgroup.  'a': A with a foreign disc in wave 0; 'b': A with a foreign sphere at lane 63 of wave 3;
    'c': wave 0 all misses under three waves of A; 'd': the plane from lane 0 to 62 (a run of 63) and a disc at 63."""
    b = Builder(64, 4, plane=which == "d")
    if which == "d":
        b.pixel_disk(63, 2, 1)
        b.pixel_sphere(0, 1, 2)
        return b
    b.hband(1 if which == "c" else 0, 4, 0, "right", Z_A, 1)
    if which == "a":
        b.pixel_disk(5, 0, 2)
    if which == "b":
        b.pixel_sphere(63, 3, 3)
    return b


def _f63(H):
    """63 x 4: every live lane of a right-edge workgroup with 63 live lanes is A.  63 x 3 (no background): row 0 one
    band, row 2 another, row 1 a band closer than `near` around the view axis -- the same primitive left and right of
    nine misses."""
    if H == 4:
        b = Builder(63, 4)
        b.hband(0, 4, 0, "right", Z_A, 1)
        return b
    b = Builder(63, 3, plane=False, near=5.0)
    b.hband(0, 1, 0, "right", Z_BAND, 0)
    b.hband(2, 3, 63, "left", Z_BAND, 2)
    x = 4.5 * b.px                                           # the hole: columns 31 - 4 .. 31 + 4
    b.hband(1, 2, 0, "right", EYE_Z - b.near / np.sqrt(1 + x * x), 3)
    return b


def _tangent_planes(H):
    """1 x H: H planes tangent to the sphere of radius 10 around the eye, plane k at the ray of row k and facing the eye:
    along ray j plane k is hit at 10 / (d_k . d_j), so each plane wins its own pixel (rows 0.06 apart: by 1.8e-3)."""
    b = Builder(1, H, plane=False, pitch=0.06)
    sc = b.scene()
    eye, d, _, _ = np_oracle.generate_rays(sc["camera"])
    for k in range(H):
        b.plane(list(eye[:3] + 10.0 * d[:3, k]), list(-d[:3, k]), k % 4)
    return b


def cases():
    """{name: scene} (ndarray leaves, float32 values, tonemap gamma 0.8)."""
    out = {"129x9": _main().scene(), "65x5": _f65x5().scene(), "63x3": _f63(3).scene(), "63x4": _f63(4).scene(),
           "1x7": _tangent_planes(7).scene(), "1x1": _tangent_planes(1).scene()}
    for which in "abcd":
        out["64x4" + which] = _f64x4(which).scene()
    return out


def ortho_case():
    """The 129 x 9 design under an orthographic camera (torch shading only)."""
    return _main(ortho=True).scene()


SLABS = ((0, 1), (1, 9), (3, 8), (2, 6), (2, 8), (2, 9))     # of 129x9; the last two: 2 and 1 dead rows under full waves
VIEW_SHIFTS = (0, 5, -3)                                     # columns


def views_case():
    """(scene, cameras, overrides): three views of 129x9, the camera moved sideways by VIEW_SHIFTS columns of the
    background plane's depth (the nearer layers move by 2 % more: 0.1 pixel), view 1 with lights of its own."""
    b = _main()
    scene = b.scene()
    cams = []
    for s in VIEW_SHIFTS:
        dx = -s * b.px * EYE_Z
        cam = copy.deepcopy(scene["camera"])
        cam["eye"] = _f32(cam["eye"] + np.array([dx, 0, 0, 0]))
        cam["at"] = _f32(cam["at"] + np.array([dx, 0, 0, 0]))
        cams.append(cam)
    lights = _f32(np.asarray(scene["lights"]["pos"]) + np.array([[0.5, -0.25, 0.5, 0], [0.25, 0.5, -0.5, 0], [-0.5, 0.25, 0.25, 0]]))
    return scene, cams, [{}, {"lights.pos": lights}, {}]


# ---- what a frame holds -----------------------------------------------------------------------------------------------
def primitive_table(scene):
    """(kind index per global primitive, material per global primitive)."""
    kind, mat = [], []
    for k, grp in scene["objects"].items():
        m = np.asarray(grp["material_idx"])
        kind += [KINDS.index(k)] * len(m)
        mat += list(m)
    return np.array(kind), np.array(mat)


def workgroups(nearest, hit, row0, W, row1=None):
    """Yields (bx, by, keys (4, 64)) per 64 x 4 workgroup of rows [row0, row1) of a frame: the winner's global index,
    -1 at a miss and at a dead lane or row."""
    nearest, hit = np.asarray(nearest), np.asarray(hit)
    row1 = nearest.shape[0] if row1 is None else row1
    for by in range((row1 - row0 + 3) // 4):
        for bx in range((W + 63) // 64):
            keys = np.full((4, 64), -1, dtype=np.int64)
            rows = range(row0 + 4 * by, min(row0 + 4 * by + 4, row1))
            c0, c1 = 64 * bx, min(64 * bx + 64, W)
            for w, r in enumerate(rows):
                keys[w, :c1 - c0] = np.where(hit[r, c0:c1], nearest[r, c0:c1], -1)
            yield bx, by, keys, len(rows), c1 - c0


def runs(row):
    """[(start, length, key)] of the maximal runs of one wave's 64 keys."""
    out, s = [], 0
    for i in range(1, 65):
        if i == 64 or row[i] != row[s]:
            out.append((s, i - s, int(row[s])))
            s = i
    return out


def merged(keys):
    """scatter_primitive_grads' workgroup merge: each wave one run of the same primitive."""
    return keys[0, 0] >= 0 and bool(np.all(keys == keys[0, 0]))


FEATURES = ("run1_lane0", "run1_lane63", "run1_inside", "run2", "run63", "cross_wave", "repeat_other", "repeat_miss",
            "merge", "three_one", "two_two", "foreign_lane0", "foreign_lane31", "foreign_lane63", "foreign_wave0",
            "wave0_miss", "dead_rows_1", "dead_rows_2", "dead_rows_3", "edge_live1", "edge_live63", "early_exit",
            "two_kinds_adjacent", "one_material_wave", "many_material_wave") + tuple("runs_of_" + k for k in KINDS)


def run_features(nearest, hit, row0, W, row1=None, kind_of=None, mat_of=None):
    """{feature: [(bx, by), ...]} for rows [row0, row1) of a frame, by the launch geometry of the backward kernels."""
    found = {}
    groups = list(workgroups(nearest, hit, row0, W, row1))
    has_hit = {(bx, by): bool((k >= 0).any()) for bx, by, k, _, _ in groups}

    def note(name, bx, by):
        found.setdefault(name, []).append((bx, by))

    for bx, by, keys, live_rows, live_lanes in groups:
        if not has_hit[bx, by]:
            if any(has_hit.get((bx + dx, by + dy), False) for dx in (-1, 0, 1) for dy in (-1, 0, 1)):
                note("early_exit", bx, by)
            continue
        full = [bool(keys[w, 0] >= 0 and np.all(keys[w] == keys[w, 0])) for w in range(4)]
        heads = [int(keys[w, 0]) for w in range(4)]
        if merged(keys):
            note("merge", bx, by)
        elif all(full):
            kinds = sorted(heads.count(k) for k in set(heads))
            if kinds == [1, 3]:
                note("three_one", bx, by)
            if heads[0] == heads[1] != heads[2] == heads[3]:
                note("two_two", bx, by)
        # four waves of one primitive but for one pixel
        vals, counts = np.unique(keys, return_counts=True)
        if len(vals) == 2 and counts.min() == 1 and vals[np.argmax(counts)] >= 0 and vals.min() >= 0:
            w, lane = [int(a[0]) for a in np.nonzero(keys == vals[np.argmin(counts)])]
            if w == 0:
                note("foreign_wave0", bx, by)
            elif lane in (0, 31, 63):
                note(f"foreign_lane{lane}", bx, by)
        if not (keys[0] >= 0).any() and all(full[1:]) and heads[1] == heads[2] == heads[3]:
            note("wave0_miss", bx, by)
        live = keys[:live_rows, :live_lanes]
        one = live[0, 0] >= 0 and bool(np.all(live == live[0, 0]))
        if one and live_lanes == 64 and live_rows < 4:
            note(f"dead_rows_{4 - live_rows}", bx, by)
        if one and live_rows == 4 and live_lanes in (1, 63):
            note(f"edge_live{live_lanes}", bx, by)
        for w in range(live_rows):
            rr = runs(keys[w])
            hits = [(s, n, k) for s, n, k in rr if k >= 0]
            for s, n, k in hits:
                if n == 1:
                    note("run1_lane0" if s == 0 else "run1_lane63" if s == 63 else "run1_inside", bx, by)
                if n in (2, 63):
                    note(f"run{n}", bx, by)
                if kind_of is not None:
                    note("runs_of_" + KINDS[kind_of[k]], bx, by)
            for (s0, n0, k0), (s1, n1, k1) in zip(rr, rr[1:]):
                if kind_of is not None and k0 >= 0 and k1 >= 0 and kind_of[k0] != kind_of[k1]:
                    note("two_kinds_adjacent", bx, by)
            for i, (s0, n0, k0) in enumerate(hits):
                for s1, n1, k1 in hits[i + 1:]:
                    if k1 == k0:
                        between = keys[w, s0 + n0:s1]
                        note("repeat_miss" if np.all(between < 0) else "repeat_other", bx, by)
            if mat_of is not None and hits:
                mats = {int(mat_of[k]) for _, _, k in hits}
                note("one_material_wave" if len(mats) == 1 else "many_material_wave", bx, by)
            # the same primitive at lane 63 here and at lane 0 of the workgroup to the right
            if keys[w, 63] >= 0:
                for bx2, by2, keys2, _, _ in groups:
                    if (bx2, by2) == (bx + 1, by) and keys2[w, 0] == keys[w, 63]:
                        note("cross_wave", bx, by)
    return found


def single_pixel_primitives(nearest, hit):
    """Global indices of the primitives that win exactly one pixel of the frame."""
    vals, counts = np.unique(np.asarray(nearest)[np.asarray(hit)], return_counts=True)
    return vals[counts == 1]


def atomic_counts(nearest, hit, row0, W, row1, n_prims, mat_of):
    """The fp32 atomic additions the backward kernels issue, from the winner map alone: (per primitive: its
    (wave, run) groups, one for a merged workgroup; the waves with a hit: what every light, colour, ambient and
    attenuation entry receives; per material: the waves shaded by it alone -- judged as the kernels judge it, against
    lane 0's material, which is 0 where lane 0 hits nothing -- plus its hit lanes in every other wave)."""
    prim = np.zeros(n_prims, dtype=np.int64)
    mats = np.zeros(int(np.max(mat_of)) + 1 if len(mat_of) else 1, dtype=np.int64)
    waves = 0
    for _, _, keys, _, _ in workgroups(nearest, hit, row0, W, row1):
        if not (keys >= 0).any():
            continue
        if merged(keys):
            prim[keys[0, 0]] += 1
        else:
            for w in range(4):
                for _, _, k in runs(keys[w]):
                    if k >= 0:
                        prim[k] += 1
        for w in range(4):
            hits = keys[w] >= 0
            if not hits.any():
                continue                                     # an all-miss wave adds zeros: no atomic
            waves += 1
            m = np.where(hits, mat_of[np.maximum(keys[w], 0)], 0)
            if np.all(m[hits] == m[0]):
                mats[m[0]] += 1
            else:
                np.add.at(mats, m[hits], 1)
    return prim, waves, mats


# ---- margins: all pairs, from the oracle's own intersection routines ----------------------------------------------------------
def margins(scene, torch_shading=False):
    """(nearest, hit, smallest relative gap between a winner and the runner-up, smallest relative gap between any
    intersection and the near / far clip, smallest distance from a hit point to a light) of the frame, all pairs."""
    from oracle import np_oracle_tch
    cam = scene["camera"]
    if torch_shading:
        res = np_oracle_tch.render(scene)
        hit = res["depth"] <= cam["far"]
    else:
        res = np_oracle.render(scene)
        hit = np.isfinite(res["depth"])
    objs = {k: {f: np.asarray(v, dtype=np.float64) if f != "material_idx" else np.asarray(v) for f, v in g.items()}
            for k, g in scene["objects"].items()}
    segs, total = np_oracle._segments(objs)
    if np_oracle_tch.is_ortho(cam):
        _, orig, dvec, H, W = np_oracle_tch.generate_rays_ortho(cam)
        dirs = np.broadcast_to(dvec[None, :], orig.shape)
    else:
        eye, d, H, W = np_oracle_tch.generate_rays(cam)
        dirs = d.T
        orig = np.broadcast_to(eye[None, :], dirs.shape)
    with np.errstate(all="ignore"):
        t = np_oracle_tch._hits_general(segs, total, orig, dirs)
    finite = np.isfinite(t)
    clip = np.min(np.minimum(np.abs(t[finite] - cam["near"]) / cam["near"], np.abs(t[finite] - cam["far"]) / cam["far"]))
    t = np.where((t >= cam["near"]) & (t <= cam["far"]), t, np.inf)
    order = np.sort(t, axis=0)
    first, second = order[0], (order[1] if total > 1 else np.full_like(order[0], np.inf))
    assert np.array_equal(np.isfinite(first).reshape(H, W), hit)
    assert np.array_equal(np.argmin(t, axis=0).reshape(H, W)[hit], res["nearest"][hit])
    with np.errstate(all="ignore"):
        gap = np.min(np.where(np.isfinite(second) & np.isfinite(first), (second - first) / first, np.inf))
    p = orig + np.where(np.isfinite(first), first, 0.0)[:, None] * dirs
    lights = np.asarray(scene["lights"]["pos"], dtype=np.float64)[:, :3]
    dist = np.sqrt(((p[:, None, :] - lights[None]) ** 2).sum(-1))[np.isfinite(first)]
    return res["nearest"], hit, float(gap), float(clip), float(dist.min())


def atomics_like(scene, key, prim, waves, mats):
    """atomic_counts' figures as an array that broadcasts against leaf `key`."""
    a, _, b = key.partition(".")
    if a in scene["objects"]:
        start = 0
        for kind, grp in scene["objects"].items():
            n = len(grp["material_idx"])
            if kind == a:
                shape = (n,) + (1,) * (np.asarray(grp[b]).ndim - 1)
                return prim[start:start + n].reshape(shape)
            start += n
    if a == "materials":
        out = np.zeros(len(scene["materials"]["albedo"]))
        out[:len(mats)] = mats[:len(out)]
        return out[:, None]
    if key == "colors":                                      # one atomic per wave and light into the light's colour row
        return waves * np.bincount(np.asarray(scene["lights"]["color_idx"]), minlength=len(scene["colors"]))[:, None]
    return np.float64(waves)
