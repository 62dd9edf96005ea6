"""Scenes for the shadow-pass tests (numpy only; importable without a GPU).

`random_shadow_scene` draws the random scenes of tests/test_hip_shadow_fuzz.py: the recipe of `_random_scene` (the
primary pass's fuzz, kept here so that both fuzzes share it) plus the torch backend's shading inputs, a random number of
lights placed where the light-view path of srh_shadow.h takes its decisions, and structural cases forced in turn.  The
deterministic builders below hold the edges a random draw reaches rarely.  `OCCURRED` counts what the scenes built so
far contain; tests/test_shadow_scenes_cpu.py asserts on it for the very seeds the GPU tests use.

`undecided` is the reference-only mask of the oracle comparisons: the (light, pixel) pairs whose visibility flips when
the oracle's own fragment positions move by 1e-9 relative / 1e-10 absolute -- many orders above the fp64 rounding
differences between kernel and oracle -- and those whose shadow ray lies in a flat primitive's plane to within that
much (a 0 / 0 hit distance).  A kernel may differ from the oracle there and nowhere else.
"""
import collections

import numpy as np

f32 = lambda a: np.asarray(a, dtype=np.float32)          # noqa: E731

# the constants of the light-view path that the scenes aim at (srh_shadow.h, srh.hip: srh_shadow_shade)
VIEW_RES_FINE, VIEW_RES_COARSE, TILE = 4096, 2048, 16
FINE_MAX_TILES = 3.2
NEAR_GAPS = (0.05, 0.0999, 0.1002, 0.3)

LIGHT_FAMILIES = ("far", "threshold", "inside", "primitive_centre", "disc_normal", "in_plane")
STRUCTURAL = ("planes_only", "one_primitive", "non_finite", "fine_view", "coarse_view", "mixed_views", "wide_occluder",
              "crowd", "far_receivers")
MANY_LIGHTS = (31, 32, 33, 63, 64)

# what the scenes built so far contain: structural cases (as measured on the finished scene where the scene alone
# shows it, see `describe`), light families, "many_lights", "view" / "no_view" per light
OCCURRED = collections.Counter()

# the seeds and sizes of tests/test_hip_shadow_fuzz.py, whose premises tests/test_shadow_scenes_cpu.py checks
FUZZ_SEED, FUZZ_COUNT = 2026, 120
# The oracle set's seed is one whose scenes meet the premise the CPU test asserts with the oracle alone (undecided
# pairs <= 0.5 %; measured 0.11 %): a light drawn INTO a plane leaves the shadowed fragments of that plane undecided
# (`undecided`), and a seed with such a plane filling the frame (2036: 1.5 %, 2040: 0.8 %) exceeds the cap.
ORACLE_SEED, ORACLE_COUNT = 2039, 15                     # each scene in both projections


def _random_scene(rng):
    """A random mixed scene for the fuzzes: 1-4 primitive types, 1-3000 primitives each with log-uniform sizes from
    sub-pixel to screen-filling, random camera (also inside the cloud), near in {0, 0.01, 0.1, 1}."""
    W, H = int(rng.choice([48, 64, 97, 128, 200])), int(rng.choice([48, 64, 80, 128, 160]))
    eye = rng.normal(size=3)
    eye = eye / np.linalg.norm(eye) * rng.choice([0.3, 1.0, 2.5, 4.0, 8.0])
    cam = {"viewport": [0, 0, W, H], "fovy": float(np.deg2rad(rng.choice([20, 45, 70, 110]))),
           "focal_length": float(rng.choice([0.5, 1.0, 3.0])), "eye": [*map(float, eye), 1.0],
           "at": [*map(float, rng.normal(size=3) * 0.2), 1.0], "up": [*map(float, rng.normal(size=3)), 0.0],
           "near": float(rng.choice([0.0, 0.01, 0.1, 1.0])), "far": float(rng.choice([5.0, 50.0, 1000.0]))}
    objs = {}
    for k in list(rng.permutation(["disk", "triangle", "sphere", "plane"]))[: rng.randint(1, 5)]:
        n = int(rng.choice([1, 5, 60, 700, 3000])) if k != "plane" else int(rng.choice([1, 2, 3]))
        pos = np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)), np.ones((n, 1))], 1)
        nrm = np.concatenate([rng.normal(size=(n, 3)), np.zeros((n, 1))], 1)
        mat = rng.randint(0, 3, n)
        if k == "disk":
            objs[k] = {"pos": f32(pos), "normal": f32(nrm), "material_idx": mat,
                       "radius": f32(np.exp(rng.uniform(np.log(0.003), np.log(1.5), n)))}
        elif k == "sphere":
            objs[k] = {"pos": f32(pos), "radius": f32(np.exp(rng.uniform(np.log(0.005), np.log(0.8), n))), "material_idx": mat}
        elif k == "plane":
            pos[:, :3] *= 2.0
            objs[k] = {"pos": f32(pos), "normal": f32(nrm), "material_idx": mat}
        else:
            c = rng.uniform(-1.5, 1.5, (n, 1, 3))
            v = c + rng.normal(size=(n, 3, 3)) * np.exp(rng.uniform(np.log(0.01), np.log(0.8), (n, 1, 1)))
            fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) * rng.choice([-1, 1], (n, 1))
            objs[k] = {"face": f32(np.concatenate([v, np.ones((n, 3, 1))], 2)),
                       "normal": f32(np.concatenate([fn, np.zeros((n, 1))], 1)), "material_idx": mat}
    return {"camera": cam, "lights": {"pos": f32([[3, 4, 5, 1], [-4, 2, 3, 1]]), "color_idx": np.array([1, 2])},
            "colors": f32([[0, 0, 0], [.8, .5, .4], [.3, .6, .9]]),
            "materials": {"albedo": f32([[.5, .5, .5], [.9, .3, .2], [.2, .7, .4]])},
            "objects": objs, "tonemap": {"type": "gamma", "gamma": 0.8}}


# ---- the host's restatement of k_scene_bounds / k_light_frames ------------------------------------------------------
def primitive_count(scene):
    return sum(len(g["material_idx"]) for g in scene["objects"].values())


def scene_bounds(scene):
    """What k_scene_bounds leaves for k_light_frames: the box of the finite discs, spheres and triangles (fp32, as the
    kernel computes it), `rad` = 1.01 |half diagonal| + 1e-6 of its bounding sphere, the mean primitive size (a radius; a
    triangle counts half its longest box edge).  `ok` is False where no light can have a view: no finite primitive at
    all, or one with a non-finite extent."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    bad, size, count = False, 0.0, 0
    with np.errstate(all="ignore"):
        for kind, g in scene["objects"].items():
            if kind == "plane":
                continue
            if kind == "triangle":
                v = f32(g["face"])[:, :, :3]
                plo, phi = v.min(axis=1), v.max(axis=1)
                psize = np.float32(0.5) * (phi - plo).max(axis=1)
            else:
                c, r = f32(g["pos"])[:, :3], np.abs(f32(g["radius"])).reshape(-1, 1)
                plo, phi = c - r, c + r
                psize = r[:, 0]
            fin = np.isfinite(plo).all(axis=1) & np.isfinite(phi).all(axis=1)
            bad |= not fin.all()
            if fin.any():
                lo, hi = np.minimum(lo, plo[fin].min(axis=0)), np.maximum(hi, phi[fin].max(axis=0))
                ok = fin & np.isfinite(psize)
                size += float(psize[ok].astype(np.float64).sum())
                count += int(ok.sum())
    have = bool(np.all(lo <= hi))
    centre = 0.5 * (lo + hi) if have else np.zeros(3)
    rad = float(np.linalg.norm(hi - centre)) * 1.01 + 1.0e-6 if have else 0.0
    return {"ok": have and not bad, "have": have, "bad": bad, "lo": lo, "hi": hi, "centre": centre, "rad": rad,
            "mean": size / count if count else 0.0}


def light_views(scene, bounds=None):
    """Per light what k_light_frames decides: None (no usable view: all pairs) or the view's resolution, with the
    distance from the box centre and the view's half extent."""
    b = bounds or scene_bounds(scene)
    out = []
    for L in np.asarray(scene["lights"]["pos"], dtype=np.float32).astype(np.float64)[:, :3]:
        dist = float(np.linalg.norm(L - b["centre"]))
        if not (b["ok"] and np.isfinite(dist) and np.isfinite(L).all() and dist > 1.3 * b["rad"] + 0.2):
            out.append(None)
            continue
        half = np.tan(1.02 * np.arcsin(b["rad"] / dist))
        tiles_fine = b["mean"] / (half * dist) * VIEW_RES_FINE / TILE
        res = VIEW_RES_FINE if tiles_fine <= FINE_MAX_TILES else VIEW_RES_COARSE
        out.append({"res": res, "dist": dist, "half": half, "tiles_fine": tiles_fine})
    return out


def describe(scene):
    """The structural cases that the finished scene shows by itself."""
    found = set()
    objs = scene["objects"]
    b = scene_bounds(scene)
    views = light_views(scene, b)
    if set(objs) == {"plane"}:
        found.add("planes_only")
    if primitive_count(scene) == 1:
        found.add("one_primitive")
    if b["bad"]:
        found.add("non_finite")
    res = {v["res"] for v in views if v}
    if VIEW_RES_FINE in res:
        found.add("fine_view")
    if VIEW_RES_COARSE in res:
        found.add("coarse_view")
    if len(res) == 2:
        found.add("mixed_views")
    # an occluder of more than 64 tiles of some light's view: its diameter against the view's extent at the box centre
    # (a lower bound for what is nearer the light), 9 tiles across so that it spans more than 8 x 8 wherever it lies
    biggest = 0.0
    for kind, g in objs.items():
        if kind in ("disk", "sphere"):
            r = np.abs(f32(g["radius"]))
            biggest = max(biggest, float(r[np.isfinite(r)].max(initial=0.0)))
    for v in views:
        if v and 2.0 * biggest / (2.0 * v["half"] * v["dist"]) * v["res"] / TILE > 9.0:
            found.add("wide_occluder")
    return found, views


# ---- lights ---------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v)


def _perp(n, rng):
    a = np.cross(n, rng.normal(size=3))
    return _unit(a)


def _draw_light(rng, scene, bounds, family):
    """One light position of `family`; families that need what the scene lacks fall back to `far`."""
    objs = scene["objects"]
    have = bounds["have"]
    centre = bounds["centre"] if have else np.zeros(3)
    rad = bounds["rad"] if have else 2.0
    if family == "threshold" and have:
        return centre + _unit(rng.normal(size=3)) * (1.3 * rad + 0.2) * rng.uniform(0.95, 1.05)
    if family == "inside" and have:
        return rng.uniform(bounds["lo"], bounds["hi"])
    if family == "primitive_centre":
        kind = str(rng.choice(sorted(objs)))
        g = objs[kind]
        i = int(rng.randint(len(g["material_idx"])))
        c = g["face"][i, :, :3].mean(axis=0) if kind == "triangle" else g["pos"][i, :3]
        if np.isfinite(c).all():
            return np.asarray(c, dtype=np.float64)
    if family == "disc_normal" and "disk" in objs:
        g = objs["disk"]
        i = int(rng.randint(len(g["material_idx"])))
        n, p = np.asarray(g["normal"][i, :3], dtype=np.float64), np.asarray(g["pos"][i, :3], dtype=np.float64)
        gap = float(rng.choice(NEAR_GAPS)) * float(rng.choice([-1.0, 1.0]))
        if np.isfinite(n).all() and np.isfinite(p).all() and np.linalg.norm(n) > 0:
            return p + gap * _unit(n)
    if family == "in_plane" and ("plane" in objs or "disk" in objs):
        kind = str(rng.choice(sorted(set(objs) & {"plane", "disk"})))
        g = objs[kind]
        i = int(rng.randint(len(g["material_idx"])))
        n, p = np.asarray(g["normal"][i, :3], dtype=np.float64), np.asarray(g["pos"][i, :3], dtype=np.float64)
        if np.isfinite(n).all() and np.isfinite(p).all() and np.linalg.norm(n) > 0:
            u = _perp(_unit(n), rng)
            return p + u * rng.uniform(-2.0, 2.0) + np.cross(_unit(n), u) * rng.uniform(-2.0, 2.0)
    if family != "far":
        OCCURRED["fell_back_to_far"] += 1
    return centre + _unit(rng.normal(size=3)) * rad * rng.uniform(3.0, 10.0)


def _set_lights(rng, scene, n_lights, first=()):
    """`n_lights` lights: the positions in `first`, then one family per light."""
    bounds = scene_bounds(scene)
    pos = [np.asarray(p, dtype=np.float64) for p in first][:n_lights]
    while len(pos) < n_lights:
        family = str(rng.choice(LIGHT_FAMILIES))
        OCCURRED[family] += 1
        pos.append(_draw_light(rng, scene, bounds, family))
    laws = f32([[1, 0, 0], [0.5, 0.1, 0.01], [1, 0, 0.02], [0.3, 0.2, 0]])
    scene["lights"] = {"pos": f32(np.concatenate([np.stack(pos), np.ones((n_lights, 1))], axis=1)),
                       "color_idx": rng.randint(1, 3, n_lights), "attenuation": laws[rng.randint(0, 4, n_lights)],
                       "ambient": f32(rng.uniform(0.0, 0.03, 3))}
    scene["materials"]["coeffs"] = f32([[1, 0, 0], [0.7, 0.3, 5], [0.5, 0.5, 20]])


def _truncate(scene, limit):
    """At most `limit` primitives: the batches are cut in proportion, none below one."""
    total = primitive_count(scene)
    if total <= limit:
        return
    for g in scene["objects"].values():
        n = len(g["material_idx"])
        keep = max(1, int(n * limit / total) - 1)
        for k in list(g):
            g[k] = g[k][:keep]


def _look_at_origin(rng, scene, distance=4.0, far=50.0):
    eye = _unit(rng.normal(size=3) + np.array([0.0, 1.0, 0.0])) * distance
    scene["camera"].update(eye=[*map(float, eye), 1.0], at=[0.0, 0.0, 0.0, 1.0], near=0.01, far=far,
                           fovy=float(np.deg2rad(45)), focal_length=1.0)


def _tiny_discs(rng, n, box, r0, r1):
    pos = np.concatenate([rng.uniform(-box, box, (n, 3)), np.ones((n, 1))], 1)
    nrm = np.concatenate([rng.normal(size=(n, 3)), np.zeros((n, 1))], 1)
    return {"pos": f32(pos), "normal": f32(nrm), "material_idx": rng.randint(0, 3, n),
            "radius": f32(np.exp(rng.uniform(np.log(r0), np.log(r1), n)))}


def _floor(y=-1.2):
    return {"pos": f32([[0, y, 0, 1]]), "normal": f32([[0, 1, 0, 0]]), "material_idx": np.array([0])}


def _structure(rng, scene, case):
    """Rebuild the scene's objects (and where it matters its camera) for one structural case; returns light positions
    that the case needs."""
    first = []
    if case == "planes_only":
        n = int(rng.choice([1, 2, 3]))
        pos = np.concatenate([rng.uniform(-3, 3, (n, 3)), np.ones((n, 1))], 1)
        nrm = np.concatenate([rng.normal(size=(n, 3)), np.zeros((n, 1))], 1)
        scene["objects"] = {"plane": {"pos": f32(pos), "normal": f32(nrm), "material_idx": rng.randint(0, 3, n)}}
    elif case == "one_primitive":
        kind = str(rng.choice(["disk", "sphere", "triangle"]))
        if kind == "triangle":
            v = rng.normal(size=(1, 3, 3)) * 0.6
            fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
            g = {"face": f32(np.concatenate([v, np.ones((1, 3, 1))], 2)), "normal": f32(np.concatenate([fn, [[0.0]]], 1))}
        else:
            g = {"pos": f32([[*rng.uniform(-0.3, 0.3, 3), 1.0]]), "radius": f32([rng.uniform(0.3, 0.9)])}
            if kind == "disk":
                g["normal"] = f32([[*rng.normal(size=3), 0.0]])
        g["material_idx"] = rng.randint(0, 3, 1)
        scene["objects"] = {kind: g}
        _look_at_origin(rng, scene)
    elif case == "non_finite":
        kinds = [k for k in scene["objects"] if k != "plane"]
        if not kinds:
            scene["objects"]["sphere"] = {"pos": f32([[0, 0, 0, 1], [0.5, 0, 0, 1]]), "radius": f32([0.3, 0.2]),
                                          "material_idx": np.array([0, 1])}
            kinds = ["sphere"]
        g = scene["objects"][str(rng.choice(sorted(kinds)))]
        field = "face" if "face" in g else "pos"
        a = np.array(g[field], dtype=np.float32, copy=True)
        a.reshape(a.shape[0], -1)[int(rng.randint(a.shape[0])), int(rng.randint(3))] = rng.choice([np.nan, np.inf, -np.inf])
        g[field] = a
    elif case in ("fine_view", "coarse_view", "mixed_views", "wide_occluder"):
        # a cloud in [-1, 1]^3 (rad = 1.75): with every radius r the lights' views switch from fine to coarse where
        # r / (half * dist) * 256 passes 3.2 -- half * dist falls from 1.6 rad for a light at the usable-view threshold
        # to 1.02 rad for a far one, so r = 0.028 (between 0.022 and 0.035) gives a far light the coarse view and a light
        # at the threshold the fine one
        r = {"fine_view": 0.012, "coarse_view": 0.06, "mixed_views": 0.028, "wide_occluder": 0.012}[case]
        n = int(rng.choice([300, 1500]))
        d = _tiny_discs(rng, n, 1.0, r, r * 1.0001)
        d["pos"][0, :3], d["pos"][1, :3] = [-1, -1, -1], [1, 1, 1]                     # pin the box
        scene["objects"] = {"disk": d, "plane": _floor()}
        if case == "wide_occluder":
            d["radius"][2] = 0.5
            d["pos"][2, :3] = rng.uniform(-0.3, 0.3, 3)
        rad = scene_bounds(scene)["rad"]
        first = [_unit(rng.normal(size=3)) * (1.3 * rad + 0.2) * 1.02, _unit(rng.normal(size=3)) * rad * 8.0]
        _look_at_origin(rng, scene)
    elif case == "crowd":
        # 1000 tiny discs in a cube of 0.03: a few tiles of any light's view, far more than a bin's slots
        d = _tiny_discs(rng, 1500, 1.0, 0.01, 0.05)
        d["pos"][:1000, :3] = rng.uniform(-0.015, 0.015, (1000, 3))
        d["radius"][:1000] = rng.uniform(0.004, 0.01, 1000)
        scene["objects"] = {"disk": d, "plane": _floor()}
        first = [np.array([0.3, 6.0, 0.2])]
        _look_at_origin(rng, scene, distance=3.0)
        scene["camera"]["fovy"] = float(np.deg2rad(rng.choice([8, 45])))
    elif case == "far_receivers":
        # a small cloud over a floor, in front of a wall 30 scene radii behind it: most fragments lie far outside the
        # bounding sphere -- their shadow rays leave the first light's view, start behind the second light's, and
        # cross the third one's on their way through the cloud
        d = _tiny_discs(rng, 200, 0.3, 0.02, 0.1)
        planes = {"pos": f32([[0, -0.35, 0, 1], [0, 0, -20, 1]]), "normal": f32([[0, 1, 0, 0], [0, 0, 1, 0]]),
                  "material_idx": np.array([0, 2])}
        scene["objects"] = {"disk": d, "plane": planes}
        scene["camera"].update(eye=[0.0, 0.3, 3.0, 1.0], at=[0.0, -0.2, 0.0, 1.0], up=[0.0, 1.0, 0.0, 0.0], near=0.01,
                               far=1000.0, fovy=float(np.deg2rad(70)), focal_length=1.0)
        first = [np.array([0.5, 1.5, 0.5]), np.array([-2.0, 0.4, -1.0]), np.array([0.1, 0.3, 3.5])]
    else:
        raise ValueError(case)
    return first


def random_shadow_scene(rng, force=None, finite=False):
    """A random scene for the shadow fuzzes.  `force` names a structural case of STRUCTURAL to build instead of the
    plain recipe's objects (None: one scene in three draws one).  `finite` swaps the non-finite case for the far
    receivers: the oracle restates the reference for finite scenes, the judge of the others is the all-pairs kernel."""
    scene = _random_scene(rng)
    cam = scene["camera"]
    W, H = int(rng.choice([33, 48, 64, 97, 128, 200])), int(rng.choice([17, 48, 64, 80, 128, 160]))
    cam["viewport"] = [0, 0, W, H]
    cam["near"] = max(cam["near"], 0.01)
    if force is None and rng.randint(3) == 0:
        force = str(rng.choice(STRUCTURAL))
    if finite and force == "non_finite":
        force = "far_receivers"
    first = _structure(rng, scene, force) if force else []
    many = rng.randint(10) == 0
    n_lights = int(rng.choice(MANY_LIGHTS if many else (1, 2, 3, 4, 7)))
    if many:
        OCCURRED["many_lights"] += 1
        _truncate(scene, 700)
        cam["viewport"] = [0, 0, min(W, 64), min(H, 48)]
    _set_lights(rng, scene, max(n_lights, len(first)) if force in ("mixed_views", "far_receivers") else n_lights, first)
    found, views = describe(scene)
    if force in ("crowd", "far_receivers"):
        found.add(force)                                   # by construction; the CPU test looks at the scenes themselves
    for name in found:
        OCCURRED[name] += 1
    OCCURRED["view"] += sum(v is not None for v in views)
    OCCURRED["no_view"] += sum(v is None for v in views)
    return scene


def fuzz_scenes(seed, count):
    """The scenes of a fuzz: every other one forces the structural cases in turn."""
    rng = np.random.RandomState(seed)
    for i in range(count):
        yield random_shadow_scene(rng, STRUCTURAL[(i // 2) % len(STRUCTURAL)] if i % 2 else None)


def oracle_scenes(seed, count, max_w=32, max_h=24, max_prims=400, many_w=16, many_h=12):
    """The scenes of the oracle comparisons: random finite scenes cut to at most max_w x max_h pixels (those with more
    than 8 lights to many_w x many_h) and `max_prims` primitives -- the oracle is O(pixels x lights x primitives) in
    numpy and `undecided` runs it five times."""
    rng = np.random.RandomState(seed)
    for i in range(count):
        scene = random_shadow_scene(rng, STRUCTURAL[(i // 2) % len(STRUCTURAL)] if i % 2 else None, finite=True)
        _truncate(scene, max_prims)
        many = len(scene["lights"]["pos"]) > 8
        vp = scene["camera"]["viewport"]
        scene["camera"]["viewport"] = [0, 0, min(vp[2], many_w if many else max_w), min(vp[3], many_h if many else max_h)]
        yield scene


# ---- deterministic builders -----------------------------------------------------------------------------------------
def _base(W, H, eye, at, objects, lights, fovy=45.0, far=50.0, proj=None):
    cam = {"viewport": [0, 0, W, H], "fovy": float(np.deg2rad(fovy)), "focal_length": 1.0, "eye": [*map(float, eye), 1.0],
           "at": [*map(float, at), 1.0], "up": [0.0, 0.0, 1.0, 0.0], "near": 0.01, "far": far}
    if proj:
        cam["proj_type"] = proj
    n = len(lights)
    return {"camera": cam,
            "lights": {"pos": f32([[*p, 1.0] for p in lights]), "color_idx": np.arange(n) % 2 + 1,
                       "attenuation": f32([[1, 0, 0]] * n), "ambient": f32([0.02, 0.02, 0.02])},
            "colors": f32([[0, 0, 0], [.8, .5, .4], [.3, .6, .9]]),
            "materials": {"albedo": f32([[.5, .5, .5], [.9, .3, .2], [.2, .7, .4]]),
                          "coeffs": f32([[1, 0, 0], [0.7, 0.3, 5], [0.5, 0.5, 20]])},
            "objects": objects, "tonemap": {"type": "gamma", "gamma": 0.8}}


def centre_pixel(scene):
    """(row, column) of the pixel whose ray passes through `at` (odd frames)."""
    W, H = scene["camera"]["viewport"][2:]
    assert W % 2 == 1 and H % 2 == 1
    return H // 2, W // 2


def light_above_receiver(receiver="disk"):
    """Fragments within 0.1 of the light: light 0 sits 0.05 above the centre of a large disc (or of a plane, with a
    small cloud far enough to the side that the light keeps a usable view) the camera looks at, and a small sphere
    0.06-0.10 above the light -- BEHIND it for the fragments below, and inside the 0.1 the reference accepts there: the
    centre pixel is blocked.  (No finite primitive can be that near a light with a usable view -- the view rule keeps
    the light 0.2 outside the bounding sphere -- so the plane variant has no such sphere and its centre pixel is lit.)
    Light 1 is far away."""
    sphere = {"pos": f32([[0, 0, 0.13, 1]]), "radius": f32([0.02]), "material_idx": np.array([1])}
    if receiver == "disk":
        objs = {"disk": {"pos": f32([[0, 0, 0, 1]]), "normal": f32([[0, 0, 1, 0]]), "radius": f32([2.0]),
                         "material_idx": np.array([0])}, "sphere": sphere}
    else:
        cloud = {"pos": f32([[0.6, 0.0, 0.1, 1], [0.7, 0.1, 0.2, 1], [0.65, -0.1, 0.3, 1]]),
                 "radius": f32([0.05, 0.04, 0.05]), "material_idx": np.array([1, 2, 1])}
        objs = {"plane": {"pos": f32([[0, 0, 0, 1]]), "normal": f32([[0, 0, 1, 0]]), "material_idx": np.array([0])},
                "sphere": cloud}
    return _base(33, 25, (0.0, -0.6, 0.6), (0.0, 0.0, 0.0), objs, [(0.0, 0.0, 0.05), (2.0, -3.0, 6.0)], fovy=35.0)


def occluder_behind_light(gap, occluder="disk"):
    """An occluder `gap` BEHIND the light as seen from the fragment: the centre pixel's fragment is the origin, the light
    is 1 straight above it, the occluder (a disc of radius 0.2, or a plane) faces down from 1 + gap.  The reference
    starts the shadow ray 0.1 along it and accepts hits closer than the light's distance from the fragment, so the
    occluder blocks iff gap < 0.1.  With the plane the receiver disc is the only finite primitive and the light keeps a
    usable view; with the disc it does not."""
    recv = {"pos": f32([[0, 0, 0, 1]]), "normal": f32([[0, 0, 1, 0]]), "radius": f32([0.3]), "material_idx": np.array([0])}
    z = 1.0 + gap
    if occluder == "disk":
        recv = {k: np.concatenate([v, w]) for (k, v), w in zip(recv.items(), (f32([[0, 0, z, 1]]), f32([[0, 0, -1, 0]]),
                                                                               f32([0.2]), np.array([1])))}
        objs = {"disk": recv}
    else:
        objs = {"disk": recv, "plane": {"pos": f32([[0, 0, z, 1]]), "normal": f32([[0, 0, -1, 0]]),
                                        "material_idx": np.array([1])}}
    return _base(33, 25, (0.0, -2.0, 0.9), (0.0, 0.0, 0.0), objs, [(0.0, 0.0, 1.0)], fovy=20.0)


def coincident_tie():
    """The lowest-index tie rule.  Discs 0 and 1 are coplanar and coincident, between the light and receiver disc 2: the
    fragment at the frame's centre lies on the third primitive and is blocked, whichever of the two is named.  Spheres
    3 and 4 coincide as well and the camera sees them from the side away from the light: the shadow ray of a fragment
    on them passes through its own sphere, both hit at the same distance, the lowest index is the blocker -- which is the
    fragment's own primitive `win` = 3, so the reference calls it lit (torch/renderer.py:306-314)."""
    disk = {"pos": f32([[0, 0, 0.5, 1], [0, 0, 0.5, 1], [0, 0, 0, 1]]), "normal": f32([[0, 0, 1, 0]] * 3),
            "radius": f32([0.25, 0.25, 1.5]), "material_idx": np.array([1, 2, 0])}
    sphere = {"pos": f32([[0.8, 0, 0.3, 1]] * 2), "radius": f32([0.25, 0.25]), "material_idx": np.array([1, 2])}
    return _base(33, 25, (0.0, -3.0, 0.35), (0.0, 0.0, 0.0), {"disk": disk, "sphere": sphere}, [(0.0, 0.6, 4.0)], fovy=40.0)


def ladder_scene(n_lights=64):
    """64 lights on a ring around a small cloud of spheres over a plane, seen from above: every light throws the
    cloud's shadow onto another part of the plane, so every bit of the visibility word is set at some hit pixels and
    clear at others.  `n_lights` truncates the ring."""
    rng = np.random.RandomState(64)
    n = 40
    sphere = {"pos": f32(np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(0.2, 0.9, (n, 1)), np.ones((n, 1))], 1)),
              "radius": f32(rng.uniform(0.08, 0.2, n)), "material_idx": rng.randint(0, 3, n)}
    plane = {"pos": f32([[0, 0, 0, 1]]), "normal": f32([[0, 0, 1, 0]]), "material_idx": np.array([0])}
    ang = 2.0 * np.pi * np.arange(64) / 64.0
    lights = [(3.0 * np.cos(a), 3.0 * np.sin(a), 2.5 + 0.01 * i) for i, a in enumerate(ang)][:n_lights]
    # far = 6.7: the plane's fragments in the frame's corners lie beyond it -- background pixels
    return _base(33, 25, (0.3, -1.0, 6.0), (0.0, 0.0, 0.3), {"sphere": sphere, "plane": plane}, lights, fovy=35.0, far=6.7)


def deterministic_scenes():
    """name -> (scene, expectation): expectation = (light, 'blocked' | 'lit') at the centre pixel, or None."""
    out = {}
    for receiver in ("disk", "plane"):
        out[f"light_above_{receiver}"] = (light_above_receiver(receiver), (0, "blocked" if receiver == "disk" else "lit"))
    for occluder in ("disk", "plane"):
        for gap in (0.05, 0.0999, 0.1002):
            out[f"{occluder}_{gap}_behind_light"] = (occluder_behind_light(gap, occluder), (0, "blocked" if gap < 0.1 else "lit"))
    out["coincident_tie"] = (coincident_tie(), (0, "blocked"))
    return out


# ---- the oracle side --------------------------------------------------------------------------------------------------
def oracle_input(scene):
    """The scene as the oracle takes it: the fp32 values the device arrays hold, in float64."""
    from surf_renderer_amd.scene import scene_to_numpy
    sc = scene_to_numpy(scene, round_fp32=True)
    if "proj_type" in scene["camera"]:
        sc["camera"]["proj_type"] = scene["camera"]["proj_type"]
    return sc


def _hangs_on_an_in_plane_ray(scene, pos, nearest):
    """(L, n) bool for fragments `pos` (n,3) on primitives `nearest`: a flat primitive holds fragment and light in its
    plane to within the perturbation of `undecided` -- its hit distance along the shadow ray is 0 / 0 -- and the pair's
    visibility is one thing if that primitive is missed and another if it is the nearest blocker."""
    from oracle import np_oracle, np_oracle_tch
    lpos = np.asarray(scene["lights"]["pos"], dtype=np.float64)[:, :3]
    objs = {k: {f: np.asarray(v, dtype=np.float64) if f != "material_idx" else np.asarray(v) for f, v in g.items()}
            for k, g in scene["objects"].items()}
    segs, total = np_oracle._segments(objs)
    frag_in, light_in = np.zeros((total, pos.shape[0]), dtype=bool), np.zeros((total, lpos.shape[0]), dtype=bool)
    for kind, start, count, g in segs:
        if kind == "sphere":
            continue
        n = np_oracle_tch.unit3(g["normal"][:, :3])
        q = g["face"][:, 0, :3] if kind == "triangle" else g["pos"][:, :3]
        off, size = np.sum(q * n, axis=1)[:, None], np.linalg.norm(q, axis=1)[:, None]
        frag_in[start:start + count] = np.abs(n @ pos.T - off) <= 1e-9 * (np.linalg.norm(pos, axis=1)[None, :] + size) + 1e-10
        light_in[start:start + count] = np.abs(n @ lpos.T - off) <= 1e-9 * (np.linalg.norm(lpos, axis=1)[None, :] + size) + 1e-10
    out = np.zeros((lpos.shape[0], pos.shape[0]), dtype=bool)
    cols = np.arange(pos.shape[0])
    with np.errstate(all="ignore"):
        for l in np.nonzero(light_in.any(axis=0))[0]:
            deg = frag_in & light_in[:, l][:, None]
            if not deg.any():
                continue
            v = lpos[l][None, :] - pos
            dist = np.sqrt(np.sum(v ** 2, axis=-1))
            dirs = v / dist[:, None]
            t = np_oracle_tch._hits_general(segs, total, pos + 0.1 * dirs, dirs)
            t = np.where((t > 0) & (t < dist[None, :]), t, np.inf)
            lit = []
            for fill in (np.inf, 0.0):                      # the in-plane primitives missed / hit before everything else
                tt = np.where(deg, fill, t)
                blocker = np.argmin(tt, axis=0)
                lit.append(~np.isfinite(tt[blocker, cols]) | (blocker == nearest))
            out[l] = lit[0] != lit[1]
    return out


def undecided(scene, res):
    """(L, H, W) bool: the (light, pixel) pairs an oracle comparison leaves out.  `res` is the oracle's own frame
    (np_oracle_tch.render(scene, shadow=True)); its fragment positions are moved to pos (1 +- 1e-9) +- 1e-10 in four
    fixed sign patterns and np_oracle_tch.light_visibility runs again: a pair whose bit flips in any of them hangs on
    less than that, and is undecided.  So is a pair that hangs on a shadow ray INSIDE the plane of a disc, plane or
    triangle (a light drawn into a primitive's plane, seen from a fragment of that primitive, with a real blocker on the
    way): the ray's distance to such a primitive is 0 / 0 -- rounding noise in the oracle, in the kernels and in the
    reference alike -- and moving the fragment OFF the plane, as all four patterns do, replaces the noise by a clean hit
    at the light instead of sampling it (_hangs_on_an_in_plane_ray).  Background pixels are never undecided."""
    from oracle import np_oracle_tch
    H, W = res["depth"].shape
    hit = (res["depth"] <= scene["camera"]["far"]).reshape(-1)
    pos = res["pos"].reshape(-1, 3)[hit]
    part = {"nearest": res["nearest"].reshape(-1)[hit]}
    base = res["visibility"].reshape(res["visibility"].shape[0], -1)[:, hit]
    flips = np.zeros_like(base)
    for rel, ab in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        part["pos"] = pos * (1.0 + rel * 1e-9) + ab * 1e-10
        flips |= np_oracle_tch.light_visibility(scene, part) != base
    flips |= _hangs_on_an_in_plane_ray(scene, pos, part["nearest"])
    out = np.zeros((base.shape[0], H * W), dtype=bool)
    out[:, hit] = flips
    return out.reshape(-1, H, W)


def unpack_bits(words, n_lights):
    """(L, ...) bool from the int64 visibility words of the Python layer (bit 63 is the sign bit)."""
    u = np.ascontiguousarray(words).view(np.uint64)
    return np.stack([(u >> np.uint64(l)) & np.uint64(1) for l in range(n_lights)]).astype(bool)


# ---- the device side ------------------------------------------------------------------------------------------------
def shadow_both_ways(scene, rows=None, **kw):
    """(binned, all-pairs) results of the shadow pass over the same primary frame (or row slab of it): per kernel
    (image, visibility words, depth)."""
    import torch
    from surf_renderer_amd import renderer
    buf = renderer.flatten_scene(scene, "cuda:0")
    cam = renderer.camera_struct(scene["camera"], "torch")
    out = []
    for all_pairs in (False, True):
        image, depth, nearest = renderer.render_buffers(buf, cam, rows=rows, shading="torch", **kw)
        vis = renderer.shadow_pass(buf, cam, rows, image, depth, nearest, kw.get("double_sided", False),
                                   kw.get("use_quartic", False), all_pairs=all_pairs)
        torch.cuda.synchronize()
        out.append((image.clone(), vis.clone(), depth.clone()))
    return out
