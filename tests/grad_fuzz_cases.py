"""Shared by the gradient fuzzers (tests/test_hip_aux_grad.py, tests/test_hip_grad_fuzz.py) and pinned on the CPU by
tests/test_grad_fuzz_cases_cpu.py: random mixed scenes, cameras with the hazards that break camera gradients, batches of
views whose overrides differ from view to view, the batch gradient definition for such overrides, and the masks that
isolate the primitives winning the fewest pixels.  Nothing here needs a GPU or imports the package: every rule that
redraws a scene is decided by the fp64 numpy oracle (oracle/np_oracle_tch.render), never by a GPU result.

Frames of the batches are W in {24, 40, 72} x H in {10, 22, 36}: partial 64-lane and 4-row workgroups and partial
16 x 16 tiles (the header of tests/views_cases.py)."""
import copy
import os

import numpy as np

from grad_cases import RUN_TO_RUN, TCH_KEYS
from oracle import np_oracle_tch, torch_oracle
from oracle.torch_oracle import LEAF_KEYS, OUTPUTS
from views_cases import get_leaf, set_leaf, view_scene

DEFAULT_CAMERA_SEED, DEFAULT_N_CAMERA = 2711, 24
DEFAULT_VIEWS_SEED, DEFAULT_N_VIEWS = 2713, 12
# SRH_FUZZ_CAMGRAD_SEED / _SCENES and SRH_FUZZ_VIEWSGRAD_SEED / _BATCHES: one-off campaigns with other seeds
# (profiles/grad_fuzz.txt), the convention of SRH_FUZZ_BWD_SEED
CAMERA_SEED = int(os.environ.get("SRH_FUZZ_CAMGRAD_SEED", DEFAULT_CAMERA_SEED))
N_CAMERA = int(os.environ.get("SRH_FUZZ_CAMGRAD_SCENES", DEFAULT_N_CAMERA))
VIEWS_SEED = int(os.environ.get("SRH_FUZZ_VIEWSGRAD_SEED", DEFAULT_VIEWS_SEED))
N_VIEWS = int(os.environ.get("SRH_FUZZ_VIEWSGRAD_BATCHES", DEFAULT_N_VIEWS))
# how many of them the masked comparison (small winners) takes; SRH_FUZZ_MASKED_SCENES / _BATCHES widen a campaign
N_MASKED_CAMERA = int(os.environ.get("SRH_FUZZ_MASKED_SCENES", 8))
N_MASKED_VIEWS = int(os.environ.get("SRH_FUZZ_MASKED_BATCHES", 4))

EYE_DISTANCES = (0.7, 4.0, 9.0)                 # 0.7: inside the cloud (primitive centres fill [-1.5, 1.5]^3)
AT_DISTANCES = (0.05, 1.0, None)                # None: the whole way to the scene's centre
NEAR_PARALLEL_DEG = 5.0
MIN_CROSS = 1e-3                                # |unit(up) x unit(at - eye)| below this is redrawn: never exactly parallel
BIG_FRAME = (72, 172)                           # 2 x 43 = 86 workgroups of 64 x 4: one more than kCamFinishRows = 85
VIEW_WIDTHS, VIEW_HEIGHTS = (24, 40, 72), (10, 22, 36)
VIEW_COUNTS = (1, 2, 3, 5, 7)
BATCH_KINDS = ("1", "2", "3", "n", "n+3", "0")
HIT_RANGE = (0.05, 1.0)
MIN_LIGHT_DISTANCE = 1e-3


def _fuzz_scene(rng, ortho):
    """All four primitive types, a random camera (perspective or orthographic) outside the cloud, small frames."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)          # noqa: E731
    W, H = int(rng.choice([32, 48, 64])), int(rng.choice([24, 40, 56]))
    eye = rng.normal(size=3)
    back = eye / np.linalg.norm(eye)
    eye = back * rng.choice([4.0, 6.0, 9.0])
    cam = {"viewport": [0, 0, W, H], "fovy": float(np.deg2rad(rng.choice([30, 45, 70]))),
           "focal_length": float(rng.choice([1.0, 3.0])), "eye": [*map(float, eye), 1.0],
           "at": [*map(float, rng.normal(size=3) * 0.2), 1.0], "up": [*map(float, rng.normal(size=3)), 0.0],
           "near": 0.1, "far": 100.0}
    if ortho:
        cam["proj_type"] = "ortho"
    objs = {}
    for k in rng.permutation(["disk", "triangle", "sphere", "plane"]):
        n = int(rng.choice([1, 5, 40])) if k != "plane" else 1
        pos = np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)), np.ones((n, 1))], 1)
        nrm = np.concatenate([rng.normal(size=(n, 3)), np.zeros((n, 1))], 1)
        mat = rng.randint(0, 3, n)
        if k == "disk":
            objs[k] = {"pos": f32(pos), "normal": f32(nrm), "material_idx": mat,
                       "radius": f32(np.exp(rng.uniform(np.log(0.05), np.log(1.2), n)))}
        elif k == "sphere":
            objs[k] = {"pos": f32(pos), "radius": f32(np.exp(rng.uniform(np.log(0.1), np.log(0.8), n))),
                       "material_idx": mat}
        elif k == "plane":                              # a wall behind the cloud, roughly facing the camera
            objs[k] = {"pos": f32(np.concatenate([-3.0 * back, [1.0]])[None]),
                       "normal": f32(np.concatenate([back + 0.2 * rng.normal(size=3), [0.0]])[None]),
                       "material_idx": mat}
        else:
            c = rng.uniform(-1.5, 1.5, (n, 1, 3))
            v = c + rng.normal(size=(n, 3, 3)) * np.exp(rng.uniform(np.log(0.1), np.log(0.8), (n, 1, 1)))
            fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) * rng.choice([-1, 1], (n, 1))
            objs[k] = {"face": f32(np.concatenate([v, np.ones((n, 3, 1))], 2)),
                       "normal": f32(np.concatenate([fn, np.zeros((n, 1))], 1)), "material_idx": mat}
    return {"camera": cam,
            "lights": {"pos": f32([[3, 4, 5, 1], [-4, 2, 3, 1]]), "color_idx": np.array([1, 2]),
                       "attenuation": f32([[1, 0, 0], [0.5, 0.1, 0.01]]), "ambient": f32([0.01, 0.02, 0.01])},
            "colors": f32([[0, 0, 0], [.8, .5, .4], [.3, .6, .9]]),
            "materials": {"albedo": f32([[.5, .5, .5], [.9, .3, .2], [.2, .7, .4]]),
                          "coeffs": f32([[1, 0, 0], [0.7, 0.3, 5], [0.5, 0.5, 20]])},
            "objects": objs, "tonemap": {"type": "gamma", "gamma": 0.8}}


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _f32(a):
    """The float32 roundings of `a`, as float64: the values the device arrays hold."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _unit(v):
    return v / np.linalg.norm(v)


def leaf_keys(scene):
    """The flat keys of the scene's differentiable leaves under torch shading: LEAF_KEYS of every kind present, TCH_KEYS."""
    return [f"{kind}.{name}" for kind in scene["objects"] for name in LEAF_KEYS[kind]] + list(TCH_KEYS)


def fp64_scene(scene):
    """Copy of a _fuzz_scene with its float32 leaves as float64 ndarrays of the same values (the camera is kept as it is:
    list-typed vectors stay lists)."""
    sc = copy.deepcopy(scene)
    for key in leaf_keys(sc):
        set_leaf(sc, key, _f32(get_leaf(sc, key)))
    return sc


def truncate_objects(scene, most):
    """Keep the first `most` primitives of every kind (in place): the large frames stay cheap for the fp64 oracle."""
    for grp in scene["objects"].values():
        for name in list(grp):
            grp[name] = grp[name][:most]


def kind_ranges(scene):
    """[(kind, first global index, count)] in the scene's own order."""
    out, start = [], 0
    for kind, grp in scene["objects"].items():
        count = len(grp["material_idx"])
        out.append((kind, start, count))
        start += count
    return out


def locate(scene, index):
    """(kind, row within the kind) of the global primitive `index`."""
    for kind, start, count in kind_ranges(scene):
        if start <= index < start + count:
            return kind, index - start
    raise IndexError(index)


def random_upstream(rng, shape, outputs):
    """{output: float32 values in [-1, 1) of `shape` (+ (3,))}, as float64."""
    return {k: _f32(rng.uniform(-1, 1, size=tuple(shape) + (() if k == "depth" else (3,)))) for k in outputs}


def random_outputs(rng, allowed=OUTPUTS):
    """A random non-empty subset of `allowed`, in OUTPUTS order."""
    keys = [k for k in allowed if rng.randint(2)]
    return tuple(keys) if keys else (str(allowed[rng.randint(len(allowed))]),)


# ---- cameras ---------------------------------------------------------------------------------------------------------------
def hazard_camera(rng, cam, back, target, eye_distance=None, away=False):
    """`cam` with eye, at and up redrawn (a copy): the eye `back` * a distance of EYE_DISTANCES, `at` on the line from the
    eye to `target` at a distance of AT_DISTANCES (away: the same distance on the far side of the eye), `up` a random
    un-normalised vector, in one case in four within NEAR_PARALLEL_DEG of the view direction but never closer than
    MIN_CROSS to parallel; half the time all three are Python lists of float64 that float32 does not hold, else float64
    arrays of float32 values."""
    cam = dict(cam)
    dist = float(EYE_DISTANCES[rng.randint(3)]) if eye_distance is None else float(eye_distance)
    eye = _unit(np.asarray(back, dtype=np.float64)) * dist
    to = np.asarray(target, dtype=np.float64) - eye
    d_at = AT_DISTANCES[rng.randint(3)]
    at = eye + to if d_at is None else eye + _unit(to) * d_at
    if away:
        at = 2.0 * eye - at
    view = _unit(at - eye)
    close = rng.randint(4) == 0
    while True:
        if close:
            ang = np.deg2rad(rng.uniform(0.3, NEAR_PARALLEL_DEG))
            perp = rng.normal(size=3)
            perp = _unit(perp - view * np.dot(perp, view))
            up = np.cos(ang) * view * rng.choice([-1.0, 1.0]) + np.sin(ang) * perp
        else:
            up = _unit(rng.normal(size=3))
        if np.linalg.norm(np.cross(up, view)) >= MIN_CROSS:
            break
    up = up * float(rng.choice([0.3, 2.5, 7.0]))
    vecs = {"eye": np.append(eye, 1.0), "at": np.append(at, 1.0), "up": np.append(up, 0.0)}
    if rng.randint(2):
        cam.update({k: [float(x) for x in v] for k, v in vecs.items()})
    else:
        cam.update({k: _f32(v) for k, v in vecs.items()})
    return cam


def camera_hazards(cam):
    """The hazard classes a camera falls into, measured on the float32 values the renderer holds."""
    eye, at, up = (np_oracle_tch.cam_vec(cam[k])[:3] for k in ("eye", "at", "up"))
    view = at - eye
    out = {"ortho" if np_oracle_tch.is_ortho(cam) else "perspective"}
    if np.linalg.norm(eye) < 1.0:
        out.add("inside")
    if np.linalg.norm(view) < 0.1:
        out.add("short_at")
    cross = np.linalg.norm(np.cross(_unit(up), _unit(view)))
    assert cross >= 0.5 * MIN_CROSS, cross
    if cross <= np.sin(np.deg2rad(NEAR_PARALLEL_DEG)) * 1.001:
        out.add("near_parallel_up")
    if isinstance(cam["up"], list):
        out.add("lists")
        assert any(float(np.float32(x)) != x for k in ("eye", "at", "up") for x in cam[k])
    if abs(np.linalg.norm(up) - 1.0) > 0.1:
        out.add("non_unit_up")
    return out


def camera_scene(rng, big=False):
    """_fuzz_scene plus the camera hazards (hazard_camera), perspective or orthographic, near = 0.1 so that a missed sphere
    is never a hit; float64 ndarray leaves of float32 values.  big: the frame is BIG_FRAME -- more workgroups than the
    camera finish kernel has rows -- with at most five primitives of a kind."""
    ortho = bool(rng.randint(2))
    scene = _fuzz_scene(rng, ortho)
    cam = scene["camera"]
    if big:
        truncate_objects(scene, 5)
        cam["viewport"] = [0, 0, *BIG_FRAME]
    assert cam["near"] == 0.1
    scene["camera"] = hazard_camera(rng, cam, cam["eye"][:3], cam["at"][:3])
    return fp64_scene(scene)


def near_parallel_up_camera(cam, degrees=0.1):
    """`cam` with an un-normalised `up` (float32 values) `degrees` from its view direction: |unit(up) x unit(at - eye)|
    = 1.7e-3 at a tenth of a degree, so the 3e-10 inside the reference's norm is 1e-4 of the cross product's squared
    length.  The regression case of the camera finish kernel's chain rule (profiles/grad_fuzz.txt)."""
    eye, at = (np_oracle_tch.cam_vec(cam[k])[:3] for k in ("eye", "at"))
    view = _unit(at - eye)
    perp = _unit(np.cross(view, [0.3, 1.0, 0.2]))
    ang = np.deg2rad(degrees)
    return dict(cam, up=_f32(np.append(2.5 * (np.cos(ang) * view + np.sin(ang) * perp), 0.0)))


def check_frame(scene, ref, away=False):
    """The redraw rules, on the fp64 numpy oracle's frame `ref` of `scene`: None if the frame is kept, else the reason.
    A look-away view must hit nothing; every other view hits between 5 % and all of its pixels, at least two primitive
    kinds win pixels, and no light lies within MIN_LIGHT_DISTANCE of a fragment."""
    hit = ref["depth"] <= scene["camera"]["far"]
    if away:
        return "the look-away view hits something" if hit.any() else None
    if not HIT_RANGE[0] <= hit.mean() <= HIT_RANGE[1]:
        return f"hit fraction {hit.mean():.3f}"
    won = {locate(scene, int(i))[0] for i in np.unique(ref["nearest"][hit])}
    if len(won) < 2:
        return f"only {sorted(won)} win pixels"
    lpos = np.asarray(get_leaf(scene, "lights.pos"), dtype=np.float64)[:, :3]
    gap = np.linalg.norm(ref["pos"][hit][:, None, :] - lpos[None, :, :], axis=-1).min()
    if gap < MIN_LIGHT_DISTANCE:
        return f"a light {gap:.2g} from a fragment"
    return None


def camera_cases(seed=None, count=None):
    """The camera fuzz: `count` dicts {scene, kw, shadow, outputs, g, slab, big, ref, hazards, redraws} from one stream.
    kw = double_sided / use_quartic; g = upstream gradients of the outputs in the loss; slab = the row the frame is also
    split at (every fourth scene; not a multiple of 4) or None; big: every sixth scene; ref = np_oracle_tch.render(scene,
    **kw), which decided the redraws (check_frame)."""
    rng = np.random.RandomState(CAMERA_SEED if seed is None else seed)
    cases, redraws = [], 0
    while len(cases) < (N_CAMERA if count is None else count):
        i = len(cases)
        big = i % 6 == 5
        scene = camera_scene(rng, big)
        kw = {"double_sided": bool(rng.randint(2)), "use_quartic": bool(rng.randint(2))}
        shadow = bool(rng.randint(2))
        outputs = random_outputs(rng)
        W, H = scene["camera"]["viewport"][2:]
        g = random_upstream(rng, (H, W), outputs)
        ref = np_oracle_tch.render(scene, **kw)
        if check_frame(scene, ref) is not None:
            redraws += 1
            continue
        r = H // 2 + 1
        cases.append(dict(scene=scene, kw=kw, shadow=shadow, outputs=outputs, g=g, big=big, ref=ref,
                          slab=(r if r % 4 else r + 1) if i % 4 == 3 else None, hazards=camera_hazards(scene["camera"]),
                          redraws=redraws))
        redraws = 0
    return cases


# ---- batches of views --------------------------------------------------------------------------------------------------------
def _jitter_leaf(rng, key, base):
    """The base leaf jittered and rounded to float32: positions, normals and vertices move (w stays), every other leaf
    is scaled (zeros stay zeros: a material without a specular term keeps none)."""
    field = key.split(".")[-1]
    if key == "lights.pos" or (field in ("pos", "normal", "face") and not key.startswith("lights")):
        off = rng.uniform(-1, 1, size=base.shape) * (0.5 if key == "lights.pos" else 0.15)
        off[..., 3] = 0.0
        return _f32(base + off)
    return _f32(base * rng.uniform(0.8, 1.2, size=base.shape))


def batch_step(n, batch):
    """Views per backward launch of render_views(batch=batch) on n views."""
    return min(batch if batch > 0 else 256, 256, n)


def views_batch(rng, n=None, batch_kind=None):
    """(scene, cameras, overrides_by_view, batch, flags): a _fuzz_scene at a frame of VIEW_WIDTHS x VIEW_HEIGHTS seen by n
    hazard cameras (n of VIEW_COUNTS, `batch` of BATCH_KINDS; drawn here unless given).  overrides_by_view[v] maps leaf
    keys to view v's own values; per key of leaf_keys(scene) the table holds no override, one for every view, or one for
    a random non-empty proper subset of the views.  flags: n, batch_kind, aux, shadow, double_sided, use_quartic, ortho,
    outputs (the outputs in the loss), g (their upstream gradients, (n, H, W[, 3])), stacked (the every-view keys given
    as slices of one parent tensor), partial ({key: views that override it}), shared_camera (None | 'up' | 'eye': one
    tensor for all views) and away (the view that looks away from the scene, or None).  Nothing is checked here: see
    views_cases."""
    n = int(VIEW_COUNTS[rng.randint(len(VIEW_COUNTS))]) if n is None else int(n)
    kind = BATCH_KINDS[rng.randint(len(BATCH_KINDS))] if batch_kind is None else batch_kind
    batch = {"n": n, "n+3": n + 3}.get(kind) or int(kind)
    ortho = rng.randint(3) == 0
    scene = _fuzz_scene(rng, ortho)
    base_cam = scene["camera"]
    base_cam["viewport"] = [0, 0, int(rng.choice(VIEW_WIDTHS)), int(rng.choice(VIEW_HEIGHTS))]
    scene = fp64_scene(scene)
    back, target = np.asarray(base_cam["eye"][:3]), np.asarray(base_cam["at"][:3])
    shared_camera = ("up", "eye")[rng.randint(2)] if rng.randint(3) == 0 else None
    away = int(rng.randint(n)) if (n >= 2 and shared_camera != "eye" and rng.randint(3) == 0) else None
    cameras = []
    for v in range(n):
        cameras.append(hazard_camera(rng, base_cam, _unit(back) + 0.35 * rng.normal(size=3), target,
                                     eye_distance=9.0 if v == away else None, away=v == away))
    if shared_camera is not None:
        for cam in cameras[1:]:
            cam[shared_camera] = copy.copy(cameras[0][shared_camera])
    scene["camera"] = dict(cameras[0])
    overrides = [{} for _ in range(n)]
    stacked, partial = set(), {}
    for key in leaf_keys(scene):
        mode = rng.randint(3)                       # 0: none, 1: every view, 2: a proper subset
        base = np.asarray(get_leaf(scene, key), dtype=np.float64)
        if mode == 1:
            views = range(n)
            if rng.randint(2):
                stacked.add(key)
        elif mode == 2 and n >= 2:
            views = sorted(rng.choice(n, size=rng.randint(1, n), replace=False).tolist())
            partial[key] = views
        else:
            views = ()
        for v in views:
            overrides[v][key] = _jitter_leaf(rng, key, base)
    aux = bool(rng.randint(2))
    flags = dict(n=n, batch_kind=kind, aux=aux, shadow=bool(rng.randint(2)), double_sided=bool(rng.randint(2)),
                 use_quartic=bool(rng.randint(2)), ortho=ortho, stacked=stacked, partial=partial,
                 shared_camera=shared_camera, away=away)
    flags["outputs"] = random_outputs(rng, OUTPUTS if aux else OUTPUTS[:2])
    W, H = base_cam["viewport"][2:]
    flags["g"] = random_upstream(rng, (n, H, W), flags["outputs"])
    return scene, cameras, overrides, batch, flags


def shade_kw(flags):
    return {"double_sided": flags["double_sided"], "use_quartic": flags["use_quartic"]}


def batch_scenes(scene, cameras, overrides):
    """The scene each view renders, for the oracles."""
    return [view_scene(scene, cameras[v], overrides[v]) for v in range(len(cameras))]


def cancelling_sums(case, refs=None):
    """[(view, leaf key, ratio)] of the batch's gradient sums that two fp32-atomic accumulations need not agree on within
    RUN_TO_RUN: per view and leaf, the largest sum over the pixels of |per-pixel term| (torch_oracle.gradient_terms_tch
    on the numpy oracle's frame, with its shadow rays where the batch has them) x 2^-23 -- what an fp32 accumulation of
    the terms in an arbitrary order is uncertain by -- over RUN_TO_RUN x the array's largest entry, where that ratio
    exceeds 1.  render_views and render() add a view's terms in different orders, so such a sum may differ between them
    by more than the bound their comparison holds an own tensor to (tests/test_hip_grad_fuzz.py), and a shared leaf's
    bound is the sum of its views' (profiles/grad_fuzz.txt: seed 9102, batch 23)."""
    scene, cameras, overrides, _, flags = case
    out = []
    for v, sc in enumerate(batch_scenes(scene, cameras, overrides)):
        if v == flags["away"]:
            continue
        shadow = flags["shadow"] and "image" in flags["outputs"]
        ref = refs[v] if refs is not None and not shadow else np_oracle_tch.render(sc, shadow=shadow, **shade_kw(flags))
        total, absolute = torch_oracle.gradient_terms_tch(
            sc, **{"grad_" + k: a[v] for k, a in flags["g"].items()}, ref=ref,
            visibility=ref["visibility"] if shadow else None, **shade_kw(flags))
        for key, a in absolute.items():
            ratio = a.max() * 2.0 ** -23 / max(RUN_TO_RUN * np.abs(total[key]).max(), 1e-300)
            if ratio > 1.0:
                out.append((v, key, float(ratio)))
    return out


def views_cases(seed=None, count=None, cancellation_rule=True):
    """The batch fuzz: `count` tuples of views_batch from one stream, n and the batch kind stratified (a permutation of
    VIEW_COUNTS and of BATCH_KINDS, cycled, so that twelve batches hold each of them), redrawn until every view passes
    check_frame on the numpy oracle's frame and -- unless cancellation_rule is off -- no gradient sum of the batch
    cancels harder than fp32 atomics resolve (cancelling_sums).  flags gains 'redraws' (check_frame) and
    'redraws_cancelling'."""
    rng = np.random.RandomState(VIEWS_SEED if seed is None else seed)
    counts, kinds = rng.permutation(len(VIEW_COUNTS)), rng.permutation(len(BATCH_KINDS))
    cases, redraws, cancelling = [], 0, 0
    while len(cases) < (N_VIEWS if count is None else count):
        i = len(cases)
        case = views_batch(rng, VIEW_COUNTS[counts[i % len(counts)]], BATCH_KINDS[kinds[i % len(kinds)]])
        scene, cameras, overrides, _, flags = case
        scenes = batch_scenes(scene, cameras, overrides)
        refs = [np_oracle_tch.render(sc, **shade_kw(flags)) for sc in scenes]
        if any(check_frame(sc, refs[v], v == flags["away"]) is not None for v, sc in enumerate(scenes)):
            redraws += 1
            continue
        if cancellation_rule and cancelling_sums(case, refs):
            cancelling += 1
            continue
        flags["redraws"], flags["redraws_cancelling"] = redraws, cancelling
        redraws = cancelling = 0
        cases.append(case)
    return cases


def mixed_batch_gradients(per_view, own_by_view):
    """views_cases.batch_gradients for overrides that differ per view: per-view gradient dicts and, per view, the keys
    that view overrides -> (shared, own).  A key view v overrides goes to own[key][v] (own[key] is a dict by view);
    otherwise view v's gradient is added to shared[key], which exists for every key some view leaves alone."""
    shared, own = {}, {}
    for v, g in enumerate(per_view):
        for k, a in g.items():
            if k in own_by_view[v]:
                own.setdefault(k, {})[v] = a
            else:
                shared[k] = shared.get(k, 0.0) + a
    return shared, own


def winner_masks(nearest, depth, far, k=3):
    """[(global primitive index, boolean pixel mask)] of the k primitives that win the fewest pixels, at least one each
    (ties: the lower index), among the hit pixels depth <= far.  Works on a frame or a stack of frames alike."""
    nearest, hit = np.asarray(nearest), np.asarray(depth) <= far
    idx, counts = np.unique(nearest[hit], return_counts=True)
    order = np.lexsort((idx, counts))[:k]
    return [(int(idx[j]), hit & (nearest == idx[j])) for j in order]


def mask_upstream(g, mask):
    """The upstream gradients zeroed outside `mask`."""
    return {k: np.where(mask if a.ndim == mask.ndim else mask[..., None], a, 0.0) for k, a in g.items()}

