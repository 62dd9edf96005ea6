"""Shared by the multi-view gradient tests: the v1 fixtures (oracle/golden_v1.py) as per-view scenes, the
batches several test modules render (the five-view batch, the orthographic pair, the shadow fixture with per-view
lights), and the per-view gradient oracle summed / stacked the way a batch's gradients are defined -- a leaf all views
share gets the sum over the views, a leaf a view overrides the gradient of that view alone."""
import copy
import json
import os

import numpy as np

from conftest import GOLDEN_DIR
from oracle import torch_oracle
from oracle.golden_io import unpack_scene

V1_CASES = ["v1_views_grad_phong", "v1_views_grad_phong_ds_quartic"]
V1_PER_VIEW = ("disk.pos", "lights.pos")
W, H = 72, 22                                   # partial 64-lane workgroup in x, partial 4-row workgroup in y
# the five-view batch 'everything at once': per-view discs and lights, view AWAY3 looks away from the scene
OWN3 = ("disk.pos", "disk.normal", "lights.pos")
KW3 = {"double_sided": True, "use_quartic": True}
EYES3 = [[0.3, 1.0, 10.0, 1.0], [2.5, -0.5, 9.0, 1.0], [0.0, 0.5, 30.0, 1.0], [-3.0, 2.0, 8.5, 1.0], [1.0, 3.0, 9.5, 1.0]]
ATS3 = [[0.0, 0.0, 0.0, 1.0], [0.5, 0.2, 0.0, 1.0], [0.0, 0.5, 60.0, 1.0], [-0.5, 0.3, -1.0, 1.0], [0.2, -0.2, 0.5, 1.0]]
AWAY3 = 2


def get_leaf(scene, key):
    a, _, b = key.partition(".")
    return scene[a] if not b else (scene[a][b] if a in ("lights", "materials") else scene["objects"][a][b])


def set_leaf(scene, key, value):
    """Assign the leaf with the flat key '<kind>.<field>' | 'lights.pos' | 'colors' | 'materials.albedo' | ..."""
    a, _, b = key.partition(".")
    if not b:
        scene[a] = value
    elif a in ("lights", "materials"):
        scene[a][b] = value
    else:
        scene["objects"][a][b] = value


def view_scene(scene, camera=None, leaves=None):
    """Deep copy of `scene` with camera fields and leaves replaced: the scene one view of a batch renders."""
    sc = copy.deepcopy(scene)
    sc["camera"].update(camera or {})
    for key, value in (leaves or {}).items():
        set_leaf(sc, key, np.asarray(value, dtype=np.float64))
    return sc


def load_v1(case):
    """(npz, base scene, [camera overrides per view], [leaf overrides per view], render kwargs)"""
    npz = np.load(os.path.join(GOLDEN_DIR, case + ".npz"), allow_pickle=False)
    scene = unpack_scene(npz)
    n = npz["cameras/eye"].shape[0]
    cams = [{"eye": npz["cameras/eye"][v].astype(np.float64), "at": npz["cameras/at"][v].astype(np.float64)}
            for v in range(n)]
    own = [{k: npz["view/" + k][v].astype(np.float64) for k in V1_PER_VIEW} for v in range(n)]
    return npz, scene, cams, own, json.loads(str(npz["kwargs"]))


def batch_gradients(per_view, own_keys):
    """Per-view gradient dicts -> (shared: sum over views of every other key, own: {key: [per view]})."""
    shared = {}
    for g in per_view:
        for k, a in g.items():
            if k not in own_keys:
                shared[k] = shared.get(k, 0.0) + a
    return shared, {k: [g[k] for g in per_view] for k in own_keys}


def oracle_batch_tch(scenes, g, refs, own_keys, visibility=None, camera=False, **kw):
    """gradients_tch per view on the upstreams {output: (n, ...)} -> batch_gradients; the camera keys are own."""
    per_view = [torch_oracle.gradients_tch(sc, **{"grad_" + k: np.asarray(a[v], dtype=np.float64) for k, a in g.items()},
                                           ref=refs[v], visibility=None if visibility is None else visibility[v],
                                           camera=camera, **kw)
                for v, sc in enumerate(scenes)]
    return batch_gradients(per_view, tuple(own_keys) + (torch_oracle.CAMERA_KEYS if camera else ()))


def view_cameras(base, eyes, ats=None):
    cams = []
    for v, eye in enumerate(eyes):
        cam = dict(base, viewport=[0, 0, W, H], eye=np.asarray(eye, dtype=np.float64))
        if ats is not None:
            cam["at"] = np.asarray(ats[v], dtype=np.float64)
        cams.append(cam)
    return cams


def batch_upstream(n, seed, h=H, w=W, outputs=("image", "depth", "normal", "pos")):
    """Seeded float32 upstream gradients {output: (n, h, w[, 3])}; one stream, drawn in the order image, depth, normal,
    pos, so image and depth are the same numbers whether or not normal and pos are asked for."""
    rng = np.random.RandomState(seed)
    g = {k: rng.uniform(-1, 1, size=(n, h, w) if k == "depth" else (n, h, w, 3)).astype(np.float32)
         for k in ("image", "depth", "normal", "pos")}
    return {k: g[k] for k in outputs}


def _jitter(base, n, amp, seed_or_rng):
    """(n,) + base.shape: base plus uniform offsets in xyz, rounded to float32."""
    rng = seed_or_rng if hasattr(seed_or_rng, "uniform") else np.random.RandomState(seed_or_rng)
    off = rng.uniform(-amp, amp, size=(n,) + base.shape)
    off[..., 3] = 0.0
    return (base[None] + off).astype(np.float32).astype(np.float64)


def scene3():
    """(scene, cameras, {key: stacked per-view values}) of the five-view batch."""
    scene = unpack_scene(np.load(os.path.join(GOLDEN_DIR, "g10_torch_autograd_phong_ds_quartic.npz"), allow_pickle=False))
    assert "sphere" in scene["objects"]
    rng = np.random.RandomState(31)
    own = {key: _jitter(np.asarray(get_leaf(scene, key), dtype=np.float64), len(EYES3), amp, rng)
           for key, amp in (("disk.pos", 0.4), ("disk.normal", 0.2), ("lights.pos", 0.8))}
    return scene, view_cameras(scene["camera"], EYES3, ATS3), own


def ortho_case():
    scene = unpack_scene(np.load(os.path.join(GOLDEN_DIR, "g11_torch_autograd_ortho.npz"), allow_pickle=False))
    assert scene["camera"]["proj_type"] == "ortho"
    eye = np.asarray(scene["camera"]["eye"], dtype=np.float64)
    return scene, view_cameras(scene["camera"], [eye, eye + np.array([1.0, -0.5, 0.0, 0.0])])


def shadow_case():
    """(scene, render kwargs without 'shadow', three cameras, per-view light positions) on the s1a shadow fixture."""
    npz = np.load(os.path.join(GOLDEN_DIR, "s1a_mixed_shadow_64x48.npz"), allow_pickle=False)
    scene = unpack_scene(npz)
    kw = {k: v for k, v in json.loads(str(npz["kwargs"])).items() if k != "shadow"}
    eye = np.asarray(scene["camera"]["eye"], dtype=np.float64)
    cams = view_cameras(scene["camera"], [eye, eye + np.array([0.5, 0.2, 0.0, 0.0]), eye + np.array([-0.4, 0.3, 0.4, 0.0])])
    return scene, kw, cams, _jitter(np.asarray(scene["lights"]["pos"], dtype=np.float64), len(cams), 0.5, 17)


def visibility_rows(bits, n_lights):
    """Per view, the (L, N) 0 / 1 factors of the renderer's per-pixel light bit masks."""
    return [np.stack([((b >> l) & 1).astype(np.float64).reshape(-1) for l in range(n_lights)]) for b in bits]
