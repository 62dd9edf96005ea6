"""Shared by the multi-view gradient tests: the v1 fixtures (tools/gen_golden_views_grad.py) as per-view scenes, and
the per-view gradient oracle summed / stacked the way a batch's gradients are defined -- a leaf all views share gets
the sum over the views, a leaf a view overrides the gradient of that view alone."""
import copy
import json
import os

import numpy as np

from conftest import GOLDEN_DIR
from oracle import torch_oracle
from oracle.golden_io import unpack_scene

V1_CASES = ["v1_views_grad_phong", "v1_views_grad_phong_ds_quartic"]
V1_PER_VIEW = ("disk.pos", "lights.pos")


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


def oracle_batch_tch(scenes, g_img, g_dep, refs, own_keys, visibility=None, **kw):
    per_view = [torch_oracle.gradients_tch(sc, g_img[v], None if g_dep is None else g_dep[v], ref=refs[v],
                                           visibility=None if visibility is None else visibility[v], **kw)
                for v, sc in enumerate(scenes)]
    return batch_gradients(per_view, own_keys)
