#!/usr/bin/env python3
"""Fraction of tile-list entries the binned disc kernel sweeps at BASELINE config 5 (measurement; one MI355X).
Needs a library built with -DSRH_DIAG_SWEPT (in SRH_LIB): each tile's first two pixels of `nearest` then hold the
entries swept and the entries listed.  usage: SRH_LIB=build/abl/diag_swept.so tools/occl_stats.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from surf_renderer_amd import renderer, synthetic  # noqa: E402

scene = synthetic.disk_cloud_scene()
buf = renderer.flatten_scene(scene, device="cuda:0")
cam = renderer.camera_struct(scene["camera"])
_, _, nearest = renderer.render_buffers(buf, cam, mode="binned", waves_per_tile=1)
torch.cuda.synchronize()
nr = nearest.cpu().numpy()
swept = nr[::16, 0::16].astype(np.int64)
listed = nr[::16, 1::16].astype(np.int64)
busy = listed > 0
print(json.dumps({"lib": os.environ.get("SRH_LIB", "in-tree"), "busy_tiles": int(busy.sum()),
                  "entries_listed": int(listed.sum()), "entries_swept": int(swept.sum()),
                  "fraction_swept": float(swept.sum() / max(listed.sum(), 1)),
                  "tiles_over_128": int((listed > 128).sum())}))
