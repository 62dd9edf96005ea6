#!/usr/bin/env python3
"""Generate tests/golden/camera_warp/cw1_*.npz: the reference's OWN depth lift (cam_to_world_batched(z_to_pcl_CC_batched(
-depth, camera), None, camera)['pos']), projection_renderer_differentiable_fast and projection_reverse_renderer, imported
UNMODIFIED and run on the CPU in float32 under autograd, with the cameras' eye, at and up as leaves that require grad --
the gradient the layers' camera_grad=True gives -- on seeded cases of tests/surfels_cases.py, projection_cases.py and
reverse_projection_cases.py.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  The camera tensors come from ref_harness.layer_camera and get requires_grad_() here; a case of exactly
three views is recorded view by view (ref_harness.run_views).

Stored per fixture: what ref_harness.pack_layer stores (in/<input>, in/<camera>/<entry>, grad_in/<output>, ref/<output>,
grad/<input>), the layer's own in/ keys, and grad/<camera>/<eye, at, up> = d sum(output * grad_in) / d that tensor, in
its own shape.  The subfolder keeps the fixtures out of the top-level globs (the golden drift check,
conftest.golden_cases)."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import projection_cases as pc  # noqa: E402
import projection_oracle as po  # noqa: E402
import reverse_projection_cases as rc  # noqa: E402
import reverse_projection_oracle as ro  # noqa: E402
import surfels_cases as sc  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.torch.projection_layer as ref_projection  # noqa: E402

KEYS = ("eye", "at", "up")
CASES = {"lift": ("2x2", "17x9", "12x16"), "projection": ("2x2", "3x5", "12x16"), "reverse": ("1x1", "3x5", "12x16")}


def camera_leaves(camera):
    cam = R.layer_camera(camera)
    for k in KEYS:
        cam[k].requires_grad_()
    return cam


def finish(layer, name, c, leaves, cameras, run, extra):
    flat = R.pack_layer(c, leaves, R.run_views(run, c["shape"][0]), cameras=tuple(cameras))
    for label, cam in cameras.items():
        for k in KEYS:
            g = cam[k].grad
            flat[f"grad/{label}/{k}"] = g.numpy() if g is not None else np.zeros(tuple(cam[k].shape), np.float32)
            print(f"{layer} {name} {label}.{k:3s} |grad| max {np.abs(flat[f'grad/{label}/{k}']).max():.4g}")
    flat.update(extra)
    R.write(f"cw1_{layer}_{name}", flat)


def lift(name):
    c = sc.case(name)
    B, H, W = c["shape"]
    leaves = {"depth": torch.tensor(c["depth"], requires_grad=True)}
    cameras = {"camera": camera_leaves(c["camera"])}

    def run(views):
        cam = R.camera_views(cameras["camera"], views)
        with R.quiet():
            pos = R.ref_tch.z_to_pcl_CC_batched(-leaves["depth"][views].reshape(-1, H * W), cam)
            pos = R.ref_utils.cam_to_world_batched(pos, None, cam)["pos"]
        assert pos.shape[-1] == 4 and bool((pos[..., 3] == 1).all())
        return {"pos": pos[..., :3]}

    finish("lift", name, c, leaves, cameras, run, {"in/frame": np.asarray(c["frame"])})


def projection(name):
    c = pc.case(name)
    B, H, W, D = c["shape"]
    leaves = {k: torch.tensor(c[k], requires_grad=True) for k in po.INPUTS if c[k] is not None}
    cameras = {"camera": camera_leaves(c["camera"])}

    def run(views):
        with R.quiet():
            out, proj_out = ref_projection.projection_renderer_differentiable_fast(
                leaves["surfels"][views], leaves["rgb"][views].reshape(-1, H, W, D),
                R.camera_views(cameras["camera"], views),
                rotated_image=leaves["rotated_image"][views].reshape(-1, H, W, D) if "rotated_image" in leaves else None,
                blur_size=c["blur_size"], **c["flags"])
        return dict(proj_out, out=out)

    finish("projection", name, c, leaves, cameras, run,
           {"in/blur_size": np.asarray(c["blur_size"], dtype=np.float64),
            "in/flags": np.asarray(json.dumps(c["flags"], sort_keys=True))})


def reverse(name):
    c = rc.case(name)
    leaves = {k: torch.tensor(c[k], requires_grad=True) for k in ro.INPUTS if c[k] is not None}
    cameras = {label: camera_leaves(c[label]) for label in ("camera1", "camera2")}

    def run(views):
        with R.quiet():
            out, proj_out = ref_projection.projection_reverse_renderer(
                leaves["rgb"][views], leaves["in_pos_wc"][views], leaves["out_pos_wc"][views],
                *(R.camera_views(cam, views) for cam in cameras.values()),
                rotated_image=leaves["rotated_image"][views] if "rotated_image" in leaves else None, **c["flags"])
        return dict(proj_out, out=out)

    finish("reverse", name, c, leaves, cameras, run, {"in/flags": np.asarray(json.dumps(c["flags"], sort_keys=True))})


if __name__ == "__main__":
    R.OUT = R.fixture_dir("camera_warp")
    for layer, fn in (("lift", lift), ("projection", projection), ("reverse", reverse)):
        for n in CASES[layer]:
            fn(n)
