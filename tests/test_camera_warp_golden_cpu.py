"""CPU: tests/camera_chain_oracle.py against the reference's OWN camera gradients, tests/golden/camera_warp/cw1_*.npz
(tools/gen_camera_warp_golden.py: the unmodified reference on the CPU in float32, eye / at / up of every camera as
leaves), for the depth lift, projection_renderer_differentiable_fast and projection_reverse_renderer.

Tolerance.  The reference's arithmetic is float32 and the restatement's float64, so the difference is the reference's
own rounding.  MEASURED is max|ref32 - oracle| / max|oracle| per camera entry, the worst over the layer's fixtures, as
measured when the fixtures were recorded; the assertion is 4 x that, the margin of the projection layer's float32
comparison (the surfel re-projection layer).  An entry whose own largest gradient is below 1e-6 of its
camera's largest is a sum that cancels (reverse 1x1: camera2['at'], the one surfel sits on the optical axis) or cannot
be reached at all (reverse: camera2['up'], row 2 of the matrix is unit(eye - at)); float32 cannot resolve it, and its
error is measured against the camera's largest entry instead.  Where both are exactly 0 (reverse 1x1 camera1: one texel,
a sample scale of 0) the comparison is exact.

Mutations (test_a_wrong_lookat_misses_the_bound): with the un-orthogonalised `up` as the y axis the restatement misses
the bound on every fixture.  Dropping the 1e-10 under normalize's square root moves the gradients by some 1e-10 of their
size, four orders below the float32 reference's own error: these fixtures cannot see it, and the test asserts exactly
that, so nobody takes them for a guard of it.  The guard is in fp64: tests/test_camera_chain_oracle_cpu.py::
test_the_restatements_matrices_are_the_layers_own_and_fp64_sees_the_epsilon holds the restatement's matrices to
_camera.view_matrices / inverse_view_matrices bit for bit and shows that without the 1e-10 they differ."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import camera_chain_oracle as co
import projection_oracle as po
import reverse_projection_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_warp")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "cw1_*.npz")))
EXPECTED = {"cw1_lift_2x2", "cw1_lift_17x9", "cw1_lift_12x16", "cw1_projection_2x2", "cw1_projection_3x5",
            "cw1_projection_12x16", "cw1_reverse_1x1", "cw1_reverse_3x5", "cw1_reverse_12x16"}
MEASURED = {  # worst max|ref32 - oracle| / max|oracle| over the layer's fixtures
    "lift": {"camera": {"eye": 6.93e-07, "at": 2.08e-07, "up": 2.51e-07}},
    "projection": {"camera": {"eye": 2.4e-06, "at": 1.71e-06, "up": 3.59e-06}},
    "reverse": {"camera1": {"eye": 3.8e-07, "at": 8.68e-07, "up": 9e-07},
                "camera2": {"eye": 1.84e-06, "at": 5.5e-07, "up": 5.76e-08}},
}
MARGIN = 4.0
CANCELS = 1e-6


def oracle(name):
    """(layer, {camera: {entry: the reference's gradient}}, {camera: {entry: the restatement's}})."""
    f = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    layer = name.split("_")[1]
    labels = sorted({k.split("/")[1] for k in f.files if k.startswith("in/camera")})
    cams = {c: {k.split("/")[2]: f[k] for k in f.files if k.startswith(f"in/{c}/")} for c in labels}
    for c in cams.values():
        c["fovy"], c["focal_length"] = float(c["fovy"]), float(c["focal_length"])
    ups = {k[len("grad_in/"):]: f[k] for k in f.files if k.startswith("grad_in/")}
    ins = {k[3:]: f[k] for k in f.files if k.startswith("in/") and k.count("/") == 1}
    if layer == "lift":                         # the batched reference function builds its grid with torch.linspace
        got = co.lift_gradients(ins, cams["camera"], ups, str(f["in/frame"]), grid="torch")
    elif layer == "projection":
        got = co.project_gradients({k: ins.get(k) for k in po.INPUTS}, cams["camera"], ups, float(f["in/blur_size"]),
                                   **json.loads(str(f["in/flags"])))
    else:
        got = co.reverse_gradients({k: ins.get(k) for k in ro.INPUTS}, cams["camera1"], cams["camera2"], ups,
                                   **json.loads(str(f["in/flags"])))
    ref = {c: {k: f[f"grad/{c}/{k}"].astype(np.float64) for k in co.CAMERA_KEYS} for c in labels}
    return layer, ref, got[2]


def errors(ref, got):
    """{(camera, entry): max|ref - got| / scale}, scale as the module's docstring has it; None where both are 0."""
    out = {}
    for c in ref:
        top = max(np.abs(a).max() for a in got[c].values())
        for k in co.CAMERA_KEYS:
            assert ref[c][k].shape == got[c][k].shape, (c, k)
            own = np.abs(got[c][k]).max()
            scale = own if own > CANCELS * top else top
            out[c, k] = None if scale == 0 and not np.any(ref[c][k]) else np.abs(ref[c][k] - got[c][k]).max() / scale
    return out


def test_the_fixtures_are_the_cases_the_layers_were_recorded_on():
    assert set(FIXTURES) == EXPECTED


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_restatement_gives_the_references_camera_gradients(name):
    layer, ref, got = oracle(name)
    for (c, k), err in errors(ref, got).items():
        print(f"{name} {c}.{k}: {err if err is None else format(err, '.3g')} (measured worst {MEASURED[layer][c][k]:.3g})")
        assert err is None or err <= MARGIN * MEASURED[layer][c][k], (name, c, k, err)
    if name != "cw1_reverse_1x1":
        assert all(np.abs(g).max() > 0 for g in ref[sorted(ref)[0]].values()), name


def _lookat_with_the_given_up(eye, at, up):
    z = po._normalize(eye - at)
    x = po._normalize(torch.cross(po._normalize(up), z, dim=-1))
    y = po._normalize(up)                                           # not z x x
    top = torch.cat((torch.stack((x, y, z), dim=-1), eye[..., None]), dim=-1)
    row = torch.zeros((eye.shape[0], 1, 4), dtype=eye.dtype, device=eye.device)
    row[..., 3] = 1
    return torch.linalg.inv(torch.cat((top, row), dim=-2))


def _camera_to_world_with_the_given_up(camera, dtype):
    eye, at, up = (co.vector(camera, k, dtype) for k in co.CAMERA_KEYS)
    z = po._normalize(eye - at)
    x = po._normalize(torch.cross(po._normalize(up), z, dim=-1))
    return torch.stack((x, po._normalize(up), z), dim=-1), eye


def _normalize_without_epsilon(u):
    return po.nonzero_divide(u, torch.sqrt(torch.sum(u * u, dim=-1, keepdim=True)))


@pytest.mark.parametrize("name", ["cw1_lift_12x16", "cw1_projection_12x16", "cw1_reverse_12x16"])
def test_a_wrong_lookat_misses_the_bound(name, monkeypatch):
    layer, ref, _ = oracle(name)
    with monkeypatch.context() as m:
        m.setattr(po, "lookat", _lookat_with_the_given_up)
        m.setattr(co, "camera_to_world", _camera_to_world_with_the_given_up)
        wrong = errors(ref, oracle(name)[2])
    assert any(e is not None and e > MARGIN * MEASURED[layer][c][k] for (c, k), e in wrong.items()), wrong
    with monkeypatch.context() as m:                                 # beneath what a float32 reference can show
        m.setattr(po, "_normalize", _normalize_without_epsilon)
        unseen = errors(ref, oracle(name)[2])
    assert all(e is None or e <= MARGIN * MEASURED[layer][c][k] for (c, k), e in unseen.items()), unseen
