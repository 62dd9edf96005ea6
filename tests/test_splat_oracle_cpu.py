"""The fp64 splat-renderer restatement (tests/splat_oracle.py) against the reference's render_splats_along_ray under
autograd (tests/golden/p1_*.npz, oracle/golden_p1.py): the four forward outputs and d loss / d leaf for every
differentiable input, loss = sum image g_i + sum depth g_d + sum normal g_n + sum pos g_p.

Tolerances: the reference computes in float32.  Image, depth and pos carry a few float32 roundings of values of order
one to ten (atol 2e-5 relative to the output's largest entry).  Estimated normals come from normalised differences of
neighbouring points 0.05 apart at depth 5, where float32 keeps about four digits (atol 2e-3).  Gradients are checked per
leaf array against 3e-3 of the array's largest entry: the plane fit's float32 differences dominate, as for the normals.
"""
import os

import numpy as np
import pytest

import splat_oracle
from conftest import GOLDEN_DIR

CASES = sorted(os.path.splitext(f)[0] for f in os.listdir(GOLDEN_DIR) if f.startswith("p1_") and f.endswith(".npz"))


def _load(case):
    npz = np.load(os.path.join(GOLDEN_DIR, case + ".npz"), allow_pickle=False)
    return npz, splat_oracle.unpack(npz), splat_oracle.kwargs_of(npz)


def test_the_golden_cases_are_all_there():
    assert len(CASES) == 7, CASES


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_the_reference(case):
    npz, scene, kw = _load(case)
    out = splat_oracle.render(scene, splat_oracle.make_leaves(scene, requires_grad=False), **kw)
    given = "in/disk.normal" in npz.files
    for k in splat_oracle.OUTPUTS:
        want = npz["ref/" + k].astype(np.float64)
        got = out[k].numpy().reshape(want.shape)
        tol = 2e-3 if (k == "normal" and not given) else 2e-5 * max(np.abs(want).max(), 1.0)
        np.testing.assert_allclose(got, want, rtol=0, atol=tol, err_msg=f"{case} {k}")


@pytest.mark.parametrize("case", CASES)
def test_gradients_match_the_reference(case):
    npz, scene, kw = _load(case)
    up = {k: npz["grad_in/" + k] for k in splat_oracle.OUTPUTS}
    _, grads = splat_oracle.gradients(scene, up, **kw)
    checked = 0
    for key in npz.files:
        if not key.startswith("grad/"):
            continue
        name = key[5:]
        want = npz[key].astype(np.float64)
        got = grads[name].reshape(want.shape)
        if name == "disk.pos" and want.ndim == 2:
            assert np.all(got[:, :2] == 0) and np.all(want[:, :2] == 0)        # only column 2 (z) is read
        scale = max(np.abs(want).max(), 1e-6)
        np.testing.assert_allclose(got, want, rtol=0, atol=3e-3 * scale, err_msg=f"{case} {name}")
        checked += 1
    assert checked >= 7


def test_splats_behind_the_camera_get_no_depth_gradient():
    npz, scene, kw = _load("p1_zpos_flat_36x48")
    z = np.asarray(scene["objects"]["disk"]["pos"]).reshape(-1)
    _, grads = splat_oracle.gradients(scene, {k: npz["grad_in/" + k] for k in splat_oracle.OUTPUTS}, **kw)
    assert (z >= 0).sum() == 3
    assert np.all(grads["disk.pos"][z >= 0] == 0) and np.all(npz["grad/disk.pos"][z >= 0] == 0)
