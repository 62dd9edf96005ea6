"""CPU: tests/dense_camera_oracle.py against the reference's OWN camera gradients, tests/golden/dense_camera/dc1_*.npz
(tools/gen_dense_camera_golden.py: the unmodified reference on the CPU under autograd, eye / at / up as leaves), for
projection_renderer_differentiable and for the world-frame plane fit cam_to_world_batched(None,
estimate_surface_normals_plane_fit_batched(pos), camera)['normal'].  Both were recorded in float64 (in/precision).

Tolerance.  Reference and restatement are both float64, so the difference is summation order (the reference's matrix
products against the restatement's) and, for the normals, R^-T against R (below).  MEASURED is max|ref - oracle| /
max|oracle| per camera entry, the worst over the layer's fixtures, as measured when the fixtures were recorded -- the
same figures with 1 and with 16 torch threads; the assertion is 4 x that, the project's margin for BLAS summation-order
differences between thread counts.

    dense    eye 5.13e-16   at 4.37e-16   up 1.29e-15
    normals  eye 1.72e-10   at 1.72e-10   up 3.41e-10

The normals' 1e-10 is not rounding: the reference rotates a normal by R^-T (the inverse transpose of its lookat basis)
where the project applies R; the columns are unit vectors up to normalize's 1e-10 under the square root, so the two
differ by some 1e-10 relative, and that difference IS the measured figure (with R^-T in the restatement the same
fixtures agree to 3e-15).  At the asserted bound the fixtures therefore do not tell R^-T from R, and
test_the_fixtures_do_not_see_the_inverse_transpose asserts exactly that, so nobody takes them for a guard of it.

Mutations (test_a_wrong_constant_misses_the_bound, test_the_given_up_as_the_y_axis_misses_the_bound): each wrong
constant of dense_projection_oracle.WRONG misses the dense bound on at least one fixture; the un-orthogonalised `up` as
the y axis misses it on the normals' fixtures and -- through the view matrix -- on the dense ones."""
import glob
import os

import numpy as np
import pytest
import torch

import camera_chain_oracle as co
import dense_camera_oracle as dco
import dense_projection_oracle as do
import projection_oracle as po
from test_camera_warp_golden_cpu import _camera_to_world_with_the_given_up, _lookat_with_the_given_up

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_camera")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "dc1_*.npz")))
EXPECTED = ({f"dc1_dense_{f}_{layout}" for f in ("2x2", "3x5", "12x16", "17x9") for layout in ("grid", "flat")}
            | {f"dc1_normals_{n}" for n in ("2x2", "3x5", "12x16", "17x9")})
MEASURED = {  # worst max|ref - oracle| / max|oracle| over the layer's fixtures
    "dense": {"eye": 5.13e-16, "at": 4.37e-16, "up": 1.29e-15},
    "normals": {"eye": 1.72e-10, "at": 1.72e-10, "up": 3.41e-10},
}
MARGIN = 4.0


def load(name):
    f = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cam = {k.split("/")[2]: f[k] for k in f.files if k.startswith("in/camera/")}
    cam["fovy"], cam["focal_length"] = float(cam["fovy"]), float(cam["focal_length"])
    ups = {k[len("grad_in/"):]: f[k] for k in f.files if k.startswith("grad_in/")}
    ins = {k[3:]: f[k] for k in f.files if k.startswith("in/") and k.count("/") == 1}
    ref = {k: f[f"grad/camera/{k}"].astype(np.float64) for k in co.CAMERA_KEYS}
    return f, name.split("_")[1], cam, ups, ins, ref


def oracle(name, wrong=()):
    """(layer, the reference's {entry: gradient}, the restatement's, (reference values, restatement values))."""
    f, layer, cam, ups, ins, ref = load(name)
    assert str(f["in/precision"]) == "float64"
    if layer == "dense":
        got = dco.project_gradients({k: ins.get(k) for k in do.INPUTS}, cam, ups, float(f["in/blur_size"]), wrong=wrong)
    else:
        got = dco.normals_gradients({"pos": ins["pos"]}, cam, ups, str(f["in/frame"]), wrong=wrong)
    return layer, ref, got[2]["camera"], ({k: f["ref/" + k] for k in ups}, got[0])


def errors(ref, got):
    """{entry: max|ref - got| / max|got|}."""
    out = {}
    for k in co.CAMERA_KEYS:
        assert ref[k].shape == got[k].shape, k
        out[k] = np.abs(ref[k] - got[k]).max() / np.abs(got[k]).max()
    return out


def misses(layer, err):
    return any(e > MARGIN * MEASURED[layer][k] for k, e in err.items())


def test_the_fixtures_are_the_cases_the_layers_were_recorded_on():
    assert set(FIXTURES) == EXPECTED
    for name in FIXTURES:
        f = load(name)[0]
        B, last = f["in/camera/eye"].shape
        assert B <= 3 and last == (4 if "17x9" in name and "dense" in name else 3), name
        if last == 4:                    # the w column gets a zero gradient, in the reference too
            assert all(not np.any(f[f"grad/camera/{k}"][:, 3]) for k in co.CAMERA_KEYS), name


@pytest.mark.parametrize("threads", [1, 16])
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_restatement_gives_the_references_camera_gradients(name, threads):
    saved = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        layer, ref, got, (ref_values, values) = oracle(name)
    finally:
        torch.set_num_threads(saved)
    # the values first: the same function.  1e-9: ten times normalize's 1e-10, which is what R^-T and R differ by
    for k, v in values.items():
        np.testing.assert_allclose(v, ref_values[k].reshape(v.shape), rtol=1e-9, atol=1e-9, err_msg=f"{name} {k}")
    for k, err in errors(ref, got).items():
        print(f"{name} camera.{k} at {threads} threads: {err:.3g} (measured worst {MEASURED[layer][k]:.3g})")
        assert err <= MARGIN * MEASURED[layer][k], (name, k, err)
    assert all(np.abs(g).max() > 0 for g in ref.values()), name


@pytest.mark.parametrize("wrong", do.WRONG)
def test_a_wrong_constant_misses_the_bound(wrong):
    hit = [n for n in sorted(EXPECTED) if "dense" in n and misses("dense", errors(*oracle(n, wrong=(wrong,))[1:3]))]
    print(wrong, hit)
    assert hit, wrong


@pytest.mark.parametrize("layer", ["dense", "normals"])
def test_the_given_up_as_the_y_axis_misses_the_bound(layer, monkeypatch):
    names = [n for n in sorted(EXPECTED) if layer in n]
    if layer == "normals":
        hit = [n for n in names if misses(layer, errors(*oracle(n, wrong=("raw_up",))[1:3]))]
    else:
        monkeypatch.setattr(po, "lookat", _lookat_with_the_given_up)
        monkeypatch.setattr(co, "camera_to_world", _camera_to_world_with_the_given_up)
        hit = [n for n in names if misses(layer, errors(*oracle(n)[1:3]))]
    print(layer, hit)
    assert hit, layer


@pytest.mark.parametrize("name", sorted(n for n in EXPECTED if "normals" in n))
def test_the_fixtures_do_not_see_the_inverse_transpose(name):
    layer, ref, got, _ = oracle(name, wrong=("inverse_transpose",))
    assert not misses(layer, errors(ref, got)), name
