"""tests/mesh_sampling_oracle.py against the reference's recorded uniform_sample_mesh (tests/golden/mesh_sampling,
written by tools/gen_mesh_sampling_golden.py from the unmodified reference): the faces equal, points and normals to
2^-50 relative (they came out bit-equal when the fixtures were made), and the torch autograd restatement against
central differences of the oracle's own forward.  No GPU."""
import os

import numpy as np
import pytest

import mesh_sampling_cases as cases
import mesh_sampling_oracle as oracle
from conftest import GOLDEN_DIR

ALL = range(len(cases.REGULAR))


def fixture(k):
    return dict(np.load(os.path.join(GOLDEN_DIR, "mesh_sampling", "ms1_" + cases.tag(k) + ".npz")))


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_the_fixture_holds_the_cases_inputs(k):
    z, c = fixture(k), cases.regular(k)
    for key in ("v", "f", "uniforms", "seeds"):
        assert np.array_equal(z["in/" + key], c[key]), key
    assert z["in/v"].dtype == np.float32 and z["in/uniforms"].dtype == np.float64
    assert ("in/eye" in z) == (c["eye"] is not None)
    if c["eye"] is not None:
        assert np.array_equal(z["in/eye"], c["eye"])


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_the_oracle_reproduces_the_references_samples(k):
    z = fixture(k)
    eye = z.get("in/eye")
    for b in range(cases.VIEWS):
        r = oracle.forward(z["in/v"][b], cases.view_faces(z["in/f"], b), z["in/uniforms"][b], cases.view_eye(eye, b))
        assert np.array_equal(r["face"], z["ref/face"][b]), b
        for key in ("pos", "normal"):
            want = z["ref/" + key][b]
            assert (np.abs(r[key] - want) <= 2.0 ** -50 * np.abs(want)).all(), (b, key)


def test_the_uniforms_are_the_stream_the_reference_consumes():
    """after np.random.seed(k): random_sample(S) inside np.random.choice, then rand(S, 2)"""
    from surf_renderer_amd.mesh_sampling import draw_uniforms
    c = cases.regular(2)
    for b in range(cases.VIEWS):
        np.random.seed(int(c["seeds"][b]))
        assert np.array_equal(draw_uniforms(c["uniforms"].shape[1]), c["uniforms"][b])
        rng = np.random.RandomState(int(c["seeds"][b]))
        assert np.array_equal(draw_uniforms(c["uniforms"].shape[1], rng), c["uniforms"][b])


@pytest.mark.parametrize("k", [2, 4, 5], ids=cases.tag)
def test_the_autograd_restatement_matches_central_differences(k):
    c = cases.regular(k)
    v, f, u, eye = cases.view_of(c, 1)
    r = oracle.forward(v, f, u, eye)
    g = oracle.gradients(v, f, r["face"], r["bary"], c["g_pos"][1], c["g_normal"][1])
    assert (g["S_v"] >= np.abs(g["grad_v"]) * (1 - 1e-12)).all()        # S bounds its own sum

    def loss(vv):
        q = oracle.face_quantities(vv, f, None)
        tri = vv[f[r["face"]]]
        return float(np.sum(np.sum(r["bary"][..., None] * tri, axis=1) * c["g_pos"][1])
                     + np.sum(q["normal"][r["face"]] * c["g_normal"][1]))

    # float32-representable steps: the oracle rounds its vertices through float32
    v64 = oracle.widen(v)
    rng = np.random.RandomState(5)
    for _ in range(6):
        i, a = rng.randint(len(v64)), rng.randint(3)
        h = 2.0 ** -10 * max(1.0, abs(v64[i, a]))
        up, dn = v64.copy(), v64.copy()
        up[i, a] = np.float32(v64[i, a] + h)
        dn[i, a] = np.float32(v64[i, a] - h)
        fd = (loss(up) - loss(dn)) / (up[i, a] - dn[i, a])
        assert abs(fd - g["grad_v"][i, a]) <= 1e-3 * max(1.0, g["S_v"][i, a]), (i, a, fd, g["grad_v"][i, a])


def test_a_view_without_a_positive_weight_and_a_non_finite_face():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [1, 1, 0]], np.float32)
    u = cases.draw(1, 7)
    r = oracle.forward(v, [[0, 1, 2], [1, 3, 2], [1, 4, 2]], u)
    assert set(r["face"]) <= {0, 2} and np.isfinite(r["pos"]).all()
    r = oracle.forward(v, [[0, 1, 2]], u, eye=[0.2, 0.2, -3.0])             # culled
    assert (r["face"] == -1).all() and np.isnan(r["pos"]).all() and np.isnan(r["normal"]).all()
    g = oracle.gradients(v, [[0, 1, 2]], r["face"], r["bary"], np.ones((7, 3)), np.ones((7, 3)))
    assert (g["grad_v"] == 0).all() and (g["S_v"] == 0).all()
