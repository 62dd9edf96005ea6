"""The conditions tests/mesh_sampling_cases.py promises of its regular cases, on which the GPU tests' exact `face`
comparison and their bounds rest.  No GPU."""
import numpy as np
import pytest

import mesh_sampling_cases as cases
import mesh_sampling_oracle as oracle

ALL = range(len(cases.REGULAR))


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_shapes_and_variants(k):
    name, _mesh, F, S, f_views, eye_kind = cases.REGULAR[k]
    c = cases.regular(k)
    V = c["v"].shape[1]
    assert c["v"].shape == (cases.VIEWS, V, 3) and c["v"].dtype == np.float32
    assert c["f"].shape == ((cases.VIEWS, F, 3) if f_views else (F, 3))
    assert c["f"].min() >= 0 and c["f"].max() < V
    assert c["uniforms"].shape == (cases.VIEWS, S, 3) and c["uniforms"].dtype == np.float64
    assert (c["uniforms"] >= 0).all() and (c["uniforms"] < 1).all()
    assert {None: c["eye"] is None, "shared": np.shape(c["eye"]) == (3,),
            "per_view": np.shape(c["eye"]) == (cases.VIEWS, 3)}[eye_kind]
    assert not np.array_equal(c["v"][0], c["v"][1]) and not np.array_equal(c["v"][1], c["v"][2])
    if f_views:
        assert not np.array_equal(c["f"][0], c["f"][1])


def test_the_shapes_sit_at_the_kernels_seams():
    faces = [row[2] for row in cases.REGULAR]
    for want in (1, 2, 12, 63, 64, 65, cases.SCAN_WAVE + 1, cases.SCAN_TILE + 1, 4968):
        assert want in faces
    assert cases.SCAN_TILE == 1025 - 1                                  # the issue's 1025 is one face above the tile


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_every_r0_keeps_its_distance_from_every_cdf_value(k):
    c = cases.regular(k)
    for b in range(cases.VIEWS):
        v, f, u, eye = cases.view_of(c, b)
        w = oracle.face_quantities(v, f, eye)["weight"]
        assert (w > 0).any()
        for cdf in (oracle.cdf_numpy(w), oracle.cdf_plain(w)):
            assert (np.diff(cdf) >= 0).all() and cdf[-1] == 1.0
            assert cases.gap_to(cdf, u[:, 0]) >= cases.GAP
        # the two CDFs are as close as any fixed-order scan is to either
        assert np.abs(oracle.cdf_numpy(w) - oracle.cdf_plain(w)).max() <= len(w) * 2.0 ** -52
        assert np.array_equal(cases.draw(int(c["seeds"][b]), len(u)), u)


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_the_cull_is_decided_and_no_face_is_a_sliver_and_two_faces_are_hit(k):
    c = cases.regular(k)
    F = cases.REGULAR[k][2]
    for b in range(cases.VIEWS):
        v, f, u, eye = cases.view_of(c, b)
        q = oracle.face_quantities(v, f, eye)
        if eye is not None:
            assert (np.abs(q["facing"]) >= 1e-6).all()
            if F > 2:
                assert 0 < q["keep"].sum() < F                           # the cull culls, and not everything
        assert np.isfinite(q["area2"]).all() and (q["area2"] > 0).all()
        assert (q["conditioning"] <= 2.0 ** 10).all()
        hit = np.unique(oracle.forward(v, f, u, eye)["face"])
        assert (hit >= 0).all() and q["keep"][hit].all()
        if F > 1:
            assert len(hit) >= 2


def test_the_cases_do_not_drift():
    sums = {cases.tag(k): cases.checksum(cases.regular(k)) for k in ALL}
    assert len(set(sums.values())) == len(sums)
    assert cases.checksum(cases.regular(0)) == cases.checksum(cases.regular.__wrapped__(0))   # seeded, not cached luck
