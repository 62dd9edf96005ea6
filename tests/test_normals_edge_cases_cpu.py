"""Each case of tests/normals_edge_cases.py reaches the branch it is named for -- shown with the fp64 restatement
tests/normals_oracle.py, without a GPU.  tests/test_hip_normals_edges.py holds the kernels to the restatement on them."""
import numpy as np
import pytest
import torch

import normals_edge_cases as edges
import normals_oracle as no


def test_the_names_are_the_cases():
    assert set(edges.NAMES) == set(edges._SPEC)
    for name in edges.NAMES:
        c = edges.case(name)
        B, H, W = c["shape"]
        assert c["pos"].shape == c["upstream"]["normal"].shape == (B, H, W, 3) and c["pos"].dtype == np.float32


def test_a_side_of_two_lands_both_reflected_neighbours_on_one_pixel():
    assert no.reflect_index(2).tolist() == [1, 0, 1, 0] and no.reflect_index(3).tolist() == [1, 0, 1, 2, 1]
    # the 8 slots (dy-major) of a pixel away from the long side's ends; 2 x 3 / 3 x 2: the slots across the short side
    # come in equal pairs; 2 x 2: the four diagonals are one point
    for name, (i, j), twice, four in (("two_2x3", (0, 1), (0, 1, 2, 5, 6, 7), ()), ("two_3x2", (1, 0), (0, 2, 3, 4, 5, 7), ()),
                                      ("two_2x2", (0, 0), (1, 6, 3, 4), (0, 2, 5, 7))):
        c = edges.case(name)
        u = no.neighbour_units(torch.tensor(c["pos"].astype(np.float64))).numpy()[:, 0, i, j]
        copies = [sum(np.array_equal(u[k], u[m]) for m in range(8)) for k in range(8)]
        assert [k for k in range(8) if copies[k] == 2] == sorted(twice), (name, copies)
        assert [k for k in range(8) if copies[k] == 4] == sorted(four), (name, copies)


def test_the_long_grids_fill_two_workgroups_and_part_of_a_third():
    for name in ("wide_2x300", "tall_300x2"):
        B, H, W = edges.case(name)["shape"]
        assert B == 2 and 2 * 256 < H * W < 3 * 256 and min(H, W) == 2 and 256 % max(H, W)
    assert edges.case("b5_2x2")["shape"] == (5, 2, 2)


def test_a_constant_patch_has_no_direction_and_no_gradient():
    c = edges.case("constant_4x4")
    assert np.all(c["pos"] == c["pos"][0, 0, 0])
    a, b, d, r0, r1, det = (m.numpy() for m in no.moments(torch.tensor(c["pos"].astype(np.float64))))
    assert np.all(a == 0) and np.all(b == 0) and np.all(d == 0) and np.all(r0 == 0) and np.all(r1 == 0)
    assert np.all(det == 1e-12)
    v, g = edges.expected("constant_4x4")
    assert np.all(v["normal"][..., :2] == 0) and np.all(v["normal"][..., 2] == 1.0 / np.sqrt(1.0 + 3e-10))
    assert np.all(g["pos"] == 0) and not c["nonzero"]


def test_the_vertical_plane_cancels_the_determinant_exactly():
    c = edges.case("vertical_plane_5x6")
    assert np.array_equal(c["pos"][..., 0], c["pos"][..., 1])
    a, b, d, r0, r1, det = (m.numpy() for m in no.moments(torch.tensor(c["pos"].astype(np.float64))))
    assert np.all(a > 1) and np.array_equal(a, b) and np.array_equal(a, d) and np.array_equal(r0, r1)
    assert np.all(det == 1e-12)
    v, g = edges.expected("vertical_plane_5x6")
    assert np.all(v["normal"][..., :2] == 0) and np.all(np.isfinite(g["pos"])) and np.abs(g["pos"]).max() > 1e10


def test_duplicated_neighbours_give_a_zero_difference_that_stays_finite():
    c = edges.case("duplicates_5x6")
    assert np.array_equal(c["pos"][:, :, 2::2], c["pos"][:, :, 1:-1:2])
    u = no.neighbour_units(torch.tensor(c["pos"].astype(np.float64))).numpy()
    assert np.all(u[4, :, :, 1:-1:2] == 0) and np.all(u[3, :, :, 2::2] == 0)      # slots (0, +1) and (0, -1): the copy
    assert np.all(no.moments(torch.tensor(c["pos"].astype(np.float64)))[5].numpy() > 1e-3)      # no fit degenerates
    v, g = edges.expected("duplicates_5x6")
    assert np.all(np.isfinite(v["normal"])) and np.all(np.isfinite(g["pos"])) and np.abs(g["pos"]).max() > 0


@pytest.mark.parametrize("name", list(edges.SPECIAL))
def test_a_special_point_spoils_its_reach_and_nothing_else(name):
    c = edges.case(name)
    assert np.array_equal(np.isfinite(c["pos"]), ~((np.arange(7)[:, None, None] == 3) & (np.arange(7)[None, :, None] == 3)
                                                    & (np.arange(3) == 2))[None] | (name == "big_7x7"))
    assert np.isnan(c["upstream"]["normal"][0, 0, 6, 2]) and np.isnan(c["upstream"]["normal"]).sum() == 1
    v, g = edges.expected(name)
    finite_n, finite_g = np.isfinite(v["normal"][0]).all(-1), np.isfinite(g["pos"][0]).all(-1)
    assert np.array_equal(np.isfinite(v["normal"][0]).any(-1), finite_n)              # a pixel is spoilt in all components
    assert np.array_equal(np.isfinite(g["pos"][0]).any(-1), finite_g)
    spoilt = name != "big_7x7"
    assert np.array_equal(~finite_n, edges.reach(edges.CENTRE, 1) & spoilt)
    assert np.array_equal(~finite_g, (edges.reach(edges.CENTRE, 2) & spoilt) | edges.reach(edges.CORNER, 1))
    assert finite_g.sum() >= 20 and np.abs(g["pos"][0][finite_g]).max() > 0


def test_a_shared_camera_is_the_same_camera_for_every_view():
    s, p = edges.case("world_shared_6x5"), edges.case("world_views_6x5")
    assert np.asarray(s["camera"]["eye"]).shape == (3,) and np.asarray(p["camera"]["eye"]).shape == (2, 3)
    assert not np.array_equal(p["camera"]["eye"][0], p["camera"]["eye"][1])
    R = no.rotation(s["camera"], 2).numpy()
    assert np.array_equal(R[0], R[1])
    cam, _ = no.gradients({"pos": s["pos"]}, None, s["upstream"], "camera")
    np.testing.assert_allclose(np.einsum("brc,bhwc->bhwr", R, cam["normal"]), edges.expected("world_shared_6x5")[0]["normal"],
                               rtol=0, atol=1e-14)
