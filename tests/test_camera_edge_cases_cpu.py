"""No GPU: what the fp64 restatements with camera leaves say about the cases of tests/camera_edge_cases.py, on which
tests/test_hip_camera_edges.py holds the kView kernels.  The restatements themselves are pinned to the reference's own
runs by test_camera_chain_oracle_cpu.py, test_dense_camera_golden_cpu.py, test_camera_grad_golden_cpu.py and
test_frames_oracle_cpu.py.

Where the camera gradient is non-finite (camera_edge_cases.NONFINITE): the lift's special_3x3 and the world normals'
nan_7x7, inf_7x7 and big_7x7 (1e30 overflows the moments) in every entry, view 1 of every poisoned batch in every entry,
and nothing else.

Which entries can be compared relatively is decided here, from the restatement alone: every finite case is evaluated a
second time with its sums in another order (camera_edge_cases.second).  An entry whose two values differ by more than
1e-7 relative is rounding noise; the GPU test holds such an entry by size, and so it must BE small: below 1e-9 of the
camera's largest gradient in both orders.  No case has such an entry today.  Every other entry agrees between the two
orders to 1e-10 relative -- or, for an entry far below the camera's largest, to 1e-15 of that largest: the sums run over
terms of that size, each rounded to 2^-53 of itself, so no two orders of an fp64 sum agree better in absolute terms.
`up` of the dense row_1x5 and col_5x1 is such an entry (2e-8 of the camera's largest: `up` reaches a frame with a
one-pixel axis only through the 1e-10 under normalize's square root); its two orders differ by 4e-8 of itself, 7e-17 of
the largest."""
import numpy as np
import pytest
import torch

import camera_edge_cases as ce
import frames_oracle as fo

FINITE = [i for i in ce.ALL if i[0] != "poisoned" and (i[0], i[1]) not in ce.NONFINITE]
IDS = [ce.tag(*i) for i in ce.ALL]


def _ids(items):
    return [ce.tag(*i) for i in items]


def _leaf_shape(layer, name, variant):
    c = ce.case(layer, name, variant)
    camera = c["scene"]["camera"] if "scene" in c else c["camera"]
    return {k: np.shape(camera[k]) for k in ce.KEYS}


def test_the_cases_are_the_ones_the_layers_edge_suites_hold():
    import dense_projection_edge_cases as de
    import normals_edge_cases as ne
    import splat_edge_scenes as se
    import splats_ndc_edge_cases as sne
    assert ce.ALONG_RAY == se.CASES and len(se.CASES) == 24 and ce.NDC == sne.NAMES and len(ce.NDC) == 7
    assert ce.NORMALS == ne.NAMES and {n for n, layout, rot in ce.DENSE if layout == "grid" and not rot} == set(de.NAMES) | {"zdepth_9x7"}
    assert len(set(ce.ALL)) == len(ce.ALL)
    assert all(ce.case("normals", n)["frame"] == "world" for n in ce.NORMALS)
    c, s = ce.case("lift", "special_finite_3x3"), ce.case("lift", "special_3x3")
    assert np.all(np.isfinite(c["depth"]) | np.isneginf(c["depth"])) and c["depth"][0, 4] == 2.5 and c["depth"][0, 7] == 1.75
    keep = [0, 1, 2, 3, 5, 6, 8]
    assert np.array_equal(c["depth"][0, keep].view(np.uint32), s["depth"][0, keep].view(np.uint32))


@pytest.mark.parametrize("layer,name,variant", ce.ALL, ids=IDS)
def test_the_camera_gradient_has_the_shape_of_its_leaf_and_is_finite_where_the_table_says(layer, name, variant):
    cam = ce.expected(layer, name, variant)[2]
    shapes = _leaf_shape(layer, name, variant)
    for k in ce.KEYS:
        assert cam[k].shape == shapes[k], (k, cam[k].shape, shapes[k])
        finite = np.isfinite(cam[k])
        if layer == "poisoned":
            assert not finite[ce.POISONED_VIEW].any() and finite[[0, 2]].all(), k
        elif (layer, name) in ce.NONFINITE:
            assert not finite.any(), k
        else:
            assert finite.all(), k


@pytest.mark.parametrize("layer,name,variant", FINITE, ids=_ids(FINITE))
def test_the_loss_reaches_the_camera_and_the_exact_zeros_are_exact(layer, name, variant):
    cam = ce.expected(layer, name, variant)[2]
    zero = ce.EXACT_ZERO.get((layer, name), ())
    for k in zero:
        assert np.all(cam[k] == 0), k
    if set(zero) != set(ce.KEYS):
        assert any(np.abs(cam[k]).max() > 0 for k in ce.KEYS)
    else:
        c = ce.case(layer, name, variant)
        assert c["shape"][1:3] == (1, 1)               # both pixel scales are 0: the loss cannot reach the camera


@pytest.mark.parametrize("layer,name,variant", FINITE, ids=_ids(FINITE))
def test_a_second_summation_order_says_which_entries_are_rounding_noise(layer, name, variant):
    first, again = ce.expected(layer, name, variant)[2], ce.second(layer, name, variant)
    noise, top = ce.noise(layer, name, variant), ce.top(first)
    for k in ce.KEYS:
        a, b, n = first[k], again[k], noise[k]
        assert a.shape == b.shape and np.all(np.isfinite(b)), k
        diff, size = np.abs(a - b), np.maximum(np.abs(a), np.abs(b))
        print(f"{ce.tag(layer, name, variant)} {k}: two orders differ by {np.max(diff / np.maximum(size, 1e-300)):.3g} relative, "
              f"{diff.max() / max(top, 1e-300):.3g} of the camera's largest; {int(n.sum())} noise entries")
        assert np.all(size[n] <= 1e-9 * top), (k, np.argwhere(n))          # what is held by size is small
        assert np.all((diff <= 1e-10 * size) | (diff <= 1e-15 * top) | n), (k, diff, size)


@pytest.mark.parametrize("layer,name,variant", [i for i in ce.ALL if i[0] == "poisoned"],
                         ids=_ids([i for i in ce.ALL if i[0] == "poisoned"]))
def test_a_poisoned_batch_leaves_its_neighbours_the_gradients_they_have_alone(layer, name, variant):
    c, cam = ce.case(layer, name, variant), ce.expected(layer, name, variant)[2]
    sub = ce.poisoned_layer(name)
    for b in (0, 2):
        alone = ce._gradients(sub, ce.one_view(sub, c, b), variant)[2]
        for k in ce.KEYS:
            assert np.abs(alone[k]).max() > 0
            np.testing.assert_allclose(cam[k][b:b + 1], alone[k], rtol=1e-12, atol=0, err_msg=f"{name} view {b} {k}")
    # view 1 is the only one with a non-finite input
    inputs = [v for k, v in c.items() if isinstance(v, np.ndarray)] + list(c["upstream"].values())
    assert all(np.isfinite(v[[0, 2]]).all() for v in inputs) and any(not np.isfinite(v[1]).all() for v in inputs)


def test_the_named_surfels_of_zdepth_have_a_camera_space_z_of_exactly_zero():
    c = ce.case("project", "zdepth_16x12", True)
    cc = fo.world_to_cam_batched(torch.as_tensor(c["surfels"].astype(np.float64)), None, c["camera"])["pos"].numpy()
    named = list(ce.ZDEPTH_ROWS)
    assert len(named) == 12 and np.all(cc[0, named, 2] == 0)
    assert np.abs(np.delete(cc[0, :, 2], named)).min() > 1.0
    import frames_cases as fc
    assert fc.boundary_distance(c["surfels"], c["camera"]).min() >= fc.MARGIN
    # nonzero_divide's switch: the plane coordinates of such a surfel are f X and f Y, its gradient has no 1 / Z^2 term
    want, want_g, _ = ce.expected("project", "zdepth_16x12", False)
    f = float(c["camera"]["focal_length"])
    np.testing.assert_allclose(want["plane"][0, named, :2], f * cc[0, named, :2], rtol=1e-15)
    assert np.all(np.isfinite(want_g["surfels"]))


def test_the_named_surfels_of_the_dense_zdepth_case_have_z_zero_and_weigh_on_the_frame():
    import camera_chain_oracle as co
    c = ce.case("dense", "zdepth_9x7", ("grid", False))
    px = co.pixel_coordinates(torch.as_tensor(c["surfels"].astype(np.float64)), c["camera"]).numpy()[0]
    named = list(ce.DENSE_ZDEPTH_ROWS)
    W, H = 7, 9
    assert np.all(px[named, 2] == 0) and np.abs(np.delete(px[:, 2], named)).min() >= 1e-3
    assert np.all((px[named, 0] > 1) & (px[named, 0] < W - 1) & (px[named, 1] > 1) & (px[named, 1] < H - 1))
    # their gradient is the restatement's: X and Y move the loss, Z does not (nonzero_divide divides by 1 there)
    g = ce.expected("dense", "zdepth_9x7", ("grid", False))[1]["surfels"][0, named]
    assert np.all(np.abs(g[:, :2]).min() > 0) and np.all(g[:, 2] == 0)


def test_the_named_rows_of_w0_have_w_zero_and_bring_nothing_to_the_translation():
    c = ce.case("transform", "w0_153", "to_cam")
    rows = list(ce.W0_ROWS)
    assert len(rows) == 20 and np.all(c["pos"][:, rows, 3] == 0) and np.all(np.delete(c["pos"][..., 3], rows, axis=1) >= 0.5)
    # what the GPU test checks on these rows: grad_pos[..., 3] = g . M[:, 3] + g3
    for direction in ("to_cam", "to_world"):
        want, want_g, _ = ce.expected("transform", "w0_153", direction)
        w2c, c2w = fo._tables(c["camera"], torch.zeros(1, dtype=torch.float64))
        M = (w2c if direction == "to_cam" else c2w).numpy()
        g = c["upstream"]["pos"].astype(np.float64)
        np.testing.assert_allclose(want_g["pos"][..., 3], np.einsum("bnr,br->bn", g[..., :3], M[:, :, 3]) + g[..., 3], rtol=1e-12,
                                   atol=1e-14)


def test_the_counts_cases_have_one_lane_in_one_half_and_a_second_workgroup_of_one_lane_in_the_other():
    for name, (n_pos, n_normal) in (("counts_1_257", (1, 257)), ("counts_257_1", (257, 1))):
        c = ce.case("transform", name, "to_cam")
        assert c["pos"].shape == (2, n_pos, 4) and c["normal"].shape == (2, n_normal, 3)
    c = ce.case("transform", "b5_n1", "to_cam")
    assert c["pos"].shape == (5, 1, 4) and c["normal"].shape == (5, 1, 3)
