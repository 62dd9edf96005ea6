"""What the fp64 restatement (tests/regularizer_oracle.py) says of every edge case of tests/regularizer_edge_cases.py,
pinned here on the CPU: that each case meets the condition it exists for, that it keeps the kink margin outside its
`flat` pixels, and -- for the poisoned batches -- the class (finite / +inf / -inf / NaN) of every term of every view and
exactly which gradient entries are finite.  tests/test_regularizers_host_cpu.py and tests/test_hip_regularizers_edges.py
take their "compare here" masks from these pins (edge.PINS through edge.finite_mask), not from the code under test."""
import numpy as np
import pytest
import torch

import regularizer_cases as cases
import regularizer_edge_cases as edge
import regularizer_oracle as ro


def _f64(c, key, b=0):
    return torch.tensor(c[key][b].astype(np.float64))


def _pos_differences(c, b=0):
    return ro.neighbour_differences(_f64(c, "pos", b)).numpy()                    # (8, H, W, 3)


@pytest.mark.parametrize("name", edge.NAMES)
def test_the_case_keeps_the_contract_and_the_kink_margin(name):
    c = edge.case(name)
    B, H, W = c["depth"].shape
    for k in ro.INPUTS:
        assert c[k].dtype == np.float32 and c[k].shape == ((B, H, W, 3) if k != "depth" else (B, H, W)), k
    assert c["weights"].dtype == np.float32 and c["weights"].shape == (B, 7)
    assert c["z_min"] <= c["z_max"] and not c["single"]
    assert c["flat"] is None or (c["flat"].shape == (H, W) and c["flat"].dtype == bool)
    assert len(c["margins"]) == B and min(c["margins"]) >= edge.MARGIN            # measured when the case was drawn
    if H * W <= 1000:                                                            # and again here, where it is cheap
        assert edge.margins(c) == c["margins"]
    if c["poison"] is None:
        assert all(np.all(np.isfinite(c[k])) for k in ro.INPUTS)


@pytest.mark.parametrize("name,shape,n", [("2x300", (1, 2, 300), 3), ("300x2", (1, 300, 2), 3),
                                          ("2x8257_b2", (2, 2, 8257), 65), ("129x128", (1, 129, 128), 65),
                                          ("130x127_b3", (3, 130, 127), 65)])
def test_shape_cases_reach_their_branch(name, shape, n):
    c = edge.case(name)
    assert c["depth"].shape == shape and edge.nblk(c) == n and c["flat"] is None
    if n == 65:                     # the finish kernel's lane 0 adds two rows, lane 1 one
        assert len(range(0, n, 64)) == 2 and len(range(1, n, 64)) == 1
    if name == "130x127_b3":
        assert (shape[1] * shape[2]) % 256 != 0
        assert len({tuple(w) for w in c["weights"]}) == 3


def test_onehot_cases_are_17x9_b3_with_one_term():
    base = cases.case("17x9_b3")
    for k, name in enumerate(edge.ONEHOT_NAMES):
        c = edge.case(name)
        for key in ro.INPUTS:
            assert np.array_equal(c[key], base[key])
        assert np.array_equal(c["weights"][:, k], base["weights"][:, k]) and np.all(c["weights"][:, k] != 0)
        assert np.count_nonzero(c["weights"]) == 3
    # what each term reaches, in the restatement: the other arrays' gradients are exactly 0
    reach = {"z": {"pos"}, "unit_normal": {"normal"}, "normal_consistency": {"pos", "normal"}, "spatial": {"pos"},
             "spatial_var": {"pos"}, "image_depth_consistency": {"image", "depth"}, "away_from_camera": {"pos", "normal"}}
    assert reach == edge.REACH
    for name, term in zip(edge.ONEHOT_NAMES, ro.TERMS):
        _, g = edge.expected(name)
        for key in ro.INPUTS:
            assert (np.abs(g[key]).max() > 0) == (key in reach[term]), (name, key)


def test_convention_cases_hit_their_conventions():
    i, j = edge.PIXEL
    c = edge.case("coincident_3x3")
    block = c["pos"][0, i - 1:i + 2, j - 1:j + 2].reshape(9, 3)
    assert np.all(block == block[0]) and int(c["flat"].sum()) == 9
    assert int(np.all(c["pos"][0] == block[0], axis=-1).sum()) == 9                # exactly nine coincident positions
    d = _pos_differences(c)
    assert np.all(d[:, i, j] == 0.0)                                             # all eight d_k of the centre
    assert int(np.all(d == 0.0, axis=-1).sum()) == 40                            # 8 + 4 * 5 + 4 * 3 ordered pairs

    c = edge.case("origin")
    assert np.all(c["pos"][0, i, j] == 0.0) and int(np.all(c["pos"][0] == 0.0, axis=-1).sum()) == 1

    c = edge.case("pz_zero")
    assert c["pos"][0, i, j, 2] == 0.0 and np.all(c["pos"][0, i, j, :2] != 0.0)
    assert int((c["pos"][0, ..., 2] == 0.0).sum()) == 1

    c = edge.case("n_dot_p_zero")
    p, n = c["pos"][0, i, j].astype(np.float64), c["normal"][0, i, j].astype(np.float64)
    assert tuple(p) == (0.0, 1.0, -3.0) and tuple(n) == (1.0, 0.0, 0.0) and float(np.dot(n, p)) == 0.0

    c = edge.case("zmin_eq_zmax")
    assert c["z_min"] == c["z_max"] == 3.0 and c["pos"][0, i, j, 2] == -3.0
    assert int((np.abs(c["pos"][0, ..., 2]) == 3.0).sum()) == 1

    c = edge.case("const_pos")
    assert np.all(c["pos"][0] == np.float32(edge.CONST_POINT)) and c["flat"].all()
    v, _ = edge.expected("const_pos")
    assert v["spatial_var"][0] == 1e4 and v["spatial"][0] == 0.0 and v["normal_consistency"][0] == 0.0

    c = edge.case("huge_pos")
    assert np.array_equal(c["pos"][0, i, j], np.float32(edge.HUGE_POINT)) and c["flat"] is None
    assert np.abs(np.delete(c["pos"][0].reshape(-1, 3), i * 7 + j, axis=0)).max() < 5.0

    c = edge.case("tiny_pos")
    assert c["z_min"] == 0.0 and 1.5e-20 <= np.abs(c["pos"][..., 2]).min() and np.abs(c["pos"]).max() < 5e-20
    assert np.abs(c["pos"]).min() > np.finfo(np.float32).tiny                       # normal fp32 numbers

    for name, (H, W) in (("corner_conventions_2x5", (2, 5)), ("corner_conventions_5x2", (5, 2))):
        c = edge.case(name)
        assert c["depth"].shape == (1, H, W)
        corners = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
        assert corners <= set(c["designed"])                                     # all four corners carry a convention
        assert set(c["marks"]["still_corners"]) < corners and len(c["marks"]["still_corners"]) == 2
        a = ro.neighbour_differences(_f64(c, "image").mean(dim=-1, keepdim=True))[..., 0].numpy()
        e = ro.neighbour_differences(_f64(c, "depth")[..., None])[..., 0].numpy()
        for p in c["marks"]["still_corners"]:
            assert np.all(a[(slice(None),) + p] == 0.0) and np.all(e[(slice(None),) + p] == 0.0)    # all eight pairs
        az = [abs(float(c["pos"][(0,) + p + (2,)])) for p in c["marks"]["z"]]
        assert az == [c["z_min"], c["z_max"], c["z_min"]]
        assert len(set(c["marks"]["z"]) & corners) == 2 and len(set(c["marks"]["z"]) - corners) == 1


@pytest.mark.parametrize("name", edge.CONVENTION_NAMES + edge.SHAPE_NAMES + edge.ONEHOT_NAMES)
def test_everything_is_finite_without_poison(name):
    v, g = edge.expected(name)
    assert all(np.all(np.isfinite(v[k])) for k in ro.TERMS)
    assert all(np.all(np.isfinite(g[k])) for k in ro.INPUTS)
    assert all(edge.finite_mask(name, k).all() for k in ro.INPUTS)


@pytest.mark.parametrize("name", edge.POISONED_NAMES)
def test_poisoned_batches_are_pinned(name):
    c = edge.case(name)
    key, b, i, j, comp, was = c["poison"]
    assert c["depth"].shape == (3, 6, 7) and b == 1 and np.isfinite(was)
    bad = ~np.isfinite(c[key])
    assert int(bad.sum()) == 1 and bad[(b, i, j) if comp is None else (b, i, j, comp)]
    assert all(np.all(np.isfinite(c[k])) for k in ro.INPUTS if k != key)
    assert (i, j) == ((0, 0) if name == "nan_pos_corner" else edge.PIXEL)
    v, g = edge.expected(name)
    for t in ro.TERMS:
        assert list(edge.classify(v[t])) == ["finite", edge.PINS[name]["terms"][t], "finite"], t
    for k in ro.INPUTS:
        assert np.array_equal(np.isfinite(g[k]), edge.finite_mask(name, k)), k
        assert edge.finite_mask(name, k)[[0, 2]].all(), k                          # the outer views: everything
    # the cap: the half that does not read the poisoned input is compared in full
    for k in ({"pos": ("image", "depth"), "normal": ("image", "depth"), "image": ("pos", "normal"),
               "depth": ("pos", "normal")}[key]):
        assert edge.PINS[name]["grads"][k] == "all" and edge.finite_mask(name, k).all(), k


def test_the_pins_say_what_was_measured():
    """The structure the pins were written from, spelled out once more without edge.PINS."""
    nan5 = {"z", "normal_consistency", "spatial", "spatial_var", "away_from_camera"}
    for name in ("nan_pos", "nan_pos_corner"):
        v, g = edge.expected(name)
        c = edge.case(name)
        _, _, i, j, _, _ = c["poison"]
        assert {t for t in ro.TERMS if np.isnan(v[t][1])} == nan5
        assert np.isfinite(v["unit_normal"][1]) and np.isfinite(v["image_depth_consistency"][1])
        assert not np.isfinite(g["pos"][1]).any()                                  # no pos gradient is finite
        block = edge.block(c, i, j)
        assert int(block.sum()) == (9 if name == "nan_pos" else 4)
        assert np.isfinite(g["normal"][1][~block]).all() and not np.isfinite(g["normal"][1][block]).any()
        assert np.isfinite(g["image"]).all() and np.isfinite(g["depth"]).all()
    v, g = edge.expected("inf_depth")
    assert v["image_depth_consistency"][1] == np.inf and all(np.isfinite(g[k]).all() for k in ro.INPUTS)
    v, g = edge.expected("nan_image")
    assert np.isnan(v["image_depth_consistency"][1]) and all(np.isfinite(g[k]).all() for k in ro.INPUTS)
    v, g = edge.expected("inf_normal")
    assert v["unit_normal"][1] == v["normal_consistency"][1] == v["away_from_camera"][1] == np.inf


def test_outer_views_of_a_poisoned_batch_are_the_views_alone():
    for name in edge.POISONED_NAMES:
        c = edge.case(name)
        v, g = edge.expected(name)
        for b in (0, 2):
            one = edge.view(c, b)
            v1, g1 = ro.gradients({k: one[k] for k in ro.INPUTS}, one["weights"], c["z_min"], c["z_max"], c["z_scale"],
                                  c["unit_normal_scale"])
            for t in ro.TERMS:
                np.testing.assert_allclose(v1[t][0], v[t][b], rtol=1e-12, err_msg=f"{name} {b} {t}")   # torch's sum order
            for k in ro.INPUTS:
                np.testing.assert_allclose(g1[k][0], g[k][b], rtol=0, atol=1e-12 * np.abs(g[k][b]).max(),
                                           err_msg=f"{name} {b} {k}")
