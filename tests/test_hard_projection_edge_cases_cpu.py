"""Each case of tests/hard_projection_edge_cases.py reaches the branch it is named for, shown with the fp64 restatement
(tests/hard_projection_oracle.py, projection_oracle.pixel_coordinates) alone; and the restatement against the reference's
own projection_renderer on the two tie cases (tests/golden/hard_projection/hp2_tie_*.npz, recorded by tools/
gen_hard_projection_golden.py): that record is what ties "ties to even (torch.round)" to the reference and not only to the
restatement.  The fixtures carry the prefix hp2_ because tests/test_hard_projection_oracle_cpu.py holds the hp1_ files to
exactly the seeded cases.  Runs without a GPU."""
import os

import numpy as np
import pytest
import torch

import hard_projection_edge_cases as edges
import hard_projection_oracle as ho
from conftest import GOLDEN_DIR
from projection_checks import ATOL_SCALE, RTOL

DIR = os.path.join(GOLDEN_DIR, "hard_projection")


def _uv(c):
    p = edges.pixels(c)
    return p[..., 0] - 0.5, p[..., 1] - 0.5


@pytest.mark.parametrize("name,index", [("tie_4x6", 14), ("tie_6x4", 10)])
def test_the_named_surfels_tie_exactly_and_land_on_the_even_pixel(name, index):
    c = edges.case(name)
    B, H, W, D = c["shape"]
    u, v = _uv(c)
    for s in edges.TIE_BOTH + edges.TIE_U:
        assert u[0, s] == W / 2 - 0.5 and u[0, s] - np.floor(u[0, s]) == 0.5, s
    for s in edges.TIE_BOTH + edges.TIE_V:
        assert v[0, s] == H / 2 - 0.5 and v[0, s] - np.floor(v[0, s]) == 0.5, s
    z = edges.pixels(c)[0, :3, 2]
    assert z[0] > 0 and z[1] < 0 and z[2] == 0                         # -Z: in front, behind, Z = 0 (divided by 1)
    val, grad = edges.expected(name)
    assert list(val["index"][0, :3]) == [index] * 3
    even_u, even_v = {6: 2, 4: 2}[W], {4: 2, 6: 2}[H]                  # 2.5 -> 2 (down), 1.5 -> 2 (up)
    assert index == even_v * W + even_u
    assert val["index"][0, 3] % W == even_u and val["index"][0, 3] < H * W
    assert val["index"][0, 4] // W == even_v and val["index"][0, 4] < H * W
    # floor(x + 1/2), the usual shortcut, sends the 2.5 to 3: another pixel on the side that ties downwards
    wrong = int(np.floor(v[0, 0] + 0.5)) * W + int(np.floor(u[0, 0] + 0.5))
    assert wrong != index and 0 <= wrong < H * W
    assert val["count"][0, index] >= 3 and np.all(grad["rgb"].reshape(H * W, D)[:3] != 0)
    # every other surfel is clear of every kink, and so is the free coordinate of the two half-tied ones
    assert edges.margin(c, c["named"]) >= 1.0
    p = edges.pixels(c)[0]
    free = np.array([p[3, 1], p[4, 0]])
    assert np.abs(free - np.round(free)).min() >= 1e-4 and np.abs(p[3:, 2]).min() >= 1e-3


@pytest.mark.parametrize("name", edges.RECORDED)
def test_the_restatement_matches_the_recorded_reference_on_the_ties(name):
    npz = np.load(os.path.join(DIR, f"hp2_{name}.npz"), allow_pickle=False)
    c = edges.case(name)
    for k in ho.INPUTS:
        assert c[k].dtype == np.float32 and np.array_equal(npz["in/" + k], c[k]), k
    for k in ("eye", "at", "up", "viewport", "fovy", "focal_length"):
        assert np.array_equal(npz["in/camera/" + k], np.asarray(c["camera"][k])), k
    assert np.array_equal(npz["grad_in/out"], c["upstream"]["out"])
    val, grad = edges.expected(name)
    N = val["index"].shape[1]
    for p in ("ref64/", "ref32/"):                                     # decisions: exact, the tied surfels included
        assert np.array_equal(val["index"], npz[p + "index"]), (name, p)
        assert np.array_equal(val["mask"], npz[p + "mask"]), (name, p)
        assert np.array_equal(val["count"][0], np.bincount(npz[p + "index"][0], minlength=N + 1)[:N]), (name, p)
    for k, got in (("out", val["out"]), ("grad/rgb", grad["rgb"])):
        want = npz["ref64/" + k]
        assert want.dtype == np.float64 and want.shape == got.shape and np.all(np.isfinite(want)), (name, k)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (name, k)
        w32 = npz["ref32/" + k].astype(np.float64)
        scale = max(np.abs(want).max(), 1.0) if k == "out" else np.abs(want).max()
        np.testing.assert_allclose(w32, want, rtol=RTOL, atol=ATOL_SCALE * scale, err_msg=f"{name} {k}")
    largest = max(os.path.getsize(os.path.join(DIR, f)) for f in os.listdir(DIR) if f.startswith("hp1_"))
    assert os.path.getsize(os.path.join(DIR, f"hp2_{name}.npz")) <= largest


def test_edges_5x7_enters_the_border_pixels_from_outside_the_centres():
    c = edges.case("edges_5x7")
    B, H, W, D = c["shape"]
    u, v = _uv(c)
    val, grad = edges.expected("edges_5x7")
    bands = ((u[0] > -0.5) & (u[0] < 0), (u[0] > W - 1) & (u[0] < W - 0.5),
             (v[0] > -0.5) & (v[0] < 0), (v[0] > H - 1) & (v[0] < H - 0.5))
    for band, pair in zip(bands, ((0, 1), (2, 3), (4, 5), (6, 7))):
        assert band[list(pair)].all() and band.sum() >= 2
    idx = val["index"][0]
    assert np.all(idx[:8] < H * W) and np.all(grad["rgb"].reshape(H * W, D)[:8] != 0)        # all of them are counted
    assert np.all(idx[0:2] % W == 0) and np.all(idx[2:4] % W == W - 1)
    assert np.all(idx[4:6] // W == 0) and np.all(idx[6:8] // W == H - 1)
    assert np.signbit(np.round(u[0, 0])) and np.round(u[0, 0]) == 0                          # rint's -0.0
    assert edges.margin(c) >= 1.0


def test_nonfinite_4x6_drops_every_named_surfel_and_leaks_no_nan():
    c = edges.case("nonfinite_4x6")
    B, H, W, D = c["shape"]
    N = H * W
    s = c["surfels"][0, :8]
    assert np.isnan(s).any() and (s == np.inf).any() and (s == -np.inf).any()
    assert (np.abs(s) == np.float32(1e30)).any() and (np.abs(s) == np.float32(3e38)).any()
    assert not np.isfinite(c["surfels"][0, :8]).all(axis=-1).all() and np.isfinite(c["surfels"][0, 8:]).all()
    val, grad = edges.expected("nonfinite_4x6")
    assert np.all(val["index"][0, :8] == N)
    assert np.isnan(c["rgb"].reshape(N, D)[0]).all() and np.isfinite(c["rgb"].reshape(N, D)[1:]).all()
    up = c["upstream"]["out"].reshape(N, D)
    assert np.isnan(up[list(edges.NONFINITE_UPSTREAM)]).all() and np.isnan(up).any(axis=1).sum() == 2
    assert np.all(val["count"][0, list(edges.NONFINITE_UPSTREAM)] == 0)
    for a in (val["out"], grad["rgb"]):
        assert np.all(np.isfinite(a))
    assert np.all(grad["rgb"].reshape(N, D)[:8] == 0) and (val["index"][0, 8:] < N).any()
    assert edges.margin(c, c["named"]) >= 1.0


def test_the_all_dropped_views_hold_nothing_but_dropped_keys():
    for name in ("all_dropped_3x5", "all_dropped_b2"):
        c = edges.case(name)
        B, H, W, D = c["shape"]
        val, grad = edges.expected(name)
        assert np.all(val["index"][0] == H * W) and np.all(val["out"][0] == 0) and val["mask"][0].all()
        assert np.all(grad["rgb"][0] == 0) and np.all(val["count"][0] == 0)
        z = edges.pixels(c)[0, :, 2]
        assert (z < 0).any() and (z > 0).any()                         # behind the camera and in front of it
        assert edges.margin(c) >= 1.0
    val, grad = edges.expected("all_dropped_b2")
    assert not val["mask"][1].all() and val["count"][1].sum() > 7 and np.abs(grad["rgb"][1]).max() > 0


@pytest.mark.parametrize("name,pixel", [("cluster_last_8x8", 63), ("cluster_first_8x8", 0)])
def test_the_clusters_fill_the_last_and_the_first_pixel(name, pixel):
    c = edges.case(name)
    val, grad = edges.expected(name)
    assert np.array_equal(np.unique(val["index"]), [pixel]) and val["count"][0, pixel] == 64
    assert val["mask"].reshape(64, 3).all(axis=1).sum() == 63 and not val["mask"].reshape(64, 3)[pixel].any()
    np.testing.assert_allclose(val["out"].reshape(64, 3)[pixel], c["rgb"].astype(np.float64).reshape(64, 3).mean(0),
                               rtol=1e-14)
    assert edges.margin(c) >= 1.0


def test_torch_round_ties_to_even_on_both_sides():
    assert torch.round(torch.tensor([1.5, 2.5, -0.5, -0.25], dtype=torch.float64)).tolist() == [2.0, 2.0, -0.0, -0.0]
