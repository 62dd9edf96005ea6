"""What tests/sh9_cases.py promises of its cases: the arrays by hash (the fixtures under tests/golden/sh_lighting were
recorded on them), the shapes at the kernels' seams, and how much of every probe lies inside the disc.  No GPU.

The share inside the disc: at least half for every recorded square probe (the reference's own 16 x 16 has 195 of 256,
76 %).  The 12 x 20 probe exists for the swapped-axis quirk -- rows scaled by W, columns by H -- and that very quirk
stretches u to 2.17 and pushes columns 13 .. 19 out of the disc: 110 of its 240 pixels are inside, 45.8 %, and no
12 x 20 or 20 x 12 probe has more.  Its count is pinned exactly; the one-pixel probe has none inside."""
import hashlib

import numpy as np
import pytest

import sh9_cases as cases
import sh9_oracle as oracle

P_ALL, I_ALL = range(len(cases.PROJECTION)), range(len(cases.IRRADIANCE))
P_SUMS = {"p16x16x3": "2bb6e3afa7f92b74", "p12x20x3": "d4f86041a424e403", "p15x15x1": "db159255f9c2348f",
          "p5x5x4": "b9efa9a9958b0a75", "p40x40x3": "4a8763b9c36e79a6", "p1x1x3": "6a14106a6d84ebdd"}
I_SUMS = {"n1_c3_zonal_views": "45126a7004294e33", "n63_c1_random_shared": "ef978736f1e36ac9",
          "n64_c4_zonal_shared": "e329117dde973507", "n257_c3_random_views": "b07838664cfa46a8",
          "n1025_c4_random_shared": "2e852fcb24785bf7", "n1025_c1_zonal_views": "e9304d70292ed9c0",
          "n257_c4_zonal_views": "469adb060af585f3", "n64_c3_random_views": "e65c66d6016ba366"}
INSIDE = {(16, 16): 195, (12, 20): 110, (15, 15): 172, (5, 5): 16, (40, 40): 1255, (1, 1): 0, (136, 136): 14503}


@pytest.mark.parametrize("k", P_ALL, ids=cases.projection_tag)
def test_a_projection_case_is_pinned(k):
    H, W, C, B = cases.PROJECTION[k]
    c = cases.projection(k)
    assert c["envmap"].shape == (B, H, W, C) and c["envmap"].dtype == np.float32
    assert c["g_L"].shape == (B, C, 9) and c["g_L"].dtype == np.float32
    assert c["envmap"].min() >= 0 and c["envmap"].max() <= 2 and np.abs(c["g_L"]).max() < 1
    assert cases.checksum(c, ("envmap", "g_L")) == P_SUMS[cases.projection_tag(k)]
    assert not c["envmap"].flags.writeable


@pytest.mark.parametrize("k", I_ALL, ids=cases.irradiance_tag)
def test_an_irradiance_case_is_pinned(k):
    N, C, kind, per_view = cases.IRRADIANCE[k]
    c = cases.irradiance(k)
    assert c["M"].shape == ((cases.VIEWS, 4, 4, C) if per_view else (4, 4, C))
    assert c["normal"].shape == (cases.VIEWS, N, 3) and c["g_E"].shape == (cases.VIEWS, N, C)
    assert all(c[key].dtype == np.float32 for key in ("L", "M", "normal", "g_E"))
    assert cases.checksum(c, ("L", "M", "normal", "g_E")) == I_SUMS[cases.irradiance_tag(k)]
    length = np.linalg.norm(c["normal"].astype(np.float64), axis=-1)
    unit = length[:, 0::2].copy()
    if (N - 1) % 2 == 0:
        unit[-1, -1] = 1.0                                                                          # the zero row is even
    assert (np.abs(unit - 1) < 1e-6).all()                                                          # unit rows
    assert (c["normal"][-1, -1] == 0).all() and (length.ravel()[:-1] > 0.1).all()                   # one exactly zero
    if N > 2:
        assert (np.abs(length[:, 1::2] - 1) > 1e-3).any()                                           # not normalised
    sym = np.array_equal(c["M"], np.swapaxes(c["M"], -3, -2))
    assert sym == (kind == "zonal")


def test_the_cases_cover_what_the_kernels_branch_on():
    assert cases.PROJECTION == [(16, 16, 3, 2), (12, 20, 3, 2), (15, 15, 1, 1), (5, 5, 4, 3), (40, 40, 3, 2), (1, 1, 3, 1)]
    assert {s[0] for s in cases.IRRADIANCE} == {1, 63, 64, 257, 1025} and {s[1] for s in cases.IRRADIANCE} == {1, 3, 4}
    assert {s[2] for s in cases.IRRADIANCE} == {"zonal", "random"} and {s[3] for s in cases.IRRADIANCE} == {True, False}
    groups = lambda n: -(-n // 256)                                     # noqa: E731
    assert groups(40 * 40) == 7 and groups(136 * 136) == 73 and groups(cases.ORACLE_ONLY_N[0]) == 67      # 64 rows wrap
    assert cases.GRID_DIMS == [(6, 6), (5, 8)]


@pytest.mark.parametrize("shape", sorted(INSIDE))
def test_the_share_of_every_probe_inside_the_disc(shape):
    inside = oracle.grid(*shape)["inside"]
    assert int(inside.sum()) == INSIDE[shape]
    if shape[0] == shape[1] and shape != (1, 1):
        assert 2 * INSIDE[shape] >= shape[0] * shape[1]
    if shape == (16, 16):
        assert inside[8, 8] and oracle.grid(16, 16)["theta"][8, 8] == 0             # the r = 0 pixel
    if shape == (5, 5):
        assert INSIDE[shape] < 64                                                    # fewer than a wave
    if shape == (12, 20):
        assert not inside[:, 13:].any() and inside[:, :13].sum() == 110              # what the swapped scales cost


def test_the_lightprobe_file_is_pinned():
    raw = cases.lightprobe_bytes()
    assert len(raw) == 4 * 4 * 3 * 4 and hashlib.sha256(raw).hexdigest()[:16] == "1cf7972d39f46852"
    assert (np.frombuffer(raw, "<f4") < 0).any()
