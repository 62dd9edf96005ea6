"""GPU: depth_to_surfels on the edge inputs of tests/surfels_edge_cases.py against the fp64 restatement tests/
surfels_oracle.py; tests/test_surfels_edge_cases_cpu.py shows that each case reaches the branch it is named for.

Stated tolerances, those of tests/test_hip_surfels.py: every coordinate and every gradient entry within its own bound
2^-24 |ref| + 2^-40 A + 2^-149 (tests/entry_checks.py, surfels_oracle.magnitudes), a non-finite entry of the restatement
met by the same NaN or the same infinity; beside it the older array-scale comparison, values rtol 2e-6 with atol 2e-7
max(|want|, 1), the gradient rtol 2e-6 with atol 2e-7 max|want|.  In the special cases one array holds 1e30 next to 2.0, so there the value bound is taken
PER PIXEL (atol 2e-7 max(max|want of that pixel|, 1)): never wider than the stated one.  The only elements compared
otherwise are the outputs of the two pixels surfels_edge_cases.NONFINITE names (depth +inf on the centre pixel, NaN),
which must be non-finite exactly where the restatement's are; their gradients are finite and held to the tolerance."""
import numpy as np
import pytest
import torch

import entry_checks as ec
import surfels_edge_cases as edges
import surfels_oracle as so
from projection_checks import ATOL_SCALE, RTOL, assert_bit_identical, compare_grads, compare_values
from test_hip_surfels import _hip

pytestmark = pytest.mark.gpu


def _view(c, b):
    return dict(c, depth=c["depth"][b:b + 1], shape=(1, *c["shape"][1:]), upstream={"pos": c["upstream"]["pos"][b:b + 1]},
                camera=dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in ("eye", "at", "up")}))


def _check_entries(c, got, got_g, want, want_g, tag):
    A, A_g, _ = so.magnitudes({"depth": c["depth"]}, c["camera"], c["upstream"], c["frame"])
    ec.check_all(got, want, A, tag + " values")
    ec.check_all(got_g, want_g, A_g, tag + " gradients")


def _compare_special(got, want, tag):
    """[N, 3] values pixel by pixel: the pixels of NONFINITE equal to the restatement's as non-finite values (NaN where
    NaN, -inf where -inf), every other one finite and within the stated tolerance at its own scale."""
    assert got.shape == want.shape
    for q in range(want.shape[0]):
        if q in edges.NONFINITE:
            assert not np.isfinite(want[q]).any(), (tag, q)
            assert np.array_equal(got[q], want[q], equal_nan=True), (tag, q, got[q], want[q])
        else:
            assert np.isfinite(want[q]).all() and np.isfinite(got[q]).all(), (tag, q, got[q])
            print(f"{tag} pixel {q}: max err {np.abs(got[q] - want[q]).max():.3g}, max|want| {np.abs(want[q]).max():.3g}")
            np.testing.assert_allclose(got[q], want[q], rtol=RTOL, atol=ATOL_SCALE * max(np.abs(want[q]).max(), 1.0),
                                       err_msg=f"{tag} pixel {q}")


@pytest.mark.parametrize("name", ["special_3x3", "special_3x3_camera"])
def test_special_depths(name):
    c = edges.case(name)
    got, got_g = _hip(c)
    want, want_g = edges.expected(name)
    _check_entries(c, got, got_g, want, want_g, name)
    _compare_special(got["pos"][0], want["pos"][0], name)
    compare_grads(got_g, want_g, name)                                  # every gradient is finite, NaN and +inf included
    rest = np.asarray(c["camera"]["eye"], np.float64)[0] if c["frame"] == "world" else np.zeros(3)
    for q in edges.DEAD:                                                # +0.0, -0.0, -inf
        assert np.array_equal(got["pos"][0, q], rest) and got_g["depth"][0, q] == 0, q
    full = edges.full_gradient(c)[0]
    for q in (2, 3, 4, 7):                                              # subnormal, smallest normal, +inf, NaN: alive
        assert got_g["depth"][0, q] != 0, q
        np.testing.assert_allclose(got_g["depth"][0, q], full[q], rtol=RTOL, atol=ATOL_SCALE * np.abs(full).max())


@pytest.mark.parametrize("name", ["row_1x300", "column_300x1", "b5_1x1"])
def test_values_and_gradients_match_the_restatement_and_a_batch_equals_its_views(name):
    c = edges.case(name)
    B, H, W = c["shape"]
    whole = _hip(c)
    want, want_g = edges.expected(name)
    _check_entries(c, whole[0], whole[1], want, want_g, name)
    compare_values(whole[0], want, name)
    compare_grads(whole[1], want_g, name)
    dead = c["depth"] <= 0
    assert dead.any() and np.all(whole[1]["depth"][dead] == 0)
    eye = np.broadcast_to(np.asarray(c["camera"]["eye"], np.float64)[:, None], (B, H * W, 3))
    assert np.array_equal(whole[0]["pos"][dead], eye[dead])
    for b in range(B):
        assert_bit_identical(whole, _hip(_view(c, b)), slice(b, b + 1))


@pytest.mark.parametrize("name", ["row_1x300", "column_300x1"])
def test_outputs_are_overwritten_not_accumulated(name, monkeypatch):
    """The kernels write every element: with torch.empty handing out NaN-filled buffers the results do not change."""
    c = edges.case(name)
    want = _hip(c)
    empty, empty_like = torch.empty, torch.empty_like

    def nan_filled(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(123)

    monkeypatch.setattr(torch, "empty", lambda *a, **k: nan_filled(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: nan_filled(empty_like(*a, **k)))
    got = _hip(c)
    assert np.all(np.isfinite(got[0]["pos"])) and np.all(np.isfinite(got[1]["depth"]))
    assert_bit_identical(want, got)
