"""GPU: splat_regularizers on the edge inputs of tests/regularizer_edge_cases.py, against the fp64 restatement
(tests/regularizer_oracle.py), through the public call and with the helpers and the standing tolerance of
tests/test_hip_regularizers.py: values to rtol 2e-6 with atol 2e-7 max(|want|, 1), gradients to rtol 2e-6 with atol
2e-7 max|want| per input array -- per term under the one-hot weights.

    shapes        H = 2 / W = 2 with the other axis long; 65 workgroups per view, which is the first run of the second
                  trip of k_reg_finish's row loop; a batch of those against its views, bit for bit
    conventions   the exact zeros of edge.EXACT_ZEROS as == 0.0 on the fp32 results; const_pos; 1e19 and 1e-20 positions
    one-hot       each term's gradient alone; the arrays it does not reach exactly 0
    subsets       all fifteen requests of (pos, normal, image, depth) against the all-four call, bit for bit
    poison        a NaN or inf in one view: every term has the restatement's class (finite / +inf / -inf / NaN), the
                  other views are bit-identical to themselves run alone, the poisoned view's gradients are the
                  restatement's wherever tests/test_regularizer_edge_cases_cpu.py pins them finite (edge.finite_mask)
`-s` prints every figure; DESIGN.md 4c records the worst."""
import itertools

import numpy as np
import pytest

import regularizer_cases as cases
import regularizer_edge_cases as edge
import regularizer_oracle as ro
from test_hip_regularizers import _compare_grads, _compare_values, _hip

pytestmark = pytest.mark.gpu
TINY = float(np.finfo(np.float32).tiny)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _compare_masked(got, want, masks, tag):
    """_compare_grads where `masks` says the restatement is finite: the code under test must be finite there too."""
    for k in ro.INPUTS:
        m, w = masks[k], want[k]
        assert got[k].shape == w.shape and np.all(np.isfinite(w[m])) and m.any(), (tag, k)
        assert np.all(np.isfinite(got[k][m])), (tag, k)
        top = np.abs(w[m]).max()
        print(f"{tag} grad {k}: {int(m.sum())} of {m.size} compared, max err / max|want| "
              f"{np.abs(got[k][m] - w[m]).max() / top:.3g}")
        np.testing.assert_allclose(got[k][m], w[m], rtol=2e-6, atol=2e-7 * top, err_msg=f"{tag} grad {k}")


@pytest.mark.parametrize("name", edge.SHAPE_NAMES)
def test_shapes_match_the_restatement_and_repeat_bit_for_bit(name):
    c = edge.case(name)
    got, got_g = _hip(c)
    want, want_g = edge.expected(name)
    _compare_values(got, want, name)
    _compare_grads(got_g, want_g, name)
    again, again_g = _hip(c)
    for k in ro.TERMS:
        assert np.array_equal(got[k], again[k]), k
    for k in ro.INPUTS:
        assert np.array_equal(got_g[k], again_g[k]), k


def test_a_65_workgroup_batch_equals_its_views_bit_for_bit():
    c = edge.case("130x127_b3")
    assert edge.nblk(c) == 65
    v, g = _hip(c)
    for b in range(3):
        v1, g1 = _hip(edge.view(c, b))
        for k in ro.TERMS:
            assert np.array_equal(v[k][b:b + 1], v1[k]), (b, k)
        for k in ro.INPUTS:
            assert np.array_equal(g[k][b:b + 1], g1[k]), (b, k)


@pytest.mark.parametrize("name", edge.CONVENTION_NAMES)
def test_conventions_match_the_restatement(name):
    c = edge.case(name)
    got, got_g = _hip(c)
    want, want_g = edge.expected(name)
    _compare_values(got, want, name)
    _compare_grads(got_g, want_g, name)
    if name == "huge_pos":                   # the other pixels against their own largest entry, not the huge pixel's
        far = np.broadcast_to(~edge.block(c, *edge.PIXEL), c["depth"].shape)
        _compare_masked(got_g, want_g, {k: far for k in ro.INPUTS}, "huge_pos outside the block")
    if name in ("huge_pos", "tiny_pos"):     # nothing overflows, is lost or flushed where fp32 can hold the result
        for k in ro.TERMS:
            ok = (np.abs(want[k]) >= TINY) & (np.abs(want[k]) <= 3e38)
            assert np.all(np.isfinite(got[k])) and np.all(got[k][ok] != 0.0), (name, k)
        for k in ro.INPUTS:
            ok = np.abs(want_g[k]) >= TINY
            assert np.all(np.isfinite(got_g[k])) and np.all(got_g[k][ok] != 0.0), (name, k)
    if name == "const_pos":
        assert abs(got["spatial_var"][0] - 1e4) <= 2e-6 * 1e4
        assert got["spatial"][0] == 0.0 and got["normal_consistency"][0] == 0.0


@pytest.mark.parametrize("spec", edge.EXACT_ZEROS, ids=[f"{s[0]}-{s[1]}-{s[3]}" for s in edge.EXACT_ZEROS])
def test_the_conventions_are_exact_zeros(spec):
    name, term, keys, mark = spec
    c = edge.one_hot(edge.case(name), term)
    pixels = c["marks"][mark]
    assert len(pixels) > 0
    _, g = _hip(c)
    for k in keys:
        for (i, j) in pixels:
            assert np.all(g[k][0, i, j] == 0.0), (name, term, k, (i, j), g[k][0, i, j])
        if len(pixels) < c["depth"][0].size:
            assert np.any(g[k] != 0.0), (name, term, k)                              # the term is not switched off


@pytest.mark.parametrize("name", edge.ONEHOT_NAMES)
def test_one_term_alone(name):
    term = ro.TERMS[edge.ONEHOT_NAMES.index(name)]
    got, got_g = _hip(edge.case(name))
    want, want_g = edge.expected(name)
    _compare_values(got, want, name)
    reached = {k: want_g[k] for k in ro.INPUTS if k in edge.REACH[term]}
    assert all(np.abs(w).max() > 0 for w in reached.values())
    _compare_grads({k: got_g[k] for k in reached}, reached, name)                     # to this term's own max|want|
    for k in ro.INPUTS:
        if k not in reached:
            assert np.all(got_g[k] == 0.0), (name, k)


def test_every_subset_of_requested_gradients():
    c = cases.case("3x5")
    _, whole = _hip(c)
    for n in range(1, 5):
        for wrt in itertools.combinations(ro.INPUTS, n):
            _, g = _hip(c, wrt=wrt)
            for k in ro.INPUTS:
                if k in wrt:
                    assert np.array_equal(g[k], whole[k]), (wrt, k)
                else:
                    assert g[k] is None, (wrt, k)


@pytest.mark.parametrize("name", edge.POISONED_NAMES)
def test_poison_stays_in_its_view_and_propagates_as_in_the_restatement(name):
    c = edge.case(name)
    got, got_g = _hip(c)
    want, want_g = edge.expected(name)
    for k in ro.TERMS:
        print(f"{name} {k}: got {got[k]} want {want[k]}")
    for k in ro.TERMS:
        assert list(edge.classify(want[k])) == ["finite", edge.PINS[name]["terms"][k], "finite"], k
        assert list(edge.classify(got[k])) == list(edge.classify(want[k])), (name, k, got[k], want[k])
        fin = np.isfinite(want[k])
        np.testing.assert_allclose(got[k][fin], want[k][fin], rtol=2e-6, atol=2e-7 * max(np.abs(want[k][fin]).max(), 1.0),
                                   err_msg=f"{name} {k}")
    _compare_masked(got_g, want_g, {k: edge.finite_mask(name, k) for k in ro.INPUTS}, name)
    for b in (0, 2):
        v1, g1 = _hip(edge.view(c, b))
        for k in ro.TERMS:
            assert np.array_equal(got[k][b:b + 1], v1[k]), (b, k)
        for k in ro.INPUTS:
            assert np.array_equal(got_g[k][b:b + 1], g1[k]), (b, k)
    again, again_g = _hip(c)
    for k in ro.TERMS:
        assert _same(got[k], again[k]), k
    for k in ro.INPUTS:
        assert _same(got_g[k], again_g[k]), k
