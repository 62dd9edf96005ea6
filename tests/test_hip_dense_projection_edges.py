"""GPU: projection_renderer_differentiable on the edge inputs of tests/dense_projection_edge_cases.py against the fp64
restatement tests/dense_projection_oracle.py; tests/test_dense_projection_edge_cases_cpu.py shows that each case reaches
what it is named for and pins the restatement to the reference's own record on two of them.

Tolerances are the standing ones of tests/test_hip_dense_projection.py (projection_checks: rtol 2e-6, atol 2e-7
max(|want|, 1) for values and 2e-7 max|want| per gradient array), at the three sigma extremes as everywhere else: the
restatement's two formulations differ there by less than 2.7e-15 of each array's maximum (tests/
test_dense_projection_edge_cases_cpu.py), so the normalised `out` with a denormal mask is no worse conditioned than the
seeded frames and no per-case bound is needed.  The zero rows of the far surfels are compared exactly.  No element is
left out."""
import numpy as np
import pytest
import torch

import dense_projection_edge_cases as edges
from projection_checks import assert_bit_identical, compare_grads, compare_values
from test_hip_dense_projection import _hip

pytestmark = pytest.mark.gpu
# one_1x1: both pixel scales are 0 and the one weight is exp(0), so no coordinate moves and 1 - mask = 0
ZERO_BY_CONSTRUCTION = {"one_1x1": ("surfels", "rotated_image")}


@pytest.mark.parametrize("name,layout,rotated", edges.ALL)
def test_values_and_gradients_match_the_restatement(name, layout, rotated):
    c = edges.case(name, layout, rotated)
    tag = edges.tag(name, layout, rotated)
    got, got_g = _hip(c)
    want, want_g = edges.expected(name, layout, rotated)
    for a in list(got.values()) + list(got_g.values()):
        assert np.all(np.isfinite(a)), tag
    compare_values(got, want, tag)
    zero = ZERO_BY_CONSTRUCTION.get(name, ())
    compare_grads({k: g for k, g in got_g.items() if k not in zero}, {k: w for k, w in want_g.items() if k not in zero}, tag)
    for k in zero:
        if k in want_g:
            assert np.all(want_g[k] == 0) and np.all(got_g[k] == 0), (tag, k)
    if name == "far_9x7":                              # a surfel that weighs on no pixel gets exact zeros
        far = list(edges.FAR)
        D = c["shape"][3]
        assert np.all(got_g["surfels"][0, far] == 0) and np.all(got_g["rgb"].reshape(-1, D)[far] == 0)


@pytest.mark.parametrize("name", ["far_9x7", "tile_33x33"])
def test_every_element_is_written_and_the_overflowed_factor_never_is(name, monkeypatch):
    """With torch.empty and torch.empty_like handing out NaN-filled buffers -- the byte scratch as all-ones bytes, a NaN
    in every fp64 slot; the dense layer keeps no index in it -- the results do not change: no tile of far_9x7 picks up
    the NaN its far surfels' recurrence forms beyond the tile, and the one-pixel tiles of tile_33x33 write their
    pixels."""
    c = edges.case(name, "grid", False)
    want = _hip(c)
    empty, empty_like = torch.empty, torch.empty_like

    def nan_filled(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(255 if t.dtype == torch.uint8 else 123)

    monkeypatch.setattr(torch, "empty", lambda *a, **k: nan_filled(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: nan_filled(empty_like(*a, **k)))
    got = _hip(c)
    monkeypatch.undo()
    assert_bit_identical(want, got)
    for a in list(got[0].values()) + list(got[1].values()):
        assert not np.isnan(a).any()
