"""tests/regularizer_oracle.py against the reference's own functions, recorded in float64 (tests/golden/regularizers/
r1_*.npz, tools/gen_regularizer_golden.py): values and input gradients.

Tolerance: both sides are fp64 evaluations of the same formulas in a different summation order; over the 2^15 terms
of the largest mean the worst case is about 4e-12, so rtol 1e-9 with atol 1e-9 max|want| leaves more than 100x.

Also the kink condition of every seeded case (tests/regularizer_cases.py), which is what lets the GPU comparison
(tests/test_hip_regularizers.py) leave no element out."""
import glob
import os

import numpy as np
import pytest
import torch

import regularizer_cases as cases
import regularizer_oracle as ro
from conftest import GOLDEN_DIR

FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, "regularizers", "r1_*.npz")))


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, "regularizers", name + ".npz"), allow_pickle=False)


def test_the_fixtures_are_there():
    assert len(FIXTURES) >= 6
    for name in FIXTURES:
        npz = _load(name)
        assert npz["in/depth"].shape[1] <= 36 and npz["in/depth"].shape[2] <= 48, name
        assert np.all(npz["weights"] != 0), name
        for k in ro.INPUTS:
            assert npz["in/" + k].dtype == np.float32, (name, k)


@pytest.mark.parametrize("name", FIXTURES)
def test_values_and_gradients_match_the_reference(name):
    npz = _load(name)
    x = {k: npz["in/" + k] for k in ro.INPUTS}
    values, grads = ro.gradients(x, npz["weights"], float(npz["in/z_min"]), float(npz["in/z_max"]),
                                 float(npz["in/z_scale"]), float(npz["in/unit_normal_scale"]))
    for k in ro.TERMS:
        want = npz["ref/" + k]
        np.testing.assert_allclose(values[k], want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=f"{name} {k}")
    for k in ro.INPUTS:
        want = npz["grad/" + k]
        assert np.all(np.isfinite(want)) and np.abs(want).max() > 0, (name, k)
        np.testing.assert_allclose(grads[k], want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=f"{name} grad {k}")


@pytest.mark.parametrize("name", FIXTURES)
def test_a_fixture_holds_the_inputs_of_its_seeded_case(name):
    npz, c = _load(name), cases.case(name[3:])
    for k in ro.INPUTS + ("weights",):
        assert np.array_equal(npz[k if k == "weights" else "in/" + k], c[k]), (name, k)


@pytest.mark.parametrize("name", cases.NAMES)
def test_no_drawn_input_sits_on_a_kink(name):
    c = cases.case(name)
    assert min(cases.margins(c)) >= cases.MARGIN
    for k in ro.INPUTS:                                      # fp32-representable, as the GPU sees them
        assert c[k].dtype == np.float32


def test_the_flat_patch_hits_the_conventions_it_is_there_for():
    c = cases.case("flat_patch")
    x = {k: torch.tensor(c[k][0].astype(np.float64)) for k in ro.INPUTS}
    a = ro.neighbour_differences(x["image"].mean(dim=-1, keepdim=True))[..., 0]
    b = ro.neighbour_differences(x["depth"][..., None])[..., 0]
    assert int(((a == 0) & (b == 0)).sum()) >= 8 * 4            # sign(0) = 0 inside the 4 x 4 block
    az = x["pos"][..., 2].abs()
    assert int((az == c["z_min"]).sum()) == 3 and int((az == c["z_max"]).sum()) == 3
    assert int(((az > c["z_min"]) & (az < c["z_max"])).sum()) >= 5
    # without the flat mask the same case fails the condition: the mask is what admits the exact zeros
    assert min(ro.decision_margin(*(x[k] for k in ro.INPUTS), c["z_min"], c["z_max"]) for _ in (0,)) == 0.0


def test_the_end_to_end_case_is_clear_of_kinks():
    """The rendered views of tests/test_hip_regularizers.py's end-to-end case: the GPU feeds fp32-rounded renderer
    outputs to the regularisers, so every decision quantity of the fp64 composition stays 1e-5 clear of zero -- except
    u_k . n, which is zero BY CONSTRUCTION between the sub-pixels of one splat (they lie on the plane n is normal to):
    that term's gradient does not exist there, and the end-to-end loss weights it 0."""
    import regularizer_e2e as e2e
    for b in range(e2e.B):
        out = e2e.oracle_view(b, requires_grad=False)[0]
        assert ro.decision_margin(out["pos"], out["normal"], out["image"], out["depth"], e2e.Z_MIN, e2e.Z_MAX,
                                  skip=("consistency",)) >= 1e-5
        d = ro.neighbour_differences(out["pos"])
        within = torch.sum(ro._unit(d) * out["normal"], dim=-1).abs().min()
        assert float(within) < 1e-12                          # the kink the docstring speaks of
    assert e2e.WEIGHTS[ro.TERMS.index("normal_consistency")] == 0.0


def test_a_batch_is_its_views():
    c = cases.case("17x9_b3")
    whole, _ = cases.expected("17x9_b3")
    for b in range(3):
        one = ro.terms(*(torch.tensor(c[k][b].astype(np.float64)) for k in ro.INPUTS), c["z_min"], c["z_max"])
        for k in ro.TERMS:
            np.testing.assert_allclose(float(one[k]), whole[k][b], rtol=1e-12)
