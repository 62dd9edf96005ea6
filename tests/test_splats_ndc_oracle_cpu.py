"""tests/splats_ndc_oracle.py, the fp64 restatement the GPU tests compare with, against the reference's own
render_splats_NDC as recorded in tests/golden/splats_ndc/sn1_*.npz (tools/gen_splats_ndc_golden.py: the reference
unmodified, in float64 under autograd), at the bar tests/test_regularizer_oracle_cpu.py sets: rtol 1e-9, atol
1e-12 max|want|.  And the committed cases still satisfy their kink margins and their coverage.  Runs without a GPU."""
import json
import os

import numpy as np
import pytest

import splats_ndc_cases as cases
import splats_ndc_oracle as oracle
from conftest import GOLDEN_DIR

DIR = os.path.join(GOLDEN_DIR, "splats_ndc")


def load(name):
    npz = np.load(os.path.join(DIR, f"sn1_{name}.npz"), allow_pickle=False)
    return npz, oracle.unpack(npz), oracle.kwargs_of(npz)


def restatement(npz, scene, kw):
    """(outputs, gradients) of the restatement in the fixture's layout: views stacked, shared leaves summed."""
    return oracle.batch_gradients(scene, {k: npz["grad_in/" + k] for k in oracle.OUTPUTS}, **kw)


def test_every_case_has_its_fixture():
    have = sorted(f[4:-4] for f in os.listdir(DIR) if f.startswith("sn1_") and f.endswith(".npz"))
    assert have == sorted(cases.NAMES)
    assert hasattr(oracle, "render") and hasattr(oracle, "gradients")


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_restatement_matches_the_float64_reference(name):
    npz, scene, kw = load(name)
    outs, grads = restatement(npz, scene, kw)
    for k in oracle.OUTPUTS:
        want = npz["ref64/" + k]
        assert want.dtype == np.float64
        np.testing.assert_allclose(outs[k], want, rtol=1e-9, atol=1e-12 * np.abs(want).max(), err_msg=f"{name} {k}")
    for k in oracle.LEAVES:
        want = npz["grad64/" + k]
        np.testing.assert_allclose(grads[k], want, rtol=1e-9, atol=1e-12 * np.abs(want).max(), err_msg=f"{name} d/d {k}")


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_fixture_holds_the_seeded_case(name):
    npz, scene, kw = load(name)
    c = cases.case(name)
    assert kw == c["kwargs"]
    packed = oracle.pack(c["scene"])
    for k, v in packed.items():
        np.testing.assert_array_equal(npz[k], v, err_msg=f"{name} {k}")
    for k, g in c["upstream"].items():
        np.testing.assert_array_equal(npz["grad_in/" + k], g)
        assert g.dtype == np.float32 and np.abs(g).max() < 1.0


def test_the_committed_cases_keep_their_margins_and_cover_every_branch():
    seen = []
    for name in cases.NAMES:
        npz, scene, kw = load(name)
        m = cases.margins(scene, **kw)
        assert all(v[0] >= cases.MARGIN for v in m.values()), (name, m)
        cases.check_special({"name": name, "scene": scene, "kwargs": kw})
        seen.append(m)
    cov = cases.coverage(seen)
    assert set(cov) == set(cases.BRANCHES) and all(cov.values()), cov


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_reference_float32_error_is_a_quarter_of_the_float32_tolerance_at_most(name):
    """What keeps the GPU tests' float32 tolerances (outputs 2e-5 max(max|want|, 1), gradients 3e-3 max(max|want|, 1e-6))
    far above the reference's own float32 rounding on every committed fixture."""
    npz, _, _ = load(name)
    meta = json.loads(str(npz["meta"]))
    for key in npz.files:
        for p32, p64, kind in (("ref32/", "ref64/", "ref/"), ("grad32/", "grad64/", "grad/")):
            if key.startswith(p32):
                a, w = npz[key].astype(np.float64), npz[p64 + key[len(p32):]]
                err = float(np.abs(a - w).max())
                tol = 2e-5 * max(np.abs(w).max(), 1.0) if kind == "ref/" else 3e-3 * max(np.abs(w).max(), 1e-6)
                assert err <= tol / 4, (name, key, err, tol)
                assert meta[kind + key[len(p32):]]["err"] == pytest.approx(err, rel=1e-12, abs=0)
