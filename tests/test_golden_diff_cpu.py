"""oracle.golden_io.diff_npz, the comparison behind ``python -m oracle.gen_golden --check``: it must report a missing key,
a dtype, shape, value or ``meta`` change by key, treat NaN as equal to NaN, and find a committed fixture equal to itself.
No reference needed."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from oracle.golden_io import diff_npz


def _npz(path, **arrays):
    np.savez_compressed(path, **arrays)
    return np.load(path, allow_pickle=False)


def _base():
    return {"out/image": np.arange(24, dtype=np.float32).reshape(2, 4, 3), "out/depth": np.linspace(0, 1, 8).reshape(2, 4),
            "out/nearest": np.arange(8, dtype=np.int64).reshape(2, 4), "grad/colors": np.ones((3, 3), np.float32),
            "meta": np.asarray('{"has_tonemap": true}')}


def test_reports_each_difference_by_key(tmp_path):
    other = _base()
    del other["grad/colors"]                                              # a missing key
    other["out/image"] = other["out/image"].astype(np.float64)            # a dtype change, values equal
    other["out/depth"] = other["out/depth"].reshape(4, 2)                 # a shape change
    other["out/nearest"] = other["out/nearest"].copy()
    other["out/nearest"][1, 2] += 1                                       # one flipped element
    other["meta"] = np.asarray('{"has_tonemap": true, "proj_type": "perspective"}')
    a, b = _npz(tmp_path / "a.npz", **_base()), _npz(tmp_path / "b.npz", **other)
    got = dict(diff_npz(a, b))
    assert sorted(got) == ["grad/colors", "meta", "out/depth", "out/image", "out/nearest"]
    assert "only in the first" in got["grad/colors"]
    assert "float32" in got["out/image"] and "float64" in got["out/image"]
    assert "(2, 4)" in got["out/depth"] and "(4, 2)" in got["out/depth"]
    assert got["out/nearest"].startswith("1 of 8 values differ") and "(1, 2)" in got["out/nearest"]
    assert "proj_type" in got["meta"]
    assert dict(diff_npz(b, a))["grad/colors"] == "only in the second"


def test_nan_equals_nan(tmp_path):
    arrays = _base()
    arrays["out/depth"][0, 1] = arrays["out/image"][1, 3, 2] = np.nan
    a, b = _npz(tmp_path / "a.npz", **arrays), _npz(tmp_path / "b.npz", **arrays)
    assert diff_npz(a, b) == []
    arrays["out/depth"][1, 0] = np.nan                                    # ... but NaN is not equal to a number
    assert [k for k, _ in diff_npz(a, _npz(tmp_path / "c.npz", **arrays))] == ["out/depth"]


@pytest.mark.parametrize("name", ["g1_demo_64x48", "n1_aux_grad_phong", "p1_estimated_36x48"])
def test_committed_fixture_equals_itself(name):
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    assert diff_npz(np.load(path, allow_pickle=False), np.load(path, allow_pickle=False)) == []
