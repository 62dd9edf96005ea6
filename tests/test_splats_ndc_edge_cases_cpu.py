"""Each case of tests/splats_ndc_edge_cases.py reaches the branch it is named for, shown with the fp64 restatement
(tests/splats_ndc_oracle.py) alone; and the restatement against the reference's own render_splats_NDC on these cases
(tests/golden/splats_ndc/sn2_*.npz, tools/gen_splats_ndc_golden.py) at the bar of tests/test_splats_ndc_oracle_cpu.py:
rtol 1e-9, atol 1e-12 max|want|.  sign(0), relu'(0) and pow at base 0 are exactly where a restatement can drift from the
function it restates.  Runs without a GPU."""
import os

import numpy as np
import pytest

import splats_ndc_cases as cases
import splats_ndc_edge_cases as edges
import splats_ndc_oracle as oracle
from conftest import GOLDEN_DIR

DIR = os.path.join(GOLDEN_DIR, "splats_ndc")
WAVE = 64


def _waves(mat):
    return [mat[i:i + WAVE] for i in range(0, len(mat), WAVE)]


@pytest.mark.parametrize("name", edges.NAMES)
def test_every_splat_that_is_not_at_a_kink_keeps_the_margins(name):
    c = edges.case(name)
    m = edges.margins(c)
    assert set(m) == {"diffuse", "specular", "light sum"} | ({"cam_dir . n"} if c["kwargs"].get("double_sided") else set())
    assert all(v[0] >= cases.MARGIN for v in m.values()), (name, m)
    assert (len(c["at_kink"]) == 2) == name.startswith("zero_normals")


def test_uniform_waves_holds_two_uniform_waves_of_either_material_and_a_mixed_one():
    c = edges.case("uniform_waves")
    assert oracle.grid(c["scene"]["camera"]) == (16, 12) and oracle.n_views(c["scene"]) == 0
    w = _waves(np.asarray(c["scene"]["objects"]["disk"]["material_idx"]))
    assert len(w) == 3 and all(len(x) == WAVE for x in w)
    assert np.all(w[0] == 1) and np.all(w[1] == 0) and set(w[2]) == {0, 1}


@pytest.mark.parametrize("name,B", [("uniform_partial", 0), ("uniform_b3", 3)])
def test_uniform_partial_has_dead_lanes_that_read_another_material(name, B):
    c = edges.case(name)
    assert oracle.grid(c["scene"]["camera"]) == (16, 5) and oracle.n_views(c["scene"]) == B
    mat = np.asarray(c["scene"]["objects"]["disk"]["material_idx"])
    w = _waves(mat)
    assert len(w) == 2 and np.all(w[0] == 1) and len(w[1]) == 16 and np.all(w[1] == 0)
    assert mat[0] == 1                                                 # what a dead lane (pix = 0) of wave 1 reads
    if B:
        disk, sc = c["scene"]["objects"]["disk"], c["scene"]
        assert disk["pos"].shape == (3, 80, 3) and disk["normal"].shape == (3, 80, 3)
        assert sc["camera"]["eye"].shape == (3, 4) and sc["lights"]["pos"].shape == (3, 2, 4)


@pytest.mark.parametrize("name", ["uniform_waves", "uniform_partial", "uniform_b3"])
def test_each_uniform_wave_moves_its_material_s_gradient_far_beyond_the_tolerance(name):
    """The gradient the uniform wave of material 1 (m0 != 0) sends to its row, alone, is far above the atomic tolerance
    of the GPU comparison (2e-4 max|want| + 1e-6): were it added to row 0, or lost, the comparison would fail.  The
    tolerance follows the array's largest entry, which material 1's exponent 12 on an unnormalised view direction sets;
    the wave of material 0 is only shown to reach its own row and no other."""
    c = edges.case(name)
    _, full = edges.expected(name)
    mat = np.asarray(c["scene"]["objects"]["disk"]["material_idx"])
    for lanes, m in ((slice(0, WAVE), 1), (slice(WAVE, 2 * WAVE), 0)):
        keep = np.zeros(len(mat), bool)
        keep[lanes] = True
        ups = {}
        for k, v in c["upstream"].items():                             # the upstream gradient of this wave's splats alone
            tail = () if k == "depth" else (3,)
            lead = v.shape[:v.ndim - 2 - len(tail)]
            flat = np.array(v, copy=True).reshape(lead + (len(mat),) + tail)
            flat[(slice(None),) * len(lead) + (~keep,)] = 0
            ups[k] = flat.reshape(v.shape)
        _, part = oracle.batch_gradients(c["scene"], ups, **c["kwargs"])
        assert np.all(mat[lanes] == m)
        for leaf in ("materials.albedo", "materials.coeffs"):
            tol = 2e-4 * np.abs(full[leaf]).max() + 1e-6
            assert np.all(part[leaf][1 - m] == 0), (name, leaf)
            assert np.abs(part[leaf][m]).max() > (100 * tol if m == 1 else 0), (name, leaf, part[leaf][m], tol)


@pytest.mark.parametrize("name", [n for n in edges.NAMES if n.startswith("zero_normals")])
def test_zero_normals_put_the_dots_on_their_kinks_exactly(name):
    c = edges.case(name)
    sc, kw, at = c["scene"], c["kwargs"], list(c["at_kink"])
    disk = sc["objects"]["disk"]
    assert oracle.grid(sc["camera"]) == (3, 5)
    assert np.all(disk["normal"][at] == 0) and np.all(np.abs(disk["normal"]).sum(-1)[np.setdiff1d(np.arange(15), at)] > 0)
    mat = np.asarray(disk["material_idx"])
    assert sorted(mat[at]) == [0, 1]
    d = oracle.decisions(sc, **dict(kw, double_sided=True))
    assert np.all(d["cam_dir . n"][at] == 0) and np.all(d["diffuse"][at] == 0) and np.all(d["specular"][at] == 0)
    d = oracle.decisions(sc, **kw)
    assert np.all(d["diffuse"][at] == 0)
    if kw.get("double_sided"):
        assert np.all(d["specular"][at] == 0)
    else:                                                              # the view direction alone: clear of the kink
        assert np.abs(d["specular"][at]).min() >= cases.MARGIN
    assert np.abs(d["light sum"][at]).min() >= cases.MARGIN            # the last relu is not at its kink
    coeffs = np.asarray(sc["materials"]["coeffs"])
    if "_l1" in name:                                                  # a zero-normal splat with exponent 0: 0 ** 0 = 1
        assert sc["lights"]["pos"].shape == (1, 4) and coeffs[0, 2] == 0 and coeffs[0, 1] > 0
        if kw.get("double_sided"):
            s = at[int(np.flatnonzero(mat[at] == 0)[0])]
            amb, alb = np.asarray(sc["lights"]["ambient"], np.float64), np.asarray(sc["materials"]["albedo"], np.float64)[0]
            col = np.asarray(sc["colors"], np.float64)[np.asarray(sc["lights"]["color_idx"])[0]]
            np.testing.assert_allclose(d["light sum"][s], coeffs[0, 1] * 1.0 * col * alb + amb * alb, rtol=1e-14)
    else:
        assert sc["lights"]["pos"].shape == (2, 4) and list(coeffs[:, 2]) == [5.0, 12.0]
    outs, grads = edges.expected(name)
    assert all(np.all(np.isfinite(v)) for v in outs.values()) and all(np.all(np.isfinite(v)) for v in grads.values())
    # cam_dir . n and light . n both vanish, and the specular dot is of second order in n: the shading sends a zero normal
    # exactly nothing, on either side setting, so what it gets is the `normal` output's own upstream gradient
    up_n = c["upstream"]["normal"].reshape(-1, 3).astype(np.float64)[at]
    assert np.array_equal(grads["disk.normal"][at], up_n) and np.abs(up_n).min() > 0


@pytest.mark.parametrize("name", edges.RECORDED)
def test_the_restatement_matches_the_float64_reference(name):
    npz = np.load(os.path.join(DIR, f"sn2_{name}.npz"), allow_pickle=False)
    c = edges.case(name)
    assert oracle.kwargs_of(npz) == c["kwargs"]
    for k, v in oracle.pack(c["scene"]).items():                       # the fixture holds the case
        np.testing.assert_array_equal(npz[k], v, err_msg=f"{name} {k}")
    for k, g in c["upstream"].items():
        np.testing.assert_array_equal(npz["grad_in/" + k], g)
    outs, grads = edges.expected(name)
    for k in oracle.OUTPUTS:
        want = npz["ref64/" + k]
        assert want.dtype == np.float64 and np.all(np.isfinite(want))
        np.testing.assert_allclose(outs[k], want, rtol=1e-9, atol=1e-12 * np.abs(want).max(), err_msg=f"{name} {k}")
    for k in oracle.LEAVES:
        want = npz["grad64/" + k]
        assert np.all(np.isfinite(want))
        np.testing.assert_allclose(grads[k], want, rtol=1e-9, atol=1e-12 * np.abs(want).max(), err_msg=f"{name} d/d {k}")
    largest = max(os.path.getsize(os.path.join(DIR, f)) for f in os.listdir(DIR) if f.startswith("sn1_"))
    assert os.path.getsize(os.path.join(DIR, f"sn2_{name}.npz")) <= largest


def test_every_recorded_case_has_its_fixture_and_no_other():
    have = sorted(f[4:-4] for f in os.listdir(DIR) if f.startswith("sn2_") and f.endswith(".npz"))
    assert have == sorted(edges.RECORDED)


def test_the_abi_scene_is_one_partial_workgroup_with_a_one_lane_wave():
    c = edges.abi_scene()
    assert oracle.grid(c["scene"]["camera"]) == (13, 5)
    mat = np.asarray(c["scene"]["objects"]["disk"]["material_idx"])
    assert len(mat) == 65 and set(mat[:64]) == {0, 1}
    assert all(v[0] >= cases.MARGIN for v in edges.margins(c).values())
