"""CPU only: what tests/test_hip_splat_entries.py relies on, pinned with the fp64 oracle alone -- the per-term sums of
splat_oracle.gradient_terms, the add counts of splat_entry_bounds.add_counts against hand-written figures, the distance
of every relu argument from its threshold (so that no comparison on the GPU can decide otherwise than the oracle), and
that each designed case reaches the branch it is named for."""
import numpy as np
import pytest

import splat_entry_bounds as EB
import splat_oracle
from splat_edge_scenes import CASES, build, reference, sub_ray_dot_normal, terms
from test_splat_oracle_cpu import CASES as FIXTURES, _load

NEW = ("materials_by_wave", "materials_mixed_tail", "zero_attenuation", "steep_given_k2")


def _fixture(name):
    npz, scene, kw = _load(name)
    return scene, kw, {k: npz["grad_in/" + k] for k in splat_oracle.OUTPUTS}


# ---- the oracle's per-term sums ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_term_totals_equal_the_gradients(name):
    scene, kw, notes, up, out, grads = reference(name)
    total, absolute = terms(name)
    assert set(total) == set(absolute) == set(grads)
    for k, g in grads.items():
        assert total[k].shape == absolute[k].shape == g.shape, k
        np.testing.assert_allclose(total[k], g, rtol=1e-10, atol=1e-10 * np.nanmax(np.abs(g)), err_msg=k)   # NaN == NaN
        fin = np.isfinite(total[k])
        assert np.all(absolute[k][fin] >= np.abs(total[k][fin]) * (1 - 1e-12)), k
        assert np.isfinite(absolute[k]).all() and np.all(absolute[k] >= 0), k


def test_term_totals_of_a_geometry_only_fixture_leave_the_shading_leaves_at_zero():
    scene, kw, up = _fixture("p1_norm_depth_36x48")
    assert kw == {"norm_depth_image_only": True}
    total, absolute = splat_oracle.gradient_terms(scene, up, **kw)
    want = splat_oracle.gradients(scene, up, **kw)[1]
    for k in want:
        np.testing.assert_allclose(total[k], want[k], rtol=1e-10, atol=1e-10 * max(np.abs(want[k]).max(), 1e-300))
        assert (k == "disk.pos") == bool(absolute[k].any()), k


def test_terms_are_grouped_as_the_kernel_adds_them():
    """lights_5: lights 1 and 3 share colour row 1, lights 0 and 4 row 2 -- a row's absolute is the sum over its lights
    of each light's own sum, above |total| where the lights' terms differ in sign; light_vis: K^2 terms per entry."""
    scene, kw, notes, up, out, grads = reference("lights_5")
    total, absolute = terms("lights_5")
    assert np.array_equal(splat_oracle.clamped_color_idx(scene), [2, 1, 3, 1, 2])
    assert not absolute["colors"][0].any() and absolute["colors"][1:].all()
    raw = {}
    splat_oracle.gradient_terms(scene, up, _raw=raw, **kw)
    assert raw["colors"].shape == (6, 6, 5, 3) and raw["lights.pos"].shape == (6, 6, 5, 4)
    assert raw["materials.albedo"].shape == (6, 6, 3) and raw["lights.ambient"].shape == (6, 6, 3)
    np.testing.assert_allclose(absolute["colors"][1], np.abs(raw["colors"][:, :, [1, 3]]).sum(axis=(0, 1, 2)), rtol=1e-12)
    scene, kw, notes, up, out, grads = reference("k4_given")
    t = splat_oracle.light_vis_terms(scene, up, **kw)
    assert t.shape == (2, 35, 16)
    np.testing.assert_allclose(t.sum(-1), grads["disk.light_vis"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(np.abs(t).sum(-1), terms("k4_given")[1]["disk.light_vis"], rtol=1e-12)
    # sub = c K + r is the sub-pixel at output (i K + c, j K + r): splat 9 = (1, 2), sub 6 = (c 1, r 2) -> output (5, 10)
    only = {"image": np.zeros_like(up["image"])}
    only["image"][5, 10] = up["image"][5, 10]
    t1 = splat_oracle.light_vis_terms(scene, only, **kw)
    assert np.array_equal(np.argwhere(t1.any(axis=0)), [[9, 6]])


# ---- the add counts ------------------------------------------------------------------------------------------------------
HAND = {   # lights.pos / lights.attenuation per light, colors per row, ambient, materials per row
    # N = 4, one wave holding materials (1, 3): mixed, one atomicAdd per lane
    "grid_2x2": (1, [0, 1, 1], 1, [1, 3]),
    # N = 65: wave 0 holds (38, 26), mixed; wave 1 is one live lane of material 1, uniform
    "wave_5x13": (2, [0, 2, 2], 2, [38, 26 + 1]),
    # N = 257: four mixed waves (36, 28), (40, 24), (31, 33), (35, 29); the fifth is one live lane of material 0
    "block_1x257": (5, [0, 5, 5], 5, [36 + 40 + 31 + 35 + 1, 28 + 24 + 33 + 29]),
    # N = 36, color_idx (2, 1, 3, 1, 2): rows 1 and 2 take two lights each, row 3 one
    "lights_5": (1, [0, 2, 2, 1], 1, [19, 17]),
    # two uniform waves, one row each; row 2 unused
    "materials_by_wave": (2, [0, 2, 2], 2, [1, 1, 0]),
    # N = 70, K = 2: 2 waves x 4 sub-pixels, color_idx (1, 2, 1); wave 1's six live lanes are uniform
    "materials_mixed_tail": (8, [0, 16, 8], 2, [1, 1, 0]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_add_counts_equal_hand_written_figures(name):
    scene, kw, notes = build(name)
    per_light, colors, ambient, materials = HAND[name]
    c = EB.add_counts(scene, kw)
    L = len(scene["lights"]["pos"])
    assert c["lights.pos"].tolist() == c["lights.attenuation"].tolist() == [[per_light]] * L
    assert c["colors"].reshape(-1).tolist() == colors and c["lights.ambient"].tolist() == [ambient]
    assert c["materials.albedo"].reshape(-1).tolist() == c["materials.coeffs"].reshape(-1).tolist() == materials
    for k, v in EB.add_counts(scene, kw, views=3).items():
        assert np.array_equal(v, 3 * c[k]), k
    for k, v in c.items():                                   # broadcastable to the leaf, and 0 exactly where no term lands
        a = terms(name)[1][k]
        assert np.broadcast_to(v, a.shape).shape == a.shape
        assert np.array_equal(np.broadcast_to(v, a.shape)[..., 0] > 0, a.any(axis=-1)) or k == "lights.ambient", k


def test_bounds_follow_their_formulas():
    a = np.array([0.0, 1.0, 3.0])
    bound, acc = EB.atomic_bound(a, np.array([0.0, 5.0, 64.0]))
    np.testing.assert_allclose(bound, np.array([0.0, 12.0, 3 * 71.0]) * 2.0 ** -24 * (1 + 2.0 ** -20), rtol=1e-15)
    assert np.array_equal(bound, acc)
    np.testing.assert_allclose(EB.written_bound(np.array([-2.0]), np.array([4.0]), 2.0 ** -40),
                               (2.0 ** -23 + 2.0 ** -38) * (1 + 2.0 ** -20), rtol=1e-15)
    np.testing.assert_allclose(EB.light_vis_bound(np.array([1.0]), np.array([2.0]), 8), 128 * 2.0 ** -24 * (1 + 2.0 ** -20))
    assert np.array_equal(EB.light_vis_bound(np.array([1.0]), np.array([2.0]), 1, 0.0), EB.written_bound([1.0], [2.0], 0.0))
    np.testing.assert_allclose(EB.shared_written_bound([np.array([1.0]), np.array([-2.0]), np.array([3.0])], [0.5, 0.25, 0.25]),
                               1.0 + 2 * 2.0 ** -24 * 6.0 * (1 + 2.0 ** -20), rtol=1e-15)
    assert EB.written_excess(np.array([1.0 + 2.0 ** -23]), np.array([1.0]), np.array([2.0])) == 2.0 ** -25
    assert EB.C64 == EB.C64_FACTOR * EB.C64_MEASURED and EB.C64 <= EB.C64_CAP == 2.0 ** -36


# ---- every relu away from its threshold ----------------------------------------------------------------------------------
def _z(scene):
    pos = np.asarray(scene["objects"]["disk"]["pos"])
    return pos if pos.ndim == 1 else pos[:, 2]


@pytest.mark.parametrize("name", tuple(CASES) + tuple(FIXTURES))
def test_no_relu_argument_is_near_its_threshold(name):
    if name in CASES:
        scene, kw, _ = build(name)
    else:
        scene, kw, _ = _fixture(name)
    margins = splat_oracle.decision_margin(scene, **kw)
    assert set(margins) == ({"-z"} if kw.get("norm_depth_image_only") else {"-z", "afac * ldn", "reflection", "light sum"})
    z = _z(scene)
    at_zero, clamped = np.where(z == 0)[0], np.where(z >= 0)[0]
    assert (clamped.size > 0) == (name.startswith("clamped_") or name.startswith("p1_zpos_flat")), name
    for relu, (margin, zeros) in margins.items():
        print(f"{name} {relu}: margin {margin:.3g}, {len(zeros)} exact zeros")
        assert margin >= 1e-9, (name, relu)
        # exact zeros only at the clamped splats, listed by index: -z at z == 0; the reflection dot at every clamped
        # splat (its point is the origin, so the view direction -unit(pos) is 0)
        allowed = {"-z": at_zero, "reflection": clamped}.get(relu, np.zeros(0, dtype=np.int64))
        assert np.array_equal(zeros, allowed), (name, relu, zeros)


# ---- each new case reaches its branch ------------------------------------------------------------------------------------
def test_materials_by_wave_has_uniform_waves_that_differ():
    scene, kw, notes = build("materials_by_wave")
    m = np.asarray(scene["objects"]["disk"]["material_idx"])
    assert m.size == 128 and np.all(m[:64] == 0) and np.all(m[64:] == 1) and len(scene["materials"]["albedo"]) == 3
    total, absolute = terms("materials_by_wave")
    for k in ("materials.albedo", "materials.coeffs"):
        assert np.all(total[k][:2] != 0) and not total[k][2].any() and not absolute[k][2].any(), k


def test_materials_mixed_tail_puts_material_one_in_the_live_lanes_of_the_last_wave_only():
    scene, kw, notes = build("materials_mixed_tail")
    m = np.asarray(scene["objects"]["disk"]["material_idx"])
    assert m.size == 70 and m[0] == 0 and np.array_equal(np.where(m == 1)[0], np.arange(64, 70)) and kw == {"samples": 2}
    total, absolute = terms("materials_mixed_tail")
    assert np.all(total["materials.albedo"][:2] != 0) and np.all(total["materials.coeffs"][:2] != 0)
    # material 1's six splats against material 0's 64: were the dead lanes' pixel 0 (material 0) to count, or the wave's
    # sum to land on row 0, row 1 would change by a multiple of itself
    assert not total["materials.albedo"][2].any()


def test_zero_attenuation_takes_the_den_ok_false_branch():
    scene, kw, notes = build("zero_attenuation")
    att = np.asarray(scene["lights"]["attenuation"])
    assert att.shape == (3, 3) and not att[1].any() and att[0].any() and att[2].any()
    probe = {}
    splat_oracle.render(scene, splat_oracle.make_leaves(scene, requires_grad=False), _probe=probe, **kw)
    assert np.all(probe["den"][1].numpy() == 0) and np.all(probe["den"][0].numpy() != 0) and np.all(probe["den"][2].numpy() != 0)
    total, absolute = terms("zero_attenuation")
    assert not total["lights.attenuation"][1].any() and not absolute["lights.attenuation"][1].any()
    assert np.all(total["lights.attenuation"][[0, 2]] != 0)
    assert np.all(total["lights.pos"][1, :3] != 0)           # afac = 1: the light still shades


def test_steep_given_k2_lets_the_ray_term_dominate_the_normal_gradient():
    scene, kw, notes = build("steep_given_k2")
    rn = sub_ray_dot_normal(scene, kw)
    assert rn.shape == (10, 14) and np.all(rn < 0)
    assert 0.08 <= -rn.max() <= 0.2, rn.max()                 # about -0.1 at the left edge
    assert -rn.min() > 0.9
    total, absolute = terms("steep_given_k2")
    g = np.abs(total["disk.normal"]).reshape(5, 7, 3).max(axis=-1)
    assert g[:, 0].min() > 2 * g[:, -1].max() and g[:, 0].mean() > 5 * g[:, -1].mean()      # 1 / rn^2 on the left
