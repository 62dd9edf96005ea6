"""radiance_SH9_batched and irradiance_batched on the GPU against the fp64 restatement (tests/sh9_oracle.py) and the
reference's recorded values (tests/golden/sh_lighting): every output element and every gradient entry within
2^-24 |ref| + 2^-40 A (tests/sh9_checks.py derives it); the reduction shapes whose finish rows wrap; every combination of
leaves; the chain from L; determinism, batch = views, and the order a shared M's gradient is added in.  Run with -s for
the worst measured ratios."""
import functools
import os

import numpy as np
import pytest
import torch

import sh9_cases as cases
import sh9_oracle as oracle
from conftest import GOLDEN_DIR
from sh9_checks import (DEV, check, check_irradiance, check_projection, irradiance_truth, irradiance_truth_of, leaf,
                        projection_truth, projection_truth_of, run_irradiance, run_projection)

pytestmark = pytest.mark.gpu
P_ALL, I_ALL = range(len(cases.PROJECTION)), range(len(cases.IRRADIANCE))


@functools.lru_cache(maxsize=None)
def fixture(tag):
    return dict(np.load(os.path.join(GOLDEN_DIR, "sh_lighting", "sh1_" + tag + ".npz")))


@pytest.mark.parametrize("k", P_ALL, ids=cases.projection_tag)
def test_a_batch_of_probes_has_the_oracles_and_the_references_coefficients_and_the_oracles_gradient(k):
    c, T, z = cases.projection(k), projection_truth(k), fixture(cases.projection_tag(k))
    H, W, C, B = cases.PROJECTION[k]
    got = run_projection(c["envmap"], c["g_L"])
    assert got["L"].shape == (B, C, 9) and got["grad_envmap"].shape == (B, H, W, C)
    worst = check_projection(got, T)
    for b in range(B):                                                     # the reference's own values, the same bound
        worst = max(worst, check(got["L"][b], z["ref/L"][b], T[b]["A_L"], f"reference L, view {b}"))
    if (H, W) == (1, 1):
        assert (got["L"] == 0).all() and (got["grad_envmap"] == 0).all()
    print(f"{cases.projection_tag(k)}: {worst:.3g} of the bound")


@pytest.mark.parametrize("k", I_ALL, ids=cases.irradiance_tag)
def test_a_batch_of_normals_has_the_oracles_and_the_references_irradiance_and_the_oracles_gradients(k):
    c, T, z = cases.irradiance(k), irradiance_truth(k), fixture(cases.irradiance_tag(k))
    N, C, _, per_view = cases.IRRADIANCE[k]
    got = run_irradiance(c["M"], c["normal"], c["g_E"])
    assert got["E"].shape == (cases.VIEWS, N, C) and got["grad_normal"].shape == (cases.VIEWS, N, 3)
    assert got["grad_M"].shape == c["M"].shape
    worst = check_irradiance(got, c, T)
    for b in range(cases.VIEWS):
        worst = max(worst, check(got["E"][b], z["ref/E"][b], T[0][b]["A_E"], f"reference E, view {b}"))
    assert np.array_equal(got["E"][-1, -1], cases.view_M(c, cases.VIEWS - 1)[3, 3])          # the zero normal: M[3, 3]
    print(f"{cases.irradiance_tag(k)}: {worst:.3g} of the bound")


def test_a_probe_of_73_workgroups_per_view_wraps_the_finish_rows():
    c = cases.make_projection(cases.ORACLE_ONLY, 4199)
    got = run_projection(c["envmap"], c["g_L"])
    print(f"136 x 136: {check_projection(got, projection_truth_of(c['envmap'], c['g_L'])):.3g} of the bound")


@pytest.mark.parametrize("per_view", [True, False], ids=["views", "shared"])
def test_normals_of_67_workgroups_per_view_wrap_the_finish_rows(per_view):
    c = cases.make_irradiance(cases.ORACLE_ONLY_N[:3] + (per_view,), 5299)
    got = run_irradiance(c["M"], c["normal"], c["g_E"])
    print(f"N = 16900: {check_irradiance(got, c, irradiance_truth_of(c)):.3g} of the bound")


@pytest.mark.parametrize("k", [3, 4], ids=cases.irradiance_tag)                  # an M per view, and a shared one
def test_every_combination_of_leaves_gives_the_oracles_gradients(k):
    c, T = cases.irradiance(k), irradiance_truth(k)
    both = run_irradiance(c["M"], c["normal"], c["g_E"])
    for leaves in (("M",), ("normal",)):
        got = run_irradiance(c["M"], c["normal"], c["g_E"], leaves)
        check_irradiance(got, c, T, "+".join(leaves))
        for key in ("grad_M", "grad_normal"):                                    # the other leaf does not change the bits
            assert (got[key] is None) == (key[5:] not in leaves)
            assert got[key] is None or np.array_equal(got[key], both[key]), key
    none = run_irradiance(c["M"], c["normal"], c["g_E"], ())
    assert none["grad_M"] is None and none["grad_normal"] is None and np.array_equal(none["E"], both["E"])


def test_an_m_that_needs_no_gradient_runs_the_backward_without_workspace_or_reduction(monkeypatch):
    from surf_renderer_amd import _lib
    c = cases.irradiance(3)
    lib = _lib.load()
    seen = []
    real = lib.srh_sh9_irradiance_bwd
    monkeypatch.setattr(lib, "srh_sh9_irradiance_bwd", lambda *a: seen.append(a) or real(*a))
    run_irradiance(c["M"], c["normal"], c["g_E"], ("normal",))
    run_irradiance(c["M"], c["normal"], c["g_E"], ("M",))
    (_, _, _, _, grad_n, grad_M, ws, ws_bytes, _), second = seen
    assert grad_n and grad_M is None and ws is None and ws_bytes == 0
    assert second[4] is None and second[5] and second[6] and second[7] > 0


def test_a_zero_and_a_missing_upstream_gradient_give_exact_zeros():
    from surf_renderer_amd import irradiance_batched, radiance_SH9_batched, sh_lighting
    c, p = cases.irradiance(3), cases.projection(0)
    tM, tn, env = leaf(c["M"]), leaf(c["normal"]), leaf(p["envmap"])
    E, L = irradiance_batched(tM, tn), radiance_SH9_batched(env)

    def node(t):                                                           # the layer's own node behind the reshapes
        fn = t.grad_fn
        while not hasattr(fn, "params"):
            fn = fn.next_functions[0][0]
        return fn

    # None is what autograd hands a function whose output took no part in the loss: zeros, and no launch
    _, g_M, g_n = sh_lighting._IrradianceFunction.backward(node(E), None)
    assert g_M.shape == tM.shape and g_n.shape == tn.shape and (g_M == 0).all() and (g_n == 0).all()
    assert g_M.dtype == torch.float32 and g_M.device == tM.device
    _, g_env = sh_lighting._ProjectFunction.backward(node(L), None)
    assert g_env.shape == env.shape and (g_env == 0).all()
    (E * 0.0).sum().backward()
    (L * 0.0).sum().backward()
    for t in (tM, tn, env):
        assert t.grad.shape == t.shape and (t.grad == 0).all()


@pytest.mark.parametrize("k", [5, 2], ids=cases.irradiance_tag)                  # zonal: an L per view, and a shared one
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_the_chain_from_l_through_the_zonal_matrix_has_the_oracles_gradient(k, dtype):
    from surf_renderer_amd import RealSH9_ZonalMatrix, irradiance_batched
    c = cases.irradiance(k)
    L, tn = leaf(c["L"], dtype=dtype), leaf(c["normal"])
    M = RealSH9_ZonalMatrix(L)
    assert M.dtype == torch.float64 and M.device == L.device and M.shape == c["M"].shape
    assert np.array_equal(M.detach().float().cpu().numpy(), c["M"])             # the case's M, before its one rounding
    E = irradiance_batched(M, tn)
    (E * torch.tensor(np.array(c["g_E"]), device=DEV)).sum().backward()
    assert L.grad.dtype == dtype and L.grad.shape == L.shape
    views = [oracle.chain_view(c["L"] if c["L"].ndim == 2 else c["L"][b], c["normal"][b], c["g_E"][b])
             for b in range(cases.VIEWS)]
    got_L = L.grad.cpu().numpy()
    for b, t in enumerate(views):
        check(E[b].detach().cpu().numpy(), t["E"], t["A_E"], f"E, view {b}")
        check(tn.grad[b].cpu().numpy(), t["grad_normal"], t["A_normal"], f"grad_normal, view {b}")
        if c["L"].ndim == 3:
            check(got_L[b].astype(np.float32), t["grad_L"], t["A_L"], f"grad_L, view {b}")
    if c["L"].ndim == 2:
        check(got_L.astype(np.float32), sum(t["grad_L"] for t in views), sum(t["A_L"] for t in views), "shared grad_L")
    if dtype == torch.float64:                                                   # nothing rounded it to float32 on the way
        assert (got_L != got_L.astype(np.float32)).any()


def test_the_chain_from_the_probe_to_the_irradiance_is_differentiable_end_to_end():
    from surf_renderer_amd import RealSH9_ZonalMatrix, irradiance_batched, radiance_SH9_batched
    p, c = cases.projection(0), cases.irradiance(7)
    env, tn = leaf(p["envmap"]), leaf(c["normal"][:2])
    L = radiance_SH9_batched(env)
    E = irradiance_batched(RealSH9_ZonalMatrix(L), tn)
    g_E = c["g_E"][:2]
    (E * torch.tensor(np.array(g_E), device=DEV)).sum().backward()
    # the oracle's chain on the float32 L the projection stored, then the projection's gradient under that g_L
    for b in range(2):
        t = oracle.chain_view(L[b].detach().cpu().numpy(), c["normal"][b], g_E[b])
        check(E[b].detach().cpu().numpy(), t["E"], t["A_E"], f"E, view {b}")
        g_L32 = t["grad_L"].astype(np.float32)                                   # L is float32: its gradient is rounded once
        grad, A = oracle.project_grad(p["envmap"][b].shape, g_L32)
        got = env.grad[b].cpu().numpy()
        # g_L itself carries 2^-24 |g_L| + 2^-40 A_L, which the projection's backward multiplies by |Y| domega
        slack = oracle.project_grad(p["envmap"][b].shape, 2.0 ** -24 * np.abs(t["grad_L"]) + 2.0 ** -40 * t["A_L"])[1]
        err = np.abs(got.astype(np.float64) - grad)
        assert (err <= 2.0 ** -24 * np.abs(grad) + 2.0 ** -40 * A + slack).all(), b
        assert (got[A == 0] == 0).all() and np.abs(got).max() > 0


@pytest.mark.parametrize("k", [0, 3, 4], ids=cases.projection_tag)
def test_projection_runs_are_bit_identical_and_a_batch_equals_its_views(k):
    c = cases.projection(k)
    a, again = run_projection(c["envmap"], c["g_L"]), run_projection(c["envmap"], c["g_L"])
    for key in a:
        assert np.array_equal(a[key], again[key]), key
    for b in range(len(c["envmap"])):
        b1 = run_projection(c["envmap"][b:b + 1], c["g_L"][b:b + 1])
        one = run_projection(c["envmap"][b], c["g_L"][b], batched=False)
        for key in a:
            assert one[key].shape == a[key].shape[1:], key
            assert np.array_equal(b1[key][0], a[key][b]) and np.array_equal(one[key], a[key][b]), (key, b)


@pytest.mark.parametrize("k", [3, 5, 6], ids=cases.irradiance_tag)               # an M per view
def test_irradiance_runs_are_bit_identical_and_a_batch_equals_its_views(k):
    c = cases.irradiance(k)
    a, again = run_irradiance(c["M"], c["normal"], c["g_E"]), run_irradiance(c["M"], c["normal"], c["g_E"])
    for key in a:
        assert np.array_equal(a[key], again[key]), key
    for b in range(cases.VIEWS):
        b1 = run_irradiance(c["M"][b:b + 1], c["normal"][b:b + 1], c["g_E"][b:b + 1])
        shared = run_irradiance(c["M"][b], c["normal"][b:b + 1], c["g_E"][b:b + 1])         # one view: shared = its own
        for key in a:
            assert np.array_equal(b1[key][0], a[key][b]), (key, b)
        assert np.array_equal(shared["E"][0], a["E"][b]) and np.array_equal(shared["grad_normal"][0], a["grad_normal"][b])
        assert np.array_equal(shared["grad_M"], a["grad_M"][b])


def test_a_shared_ms_gradient_is_the_views_gradients_added_in_ascending_view_order():
    # exactly representable sums: a shared M over three views = the three per-view gradients added
    c = cases.irradiance(3)
    n = np.round(c["normal"] * 4) / 4
    g = np.round(c["g_E"] * 8) / 8
    per_view = run_irradiance(np.stack([c["M"][0]] * 3), n, g)
    shared, again = run_irradiance(c["M"][0], n, g), run_irradiance(c["M"][0], n, g)
    total = per_view["grad_M"][0].astype(np.float64) + per_view["grad_M"][1] + per_view["grad_M"][2]
    assert np.array_equal(shared["grad_M"].astype(np.float64), total) and np.array_equal(shared["grad_M"], again["grad_M"])
    assert np.array_equal(shared["E"], per_view["E"]) and np.array_equal(shared["grad_normal"], per_view["grad_normal"])
    # and the order: four views of one zero normal, so that grad_M[3, 3] = the sum of the upstream gradients.  In fp64
    # ((2^53 + 1) + 1) - 2^53 is 0 added in ascending order, 2 in descending order and 1 added pairwise
    ups = np.array([2.0 ** 53, 1.0, 1.0, -2.0 ** 53], np.float32).reshape(4, 1, 1)
    got = run_irradiance(np.ones((4, 4, 1), np.float32), np.zeros((4, 1, 3), np.float32), ups)
    assert got["grad_M"][3, 3, 0] == 0.0 and (got["grad_M"][:3] == 0).all() and (got["grad_M"][3, :3] == 0).all()
    assert np.array_equal(got["E"], np.ones((4, 1, 1), np.float32))
