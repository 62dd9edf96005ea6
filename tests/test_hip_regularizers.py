"""GPU: splat_regularizers (srh_regularizers_fwd / srh_regularizers_bwd) against the fp64 restatement tests/
regularizer_oracle.py on the same fp32 inputs; tests/test_regularizer_oracle_cpu.py ties that to the reference's own
functions (tests/golden/regularizers/r1_*.npz) and asserts that no seeded input sits on a kink, so no element is left
out of any comparison here.

Stated tolerances: the kernels compute the restatement's fp64 arithmetic, sum without atomics and store fp32, so values
match to rtol 2e-6 with atol 2e-7 max(|want|, 1) and gradients to rtol 2e-6 with atol 2e-7 max|want| per input array
(the project's tolerance for fp64 arithmetic with fp32 stores, tests/test_hip_splats.py).  End to end through the
renderer the gradient tolerance is that file's _compare_grads: 2e-4 max|want| + 1e-6."""
import numpy as np
import pytest
import torch

import regularizer_cases as cases
import regularizer_e2e as e2e
import regularizer_oracle as ro

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hip(c, wrt=ro.INPUTS, weights=None):
    """({term: (B,) or ()}, {input: gradient or None}) of a case from the GPU."""
    from surf_renderer_amd import REGULARIZER_TERMS, splat_regularizers
    assert REGULARIZER_TERMS == ro.TERMS
    x = {k: torch.tensor(v, device=DEV, requires_grad=k in wrt) for k, v in cases.inputs(c).items()}
    terms = splat_regularizers(x, c["z_min"], c["z_max"], z_scale=c["z_scale"], unit_normal_scale=c["unit_normal_scale"])
    w = torch.tensor(c["weights"] if weights is None else weights, device=DEV)
    if c["single"]:
        w = w[0]
    sum((w[..., k] * terms[name]).sum() for k, name in enumerate(ro.TERMS)).backward()
    torch.cuda.synchronize()
    return ({k: v.detach().cpu().numpy().astype(np.float64) for k, v in terms.items()},
            {k: (t.grad.cpu().numpy().astype(np.float64) if t.grad is not None else None) for k, t in x.items()})


def _compare_values(got, want, tag, single=False):
    for k in ro.TERMS:
        w = want[k][0] if single else want[k]
        assert got[k].shape == np.shape(w), (tag, k)
        print(f"{tag} {k}: max rel err {np.max(np.abs(got[k] - w) / np.maximum(np.abs(w), 1e-300)):.3g}")
        np.testing.assert_allclose(got[k], w, rtol=2e-6, atol=2e-7 * max(np.abs(w).max(), 1.0), err_msg=f"{tag} {k}")


def _compare_grads(got, want, tag, single=False):
    for k, w in want.items():
        w = w[0] if single else w
        assert np.all(np.isfinite(w)) and got[k].shape == w.shape, (tag, k)
        print(f"{tag} grad {k}: max err / max|want| {np.abs(got[k] - w).max() / np.abs(w).max():.3g}")
        np.testing.assert_allclose(got[k], w, rtol=2e-6, atol=2e-7 * np.abs(w).max(), err_msg=f"{tag} grad {k}")


@pytest.mark.parametrize("name", cases.NAMES)
def test_values_and_gradients_match_the_restatement(name):
    c = cases.case(name)
    got, got_g = _hip(c)
    want, want_g = cases.expected(name)
    _compare_values(got, want, name, c["single"])
    _compare_grads(got_g, want_g, name, c["single"])
    for k in ro.TERMS:
        assert got[k].dtype == np.float64 and got[k].ndim == (0 if c["single"] else 1)


@pytest.mark.parametrize("wrt", [("pos",), ("image", "depth")])
def test_inputs_that_do_not_require_grad_get_none(wrt):
    c = cases.case("17x9_b3")
    got, got_g = _hip(c, wrt=wrt)
    want, want_g = cases.expected("17x9_b3", wrt=wrt)
    _compare_values(got, want, "17x9_b3")
    for k in ro.INPUTS:
        if k not in wrt:
            assert got_g[k] is None, k
    _compare_grads({k: got_g[k] for k in wrt}, want_g, f"17x9_b3 wrt {wrt}")


def test_two_runs_are_bit_identical():
    c = cases.case("70x33_b2")
    v1, g1 = _hip(c)
    v2, g2 = _hip(c)
    for k in ro.TERMS:
        assert np.array_equal(v1[k], v2[k]), k
    for k in ro.INPUTS:
        assert np.array_equal(g1[k], g2[k]), k


def test_a_batch_equals_its_views_bit_for_bit():
    c = cases.case("70x33_b2")
    v, g = _hip(c)
    for b in range(2):
        one = dict(c, **{k: c[k][b:b + 1] for k in ro.INPUTS}, weights=c["weights"][b:b + 1])
        v1, g1 = _hip(one)
        for k in ro.TERMS:
            assert np.array_equal(v[k][b:b + 1], v1[k]), (b, k)
        for k in ro.INPUTS:
            assert np.array_equal(g[k][b:b + 1], g1[k]), (b, k)


def test_a_zero_normal_gets_no_unit_normal_gradient():
    c = dict(cases.case("5x3"))
    c["normal"] = c["normal"].copy()
    c["normal"][0, 2, 1] = 0.0
    only_unit = np.zeros((1, 7), dtype=np.float32)
    only_unit[0, ro.TERMS.index("unit_normal")] = 1.5
    got, got_g = _hip(c, weights=only_unit)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert all(np.all(np.isfinite(g)) for g in got_g.values())
    assert np.all(got_g["normal"][0, 2, 1] == 0.0)
    assert np.count_nonzero(got_g["normal"]) == got_g["normal"].size - 3        # every other normal has one
    got, got_g = _hip(c)                                                      # all seven terms: still finite
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert all(np.all(np.isfinite(g)) for g in got_g.values())
    # everywhere else the gradients are the restatement's (its own value at the zero normal is NaN: autograd's 0 / 0)
    x = {k: c[k] for k in ro.INPUTS}
    _, want_g = ro.gradients(x, c["weights"], c["z_min"], c["z_max"], c["z_scale"], c["unit_normal_scale"])
    assert not np.all(np.isfinite(want_g["normal"][0, 2, 1]))
    keep = np.ones((1, 5, 3), dtype=bool)
    keep[0, 2, 1] = False
    for k in ("pos", "image", "depth"):
        np.testing.assert_allclose(got_g[k], want_g[k], rtol=2e-6, atol=2e-7 * np.abs(want_g[k]).max(), err_msg=k)
    np.testing.assert_allclose(got_g["normal"][keep], want_g["normal"][keep], rtol=2e-6,
                               atol=2e-7 * np.abs(want_g["normal"][keep]).max())


def test_other_dtypes_and_layouts_are_converted_and_the_gradient_comes_back_in_the_leafs_own():
    from surf_renderer_amd import splat_regularizers
    c = cases.case("9x17")
    pos = torch.tensor(c["pos"].astype(np.float64), device=DEV, requires_grad=True)                    # fp64 leaf
    image_t = torch.tensor(np.ascontiguousarray(c["image"].transpose(0, 2, 1, 3)), device=DEV, requires_grad=True)
    x = {"pos": pos, "normal": torch.tensor(c["normal"], device=DEV), "image": image_t.permute(0, 2, 1, 3),
         "depth": torch.tensor(c["depth"], device=DEV)}
    terms = splat_regularizers(x, c["z_min"], c["z_max"])
    w = torch.tensor(c["weights"], device=DEV)
    sum((w[:, k] * terms[name]).sum() for k, name in enumerate(ro.TERMS)).backward()
    _, want_g = cases.expected("9x17")
    assert pos.grad.dtype == torch.float64 and pos.grad.shape == pos.shape
    assert image_t.grad.shape == image_t.shape
    _compare_grads({"pos": pos.grad.cpu().numpy(), "image": image_t.grad.permute(0, 2, 1, 3).cpu().numpy().astype(np.float64)},
                   {"pos": want_g["pos"], "image": want_g["image"]}, "9x17 converted")


def test_end_to_end_from_the_renderer_to_the_splat_depths():
    from surf_renderer_amd import render_splats_along_ray_batch, splat_regularizers
    sc = e2e.scene()
    z = torch.tensor(sc["objects"]["disk"]["pos"], device=DEV, requires_grad=True)
    sc["objects"]["disk"]["pos"] = z
    for grp, k in (("lights", "color_idx"),):
        sc[grp][k] = torch.as_tensor(sc[grp][k], device=DEV)
    sc["objects"]["disk"]["material_idx"] = torch.as_tensor(sc["objects"]["disk"]["material_idx"], device=DEV)
    res = render_splats_along_ray_batch(sc, samples=e2e.K, normal_estimation_method="plane")
    assert res["pos"].shape == (e2e.B, e2e.K * e2e.H, e2e.K * e2e.W, 3)
    terms = splat_regularizers(res, e2e.Z_MIN, e2e.Z_MAX)
    sum(float(w) * terms[k].sum() for w, k in zip(e2e.WEIGHTS, ro.TERMS)).backward()
    torch.cuda.synchronize()
    want, want_g = e2e.expected()
    for k in ro.TERMS:
        # the regularisers see the renderer's fp32-rounded outputs: the same relative bound as the gradients
        got = terms[k].detach().cpu().numpy().astype(np.float64)
        print(f"e2e {k}: got {got} want {want[k]}")
        np.testing.assert_allclose(got, want[k], rtol=2e-4, atol=1e-6, err_msg=k)
    got_g = z.grad.cpu().numpy().astype(np.float64)
    assert np.abs(want_g).max() > 0
    print(f"e2e grad disk.pos: max err / max|want| {np.abs(got_g - want_g).max() / np.abs(want_g).max():.3g}")
    np.testing.assert_allclose(got_g, want_g, rtol=0, atol=2e-4 * np.abs(want_g).max() + 1e-6)
