"""The chain surf_renderer_amd/mesh_sampling.py documents -- sample_mesh_batched into nearest_points / hausdorff, back
to the vertices -- on the GPU, stage by stage.  Each stage's reference is the fp64 oracle of that stage on the float32
inputs the stage actually got, so every bound is an existing one (tests/mesh_sampling_checks.py,
tests/pointsets_checks.py):

  1  r.pos against the mesh oracle;
  2  distances, indices, r.pos.grad and target.grad against the point-set oracle evaluated on the GPU's float32 r.pos;
  3  v.grad against the mesh oracle's gradients under the retained float32 r.pos.grad.

Under hausdorff the sampler's upstream gradient is exactly zero on all but a sample or two per view.  Run with -s for
the worst ratios."""
import functools

import numpy as np
import pytest
import torch

import mesh_sampling_cases as cases
import mesh_sampling_checks as mesh
import mesh_sampling_oracle as mesh_oracle
import pointsets_checks as points
import pointsets_oracle as points_oracle

pytestmark = pytest.mark.gpu
DEV = mesh.DEV
CASES = [3, 6]                                                          # cube_s257_eyes, f65_s65_fviews_eyes
M = 257                                                                 # points of the target cloud
LOSSES = ("nearest", "squared_directed", "hausdorff")


@functools.lru_cache(maxsize=None)
def setup(k):
    """the case, its mesh oracle per view (values only), the target [3, 257, 3] float32 -- the oracle's own points, in
    turn, displaced by seeded noise of about 0.05 so that no pair coincides -- and the seeded upstreams of the losses"""
    c = cases.regular(k)
    T = [mesh.view_oracle(*cases.view_of(c, b)) for b in range(cases.VIEWS)]
    S = c["uniforms"].shape[1]
    rng = np.random.RandomState(91000 + k)
    target = cases.f32(np.stack([t["pos"][np.arange(M) % S] for t in T]) + 0.05 * rng.standard_normal((cases.VIEWS, M, 3)))
    sign = lambda shape: rng.uniform(0.25, 1, shape) * rng.choice([-1, 1], shape)     # noqa: E731
    ups = {"g_u": cases.f32(sign((cases.VIEWS, S))), "g_v": cases.f32(sign((cases.VIEWS, M))),
           "g3": cases.f32(sign((cases.VIEWS, 3)))}
    return c, T, target, ups


def chain(k, loss, v_leaf=None):
    """one forward and backward of the chain: (r, outputs of the point-set layer, v leaf, target leaf)"""
    from surf_renderer_amd import hausdorff_batched, mesh_topology, nearest_points, sample_mesh_batched
    c, _T, target, ups = setup(k)
    v = mesh.leaf(c["v"]) if v_leaf is None else v_leaf
    t = points.leaf(target)
    topo = mesh_topology(c["f"], c["v"].shape[1])
    r = sample_mesh_batched(v, c["f"], np.array(c["uniforms"]), eye=np.array(c["eye"]), topology=topo)
    r.pos.retain_grad()
    g = {key: torch.tensor(a, device=DEV) for key, a in ups.items()}
    if loss == "nearest":
        out = nearest_points(r.pos, t)
        total = (out.dist_u * g["g_u"]).sum() + (out.dist_v * g["g_v"]).sum()
    elif loss == "squared_directed":
        out = nearest_points(r.pos, t, squared=True, directed=True)
        assert out.dist_v is None and out.idx_v is None
        total = (out.dist_u * g["g_u"]).sum()
    else:
        out = torch.stack(hausdorff_batched(r.pos, t), dim=-1)          # [B, 3] = (sym, uv, vu)
        total = (out * g["g3"]).sum()
    total.backward()
    return r, out, v, t


def numpy_of(t):
    return t.detach().cpu().numpy()


def margins(u, v):
    """the smallest relative gap between the best and the second-best squared distance, both ways: the indices are the
    oracle's where it is far above fp64's rounding"""
    worst = np.inf
    for q, t in ((u, v), (v, u)):
        s = np.sort(points_oracle.pair_d2(q, t), axis=1)
        worst = min(worst, ((s[:, 1] - s[:, 0]) / s[:, 1]).min())
    return worst


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("k", CASES, ids=cases.tag)
def test_every_stage_of_the_chain_has_its_own_oracles_values_and_gradients(k, loss):
    c, T, target, ups = setup(k)
    r, out, v, t = chain(k, loss)
    pos, g_pos, g_target, g_v = numpy_of(r.pos), numpy_of(r.pos.grad), numpy_of(t.grad), numpy_of(v.grad)
    assert g_pos.dtype == np.float32 and g_pos.shape == pos.shape and g_v.shape == c["v"].shape
    got = {key: numpy_of(a) for key, a in r._asdict().items()}
    got["grad_v"] = None
    worst = {"pos": 0.0, "dist": 0.0, "grad_pos": 0.0, "grad_target": 0.0, "grad_v": 0.0}
    for b in range(cases.VIEWS):
        where = f"{loss}, view {b}"
        # stage 1: the samples
        worst["pos"] = max(worst["pos"], mesh.check_view(got, T[b], b, where)[0])
        # stage 2: the point-set layer on the float32 points it was given
        assert margins(pos[b], target[b]) > 2.0 ** -30, where
        N = points_oracle.nearest(pos[b], target[b], squared=loss == "squared_directed")
        if loss == "hausdorff":
            N = points_oracle.nearest(pos[b], target[b])
            want = np.array(points_oracle.hausdorff(N))
            worst["dist"] = max(worst["dist"], points.check_values(numpy_of(out)[b], want, where))
            g_u, g_w = points_oracle.hausdorff_upstreams(N, ups["g3"][b].astype(np.float64))
            G = points_oracle.gradients(pos[b], target[b], N["idx_u"], N["idx_v"], g_u, g_w)
        else:
            sides = "u" if loss == "squared_directed" else "uv"
            for side in sides:
                assert np.array_equal(numpy_of(getattr(out, "idx_" + side))[b], N["idx_" + side]), (where, side)
                worst["dist"] = max(worst["dist"], points.check_values(numpy_of(getattr(out, "dist_" + side))[b],
                                                                       N["dist_" + side], f"{where} dist_{side}"))
            G = points_oracle.gradients(pos[b], target[b], N["idx_u"], N["idx_v"] if sides == "uv" else None,
                                        ups["g_u"][b], ups["g_v"][b] if sides == "uv" else None,
                                        squared=loss == "squared_directed")
        worst["grad_pos"] = max(worst["grad_pos"], points.check_grads(g_pos[b], G["grad_u"], G["S_u"], f"{where} grad_pos"))
        worst["grad_target"] = max(worst["grad_target"],
                                   points.check_grads(g_target[b], G["grad_v"], G["S_v"], f"{where} grad_target"))
        # stage 3: the sampler's backward under the float32 gradient it was handed
        f = cases.view_faces(c["f"], b)
        V = mesh_oracle.gradients(c["v"][b], f, T[b]["face"], T[b]["bary"], g_pos=g_pos[b], g_normal=None)
        worst["grad_v"] = max(worst["grad_v"], mesh.check_grads(g_v[b], V["grad_v"], V["S_v"], f"{where} grad_v"))
        if loss == "hausdorff":
            # the loss reaches v through the farthest sample and the sample nearest the farthest target point
            rows = np.flatnonzero((g_pos[b] != 0).any(axis=1))
            assert np.array_equal(rows, np.flatnonzero((G["S_u"] != 0).any(axis=1))), where
            assert 1 <= len(rows) <= 2 and set(rows) == {int(N["dist_u"].argmax()), int(N["idx_v"][N["dist_v"].argmax()])}
            assert (np.delete(g_pos[b], rows, axis=0) == 0).all(), where
            touched = np.unique(f[T[b]["face"][rows]])
            assert (np.delete(g_v[b], touched, axis=0) == 0).all() and (g_v[b][touched] != 0).any(), where
    print(f"{cases.tag(k)} {loss}: " + "; ".join(f"{key} {x:.3g}" for key, x in worst.items())
          + " (pos, grad_*: of their bound; dist: ulp)")


@pytest.mark.parametrize("k", CASES, ids=cases.tag)
def test_the_chain_is_bit_identical_from_run_to_run_and_a_float64_cpu_leaf_gets_its_gradient_back(k):
    c = setup(k)[0]
    for loss in LOSSES:
        first, again = chain(k, loss), chain(k, loss)
        for a, b in ((first[2].grad, again[2].grad), (first[3].grad, again[3].grad), (first[0].pos.grad, again[0].pos.grad)):
            assert torch.equal(a, b), loss
        v = mesh.leaf(c["v"], dtype=torch.float64, device="cpu")
        chain(k, loss, v_leaf=v)
        assert v.grad.dtype == torch.float64 and v.grad.device.type == "cpu" and v.grad.shape == v.shape
        assert np.array_equal(v.grad.numpy(), numpy_of(first[2].grad).astype(np.float64)), loss
