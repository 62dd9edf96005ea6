"""sample_mesh_batched and uniform_sample_mesh on the GPU against the fp64 oracle (tests/mesh_sampling_oracle.py) and
the reference's recorded samples (tests/golden/mesh_sampling) on the regular cases: `face` exact; bary, pos and normal
within 2^-24 |ref| + 2^-50 S; every entry of grad_v within 2^-23 |ref| + 2^-40 S (tests/mesh_sampling_checks.py derives
both); determinism, batch = views, [V, 3] = B = 1, the topology object, the reference's random stream, dtype and device
of the gradient, and the autograd plumbing of each output alone.  Run with -s for the worst measured ratios."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_sampling_cases as cases
from conftest import GOLDEN_DIR
from mesh_sampling_checks import DEV, check_values, check_view, leaf, run, run_case, view_oracle

pytestmark = pytest.mark.gpu
ALL = range(len(cases.REGULAR))
# a few shapes for the properties that do not depend on the size: shared and per-view faces, no eye, one eye, an eye per
# view, and the one past the scan's tile
SOME = [1, 4, 6, 7, 8]


@functools.lru_cache(maxsize=None)
def fixture(k):
    return dict(np.load(os.path.join(GOLDEN_DIR, "mesh_sampling", "ms1_" + cases.tag(k) + ".npz")))


@functools.lru_cache(maxsize=None)
def truth(k, upstream=("g_pos", "g_normal")):
    """per view the oracle's values and its gradients under the case's upstream gradients"""
    c = cases.regular(k)
    return [view_oracle(*cases.view_of(c, b), *[c[g][b] if g in upstream else None for g in ("g_pos", "g_normal")])
            for b in range(cases.VIEWS)]


@pytest.mark.parametrize("k", ALL, ids=cases.tag)
def test_a_batch_has_the_oracles_faces_values_and_gradients_and_the_references_samples(k):
    c, T, z = cases.regular(k), truth(k), fixture(k)
    got = run_case(c)
    S = c["uniforms"].shape[1]
    assert got["face"].dtype == np.int64 and got["face"].shape == (cases.VIEWS, S)
    for key in ("pos", "normal", "bary"):
        assert got[key].dtype == np.float32 and got[key].shape == (cases.VIEWS, S, 3)
    assert got["grad_v"].shape == c["v"].shape
    worst = worst_g = 0.0
    for b in range(cases.VIEWS):
        a, g = check_view(got, T[b], b, f"view {b}")
        worst, worst_g = max(worst, a), max(worst_g, g)
        assert np.array_equal(got["face"][b], z["ref/face"][b])
        for key in ("pos", "normal"):                                  # the reference's own samples
            check_values(got[key][b], z["ref/" + key][b], T[b]["S_" + key], f"view {b} reference {key}")
    print(f"{cases.tag(k)}: values {worst:.3g} of their bound; gradients {worst_g:.3g} of theirs")


@pytest.mark.parametrize("k", SOME, ids=cases.tag)
def test_runs_are_bit_identical_and_a_batch_equals_its_views_and_a_single_mesh_equals_b_1(k):
    c = cases.regular(k)
    a, again = run_case(c), run_case(c)
    for key in a:
        assert np.array_equal(a[key], again[key], equal_nan=True), key
    for b in range(cases.VIEWS):
        one, b1 = run_case(c, b), run_case(c, slice(b, b + 1))
        for key in a:
            assert one[key].shape == a[key].shape[1:], key
            assert np.array_equal(one[key], a[key][b]) and np.array_equal(b1[key][0], a[key][b]), (key, b)


@pytest.mark.parametrize("k", [4, 8], ids=cases.tag)
def test_a_topology_made_once_gives_what_the_call_builds_itself(k):
    from surf_renderer_amd import mesh_topology, sample_mesh_batched
    c = cases.regular(k)
    want = run_case(c)
    topo = mesh_topology(c["f"], c["v"].shape[1])
    assert topo.n_faces == cases.REGULAR[k][2] and topo.n_views == (cases.VIEWS if c["f"].ndim == 3 else None)
    assert topo.f.dtype == torch.int32 and topo.f.device.type == "cuda" and topo.corner_order.dtype == torch.int32
    for f in (c["f"], None):                                           # with the topology f is optional
        got = run(c["v"], f, c["uniforms"], c["eye"], c["g_pos"], c["g_normal"], topology=topo)
        for key in want:
            assert np.array_equal(got[key], want[key]), key
    if c["f"].ndim == 2:                                               # a shared topology serves any number of views
        r = sample_mesh_batched(c["v"][1], None, c["uniforms"][1], eye=cases.view_eye(c["eye"], 1), topology=topo)
        assert np.array_equal(r.pos.cpu().numpy(), want["pos"][1])


def test_one_eye_for_all_views_is_that_eye_for_each():
    c = cases.regular(5)
    assert c["eye"].shape == (3,)
    a = run_case(c)
    b = run(c["v"], c["f"], c["uniforms"], np.stack([c["eye"]] * cases.VIEWS), c["g_pos"], c["g_normal"])
    none = run(c["v"], c["f"], c["uniforms"], None, c["g_pos"], c["g_normal"])
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert not np.array_equal(a["face"], none["face"])                 # and the cull does something


@pytest.mark.parametrize("k", [2, 3], ids=cases.tag)
def test_after_seeding_numpy_uniform_sample_mesh_returns_the_references_samples(k):
    from surf_renderer_amd import uniform_sample_mesh
    c, z, T = cases.regular(k), fixture(k), truth(k)
    S = c["uniforms"].shape[1]
    for b in range(cases.VIEWS):
        v, f, _, eye = cases.view_of(c, b)
        camera = None if eye is None else {"eye": eye, "at": np.zeros(3), "up": np.array([0.0, 1.0, 0.0])}
        np.random.seed(int(c["seeds"][b]))
        pos, normal = uniform_sample_mesh({"v": v, "f": f}, S, camera)          # the reference's positional call
        after = np.random.random_sample()
        assert pos.shape == (S, 3) and pos.dtype == torch.float32 and pos.device.type == "cuda"
        check_values(pos.cpu().numpy(), z["ref/pos"][b], T[b]["S_pos"], f"view {b} pos")
        check_values(normal.cpu().numpy(), z["ref/normal"][b], T[b]["S_normal"], f"view {b} normal")
        # the stream stands where the reference leaves it: 3 S draws were consumed
        rng = np.random.RandomState(int(c["seeds"][b]))
        rng.random_sample(3 * S)
        assert after == rng.random_sample()
        # a generator of the caller's, and explicit uniforms
        again = uniform_sample_mesh({"v": v, "f": f}, S, camera, rng=np.random.RandomState(int(c["seeds"][b])))
        given = uniform_sample_mesh({"v": v, "f": f}, S, camera, uniforms=c["uniforms"][b])
        for got in (again, given):
            assert torch.equal(got[0], pos) and torch.equal(got[1], normal)


def test_uniform_sample_mesh_is_differentiable_in_the_vertices():
    from surf_renderer_amd import uniform_sample_mesh
    c, T = cases.regular(2), truth(2)
    v = leaf(c["v"][0])
    pos, normal = uniform_sample_mesh({"v": v, "f": torch.tensor(c["f"], device=DEV)}, c["uniforms"].shape[1],
                                      uniforms=torch.tensor(c["uniforms"][0]))
    ((pos * torch.tensor(c["g_pos"][0], device=DEV)).sum() + (normal * torch.tensor(c["g_normal"][0], device=DEV)).sum()).backward()
    check_view({"face": T[0]["face"], "bary": T[0]["bary"], "pos": pos.detach().cpu().numpy(),
                "normal": normal.detach().cpu().numpy(), "grad_v": v.grad.cpu().numpy()}, T[0], None, "cube")


@pytest.mark.parametrize("k", SOME, ids=cases.tag)
def test_a_loss_on_each_output_alone_gives_the_oracles_gradients(k):
    c = cases.regular(k)
    for upstream in (("g_pos",), ("g_normal",)):
        got, T = run_case(c, upstream=upstream), truth(k, upstream)
        for b in range(cases.VIEWS):
            check_view(got, T[b], b, f"{upstream[0]} alone, view {b}")


def test_gradients_come_back_in_the_leafs_own_dtype_layout_and_device():
    from surf_renderer_amd import sample_mesh_batched
    c = cases.regular(6)
    want = run_case(c)
    ups = [torch.tensor(c[g], device=DEV) for g in ("g_pos", "g_normal")]

    def loss_of(leaf_v, seen):
        r = sample_mesh_batched(seen, c["f"], c["uniforms"], eye=c["eye"])
        assert r.pos.device.type == "cuda" and r.pos.dtype == torch.float32
        assert not r.face.requires_grad and not r.bary.requires_grad and r.face.dtype == torch.int64
        ((r.pos * ups[0]).sum() + (r.normal * ups[1]).sum()).backward()
        return leaf_v.grad

    v = leaf(c["v"], dtype=torch.float64, device="cpu")                          # float64 on the CPU
    g = loss_of(v, v)
    assert g.dtype == torch.float64 and g.device.type == "cpu" and g.shape == v.shape
    assert np.array_equal(g.numpy(), want["grad_v"].astype(np.float64))
    v = leaf(np.ascontiguousarray(c["v"].transpose(0, 2, 1)))                    # a transposed view on the GPU
    g = loss_of(v, v.transpose(1, 2))
    assert g.dtype == torch.float32 and g.device.type == "cuda" and g.shape == v.shape
    assert np.array_equal(g.cpu().numpy().transpose(0, 2, 1), want["grad_v"])
    v = leaf(c["v"], dtype=torch.float16)                                        # computed on its float32 values
    assert loss_of(v, v).dtype == torch.float16


def test_vertices_that_do_not_require_grad_launch_no_backward(monkeypatch):
    from surf_renderer_amd import _lib, sample_mesh_batched
    c = cases.regular(6)
    r = sample_mesh_batched(leaf(c["v"], requires_grad=False), c["f"], c["uniforms"])
    assert not r.pos.requires_grad and not r.normal.requires_grad and r.pos.grad_fn is None
    # and a graph that reaches the layer through another leaf only does not call the backward entry point
    calls = []
    lib = _lib.load()
    real = lib.srh_mesh_sample_bwd
    monkeypatch.setattr(lib, "srh_mesh_sample_bwd", lambda *a: calls.append(1) or real(*a))
    scale = torch.ones((), device=DEV, requires_grad=True)
    (sample_mesh_batched(leaf(c["v"], requires_grad=False), c["f"], c["uniforms"]).pos * scale).sum().backward()
    assert scale.grad is not None and not calls
    v = leaf(c["v"])
    sample_mesh_batched(v, c["f"], c["uniforms"]).pos.sum().backward()
    assert calls == [1] and v.grad is not None
