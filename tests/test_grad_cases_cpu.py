"""tests/grad_cases.py on CPU tensors: the helpers that replaced several hand-written variants each -- the leaf-scene
builder, the masked loss and the gradient extraction -- against what those variants did, written out by hand."""
import numpy as np
import torch

from grad_cases import NP_KEYS, TCH_KEYS, gpu_leaf_scene, leaf_grads, load, masked_loss
from oracle.torch_oracle import LEAF_KEYS
from views_cases import get_leaf


# float32 sums of about a hundred terms of magnitude up to 10 against fp64: at most 100 * 2^-24 * 10 = 6e-5; a pixel
# masked wrongly moves the loss by more than 1e-2 (asserted below)
ATOL = 1e-4


def _object_keys(scene):
    return {f"{kind}.{name}" for kind in scene["objects"] for name in LEAF_KEYS[kind]}


def test_gpu_leaf_scene_on_the_g10_fixture():
    scene = load("g10_torch_autograd_phong")[1]
    assert set(scene["objects"]) == {"disk", "plane", "sphere", "triangle"}
    for extra in (NP_KEYS, TCH_KEYS):
        sc, leaves = gpu_leaf_scene(scene, extra, device="cpu")
        assert set(leaves) == _object_keys(scene) | set(extra)
        for key, t in leaves.items():
            assert get_leaf(sc, key) is t and t.requires_grad and t.is_leaf
            assert t.dtype == torch.float32 and t.device.type == "cpu"
            assert np.array_equal(t.detach().numpy(), np.asarray(get_leaf(scene, key), dtype=np.float32)), key
            assert isinstance(get_leaf(scene, key), np.ndarray), key           # the caller's scene is untouched
        assert sc["camera"] is not scene["camera"] and sc["objects"]["disk"] is not scene["objects"]["disk"]
        assert np.array_equal(sc["objects"]["disk"]["material_idx"], scene["objects"]["disk"]["material_idx"])
    assert isinstance(gpu_leaf_scene(scene, NP_KEYS, device="cpu")[0]["materials"]["coeffs"], np.ndarray)

    skip = ("disk.pos", "lights.pos")
    sc, leaves = gpu_leaf_scene(scene, TCH_KEYS, skip=skip, device="cpu")
    assert set(leaves) == (_object_keys(scene) | set(TCH_KEYS)) - set(skip)
    for key in skip:
        t = get_leaf(sc, key)
        assert isinstance(t, torch.Tensor) and not t.requires_grad

    sc, leaves = gpu_leaf_scene(scene, TCH_KEYS, grad=False, device="cpu")
    assert leaves == {}
    assert all(isinstance(get_leaf(sc, k), torch.Tensor) and not get_leaf(sc, k).requires_grad
               for k in _object_keys(scene) | set(TCH_KEYS))


def _frame():
    """A 3 x 4 frame with two misses: (0, 1) as torch shading marks one (far + 1), (2, 3) as numpy shading does (inf)."""
    rng = np.random.RandomState(3)
    res = {k: torch.tensor(rng.uniform(-1, 1, size=(3, 4, 3)), dtype=torch.float32, requires_grad=True)
           for k in ("image", "normal", "pos")}
    depth = rng.uniform(1, 9, size=(3, 4))
    depth[0, 1], depth[2, 3] = 11.0, np.inf
    res["depth"] = torch.tensor(depth, dtype=torch.float32, requires_grad=True)
    g = {"image": rng.uniform(-1, 1, size=(3, 4, 3)), "depth": rng.uniform(-1, 1, size=(3, 4)),
         "normal": rng.uniform(-1, 1, size=(3, 4, 3)), "pos": rng.uniform(-1, 1, size=(3, 4, 3))}
    return res, g


def _by_hand(res, g, hit):
    """sum image g_i + sum over `hit` of (depth g_d + normal . g_n + pos . g_p) in fp64 on the float32 values."""
    r = {k: t.detach().numpy().astype(np.float64) for k, t in res.items()}
    u = {k: a.astype(np.float32).astype(np.float64) for k, a in g.items()}
    with np.errstate(invalid="ignore"):
        dep = np.where(hit, r["depth"] * u["depth"], 0.0)                      # inf * g stays out of the sum
    return np.sum(r["image"] * u["image"]) + np.sum(dep) + np.sum((r["normal"] * u["normal"])[hit]) + \
        np.sum((r["pos"] * u["pos"])[hit])


def test_masked_loss_is_the_formula_written_out():
    res, g = _frame()
    dep = res["depth"].detach().numpy()
    cases = [(dict(far=10.0), dep <= 10.0), (dict(far=None), np.isfinite(dep))]
    assert [int((~hit).sum()) for _, hit in cases] == [2, 1]
    for kw, hit in cases:
        loss = masked_loss(res, g, **kw)
        assert loss.dtype == torch.float32 and loss.requires_grad
        np.testing.assert_allclose(float(loss.detach()), _by_hand(res, g, hit), rtol=0, atol=ATOL)
        # the masked pixels get no gradient, the image gets its upstream everywhere
        grads = torch.autograd.grad(loss, [res["depth"], res["pos"], res["image"]])
        assert np.array_equal(grads[0].numpy() != 0, hit) and np.array_equal((grads[1].numpy() != 0).all(-1), hit)
        assert np.array_equal(grads[2].numpy(), g["image"].astype(np.float32))
    # mask=False: every pixel of every output, misses included
    finite = dict(res, depth=res["depth"].detach().clamp(max=11.0))
    everywhere = np.ones((3, 4), dtype=bool)
    for kw in (dict(far=10.0), dict(far=None)):
        np.testing.assert_allclose(float(masked_loss(finite, g, mask=False, **kw).detach()), _by_hand(finite, g, everywhere),
                                   rtol=0, atol=ATOL)
    assert abs(_by_hand(finite, g, everywhere) - _by_hand(finite, g, cases[0][1])) > 1e-2
    # None entries and absent outputs are left out
    part = {"image": g["image"], "depth": None, "pos": g["pos"]}
    want = _by_hand(res, dict(g, depth=np.zeros((3, 4)), normal=np.zeros((3, 4, 3))), cases[0][1])
    np.testing.assert_allclose(float(masked_loss(res, part, far=10.0).detach()), want, rtol=0, atol=ATOL)


def test_leaf_grads_gives_zeros_for_a_leaf_the_loss_does_not_reach():
    a = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], requires_grad=True)
    b = torch.ones((4, 1, 2), requires_grad=True)
    (a * a).sum().backward()
    got = leaf_grads({"reached": a, "not reached": b})
    assert b.grad is None
    assert got["not reached"].shape == (4, 1, 2) and got["not reached"].dtype == np.float64 and not got["not reached"].any()
    assert got["reached"].dtype == np.float64 and np.array_equal(got["reached"], 2.0 * a.detach().numpy())
