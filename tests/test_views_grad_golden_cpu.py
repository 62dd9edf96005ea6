"""The gradient of a batch of views = the per-view gradients, shared leaves summed: the definition the batched HIP
backward (srh_render_views_bwd) is tested against, pinned here to the reference torch backend running its own batch loop
under autograd with one summed loss (tests/golden/v1_views_grad_*.npz, oracle/golden_v1.py).  The per-view
side is oracle/torch_oracle.gradients_tch on the fixture's own scene, cameras and upstream gradients.

Tolerance: 2e-3 of each array's largest entry, the project's figure for float32 reference fixtures (g9 / g10 / n1 / c1).
Measured when the fixtures were made: every leaf within 1.9e-5."""
import numpy as np
import pytest

from oracle import np_oracle_tch
from views_cases import V1_CASES, V1_PER_VIEW, load_v1, oracle_batch_tch, view_scene


@pytest.fixture(scope="module", params=V1_CASES)
def batch(request):
    npz, scene, cams, own, kw = load_v1(request.param)
    scenes = [view_scene(scene, cams[v], own[v]) for v in range(len(cams))]
    refs = [np_oracle_tch.render(sc, **kw) for sc in scenes]
    g = {k: npz["grad_in/" + k].astype(np.float64) for k in ("image", "depth")}
    shared, per_view = oracle_batch_tch(scenes, g, refs, V1_PER_VIEW, **kw)
    return npz, scenes, refs, shared, per_view


def test_stored_winners_and_depths_are_the_oracles(batch):
    npz, scenes, refs, _, _ = batch
    assert npz["ref/nearest"].shape == (4, 22, 72)
    for v, ref in enumerate(refs):
        far = scenes[v]["camera"]["far"]
        hit = ref["depth"] <= far
        assert np.array_equal(npz["ref/depth"][v] <= far, hit)
        assert np.array_equal(npz["ref/nearest"][v][hit], ref["nearest"][hit]), f"view {v}"
        np.testing.assert_allclose(npz["ref/depth"][v], ref["depth"], rtol=2e-6, atol=2e-6, err_msg=f"view {v}")
    assert not (npz["ref/depth"][3] <= scenes[3]["camera"]["far"]).any()        # the fourth view hits nothing
    assert (npz["ref/depth"][:3] <= scenes[0]["camera"]["far"]).mean() > 0.9


def test_shared_leaves_are_summed_over_the_views(batch):
    npz, _, _, shared, _ = batch
    checked = 0
    for key in npz.files:
        if not key.startswith("grad/") or key.count("/") != 1:
            continue
        name = key[5:]
        want = npz[key].astype(np.float64)
        got = shared[name].reshape(want.shape)
        if name in ("plane.pos",):
            got, want = got[:, :3], want[:, :3]
        np.testing.assert_allclose(got, want, atol=2e-3 * max(np.abs(want).max(), 1e-6), err_msg=name)
        checked += 1
    assert checked == 11
    assert np.all(npz["grad/disk.radius"] == 0)


def test_per_view_leaves_get_their_own_views_gradient(batch):
    npz, _, _, _, per_view = batch
    for name in V1_PER_VIEW:
        for v in range(4):
            want = npz[f"grad/{name}/{v}"].astype(np.float64)
            got = per_view[name][v].reshape(want.shape)
            np.testing.assert_allclose(got[:, :3], want[:, :3], atol=2e-3 * max(np.abs(want).max(), 1e-6),
                                       err_msg=f"{name}/{v}")
        # the look-away view: the reference's autograd leaves zeros (not None) on its leaves
        assert npz[f"grad/{name}/3"].shape == per_view[name][3].shape[-2:] and np.all(npz[f"grad/{name}/3"] == 0)
        assert np.all(per_view[name][3] == 0)
        assert all(np.abs(npz[f"grad/{name}/{v}"]).max() > 0 for v in range(3))
