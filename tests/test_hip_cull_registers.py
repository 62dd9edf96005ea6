"""GPU: the binned disc kernel after its cull order moved into registers (DPP / permlane compare-exchanges in the
bitonic sort and in the tile minimum of the stop test) and its finish rounds stopped spilling frame constants.  The
binned frame must still equal the all-pairs fp64 frame bit for bit -- image, depth and nearest -- at the headline
workload (config 5) and on a small scene where the cull skips most of every busy tile's list, with lists of both sort
widths (up to 64 entries, and 65-128)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _render(scene, **kw):
    from surf_renderer_amd import render
    res = render(scene, device="cuda:0", **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in ("image", "depth", "nearest")}


def _assert_binned_equals_exact(scene):
    ref = _render(scene, mode="exact")
    got = _render(scene, mode="binned", waves_per_tile=1)      # one wave per tile: the culled path
    for k in ("nearest", "depth", "image"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"binned vs exact: {k}")


def test_config5_binned_equals_exact():
    from surf_renderer_amd import synthetic
    _assert_binned_equals_exact(synthetic.disk_cloud_scene(100_000, 2048, 2048))


@pytest.mark.parametrize("per_tile", [30, 80])
def test_cull_heavy_stack_equals_exact(per_tile):
    """A wall of large facing discs in front of a cloud of small ones: the wall certainly covers every pixel, so the
    sweep stops after the first sorted groups; `per_tile` sets roughly how many entries a busy tile lists (sorts of 64
    and of 128 entries)."""
    from surf_renderer_amd import synthetic
    rng = np.random.default_rng(505 + per_tile)
    width, height = 192, 128
    n_tiles = (width // 16) * (height // 16)
    n_cloud = int(per_tile * n_tiles / 2.4)                     # a small disc's box reaches ~2.4 tiles
    wall_x, wall_y = np.meshgrid(np.linspace(-2.4, 2.4, 17), np.linspace(-1.6, 1.6, 11))
    wall = np.stack([wall_x.ravel(), wall_y.ravel(), np.full(wall_x.size, 0.5) + rng.uniform(0, 1e-3, wall_x.size)], 1)
    cloud = np.stack([rng.uniform(-2, 2, n_cloud), rng.uniform(-1.4, 1.4, n_cloud), rng.uniform(-1.0, 0.3, n_cloud)], 1)
    nrm = rng.normal(size=(n_cloud, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[nrm[:, 2] < 0] *= -1.0
    pos = np.concatenate([wall, cloud])
    normal = np.concatenate([np.tile([0.0, 0.0, 1.0], (len(wall), 1)), nrm])
    rad = np.concatenate([np.full(len(wall), 0.3), np.full(n_cloud, 0.12)])
    scene = synthetic.disk_cloud_scene(4, width, height)
    n = len(rad)
    scene["camera"]["near"], scene["camera"]["far"] = 0.1, 1000.0
    scene["objects"]["disk"] = {
        "pos": np.concatenate([pos, np.ones((n, 1))], axis=1).astype(np.float32),
        "normal": np.concatenate([normal, np.zeros((n, 1))], axis=1).astype(np.float32),
        "radius": rad.astype(np.float32),
        "material_idx": np.zeros(n, dtype=np.int64)}
    _assert_binned_equals_exact(scene)
