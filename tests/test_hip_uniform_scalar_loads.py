"""GPU: the fragment stage of the binned kernels reads what is the same for every lane of a wave -- the lights, their
colours, attenuation and the ambient term -- through the scalar cache.  That changes no arithmetic: `binned` (one and
four waves per tile) and `fast` must still equal the all-pairs fp64 frame of `exact` bit for bit -- image, depth and nearest -- for
every number of lights, both shading models, a light that sits exactly on a fragment, the all-types kernel, and views
that each bring their own lights.  The scalar cache is not coherent with stores: the last test changes the lights in
place between two renders into one workspace -- eager calls, and graph replays with three frames in flight -- and checks
that the later frames show the new values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("nearest", "depth", "image")
VARIANTS = [("binned", 1), ("binned", 4), ("fast", 0)]


def _render(scene, **kw):
    from surf_renderer_amd import render
    res = render(scene, device="cuda:0", **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}


def _assert_modes_equal_exact(scene, **kw):
    ref = _render(scene, mode="exact", **kw)
    assert np.isfinite(ref["depth"]).mean() > 0.05, "the scene covers too little of the frame to test the fragment stage"
    for mode, wpt in VARIANTS:
        got = _render(scene, mode=mode, waves_per_tile=wpt, **kw)
        for k in KEYS:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{mode} (waves_per_tile={wpt}) vs exact: {k}")
    return ref


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _with_lights(scene, n, rng, phong=False):
    """`n` lights at random positions around the scene, colours from a table of n + 1 entries."""
    pos = rng.uniform(-6.0, 6.0, size=(n, 3))
    pos[:, 2] = rng.uniform(1.0, 8.0, size=n)
    scene["lights"] = {"pos": _f32(np.concatenate([pos, np.ones((n, 1))], axis=1)),
                       "color_idx": rng.integers(0, n + 1, size=n).astype(np.int64)}
    scene["colors"] = _f32(rng.uniform(0.05, 0.9, size=(n + 1, 3)))
    if phong:
        scene["lights"]["attenuation"] = _f32(rng.uniform(0.05, 1.0, size=(n, 3)))
        scene["lights"]["ambient"] = _f32([0.02, 0.01, 0.03])
        n_mat = np.asarray(scene["materials"]["albedo"]).shape[0]
        scene["materials"]["coeffs"] = _f32(np.stack([rng.uniform(0.5, 1.0, n_mat), rng.uniform(0.1, 0.5, n_mat),
                                                      rng.uniform(2.0, 20.0, n_mat)], axis=1))
    return scene


def _cloud(n_lights, rng, phong=False, n=6000, width=256, height=192):
    """Disc cloud with three materials: every tile's finish rounds shade pixels of several discs and materials."""
    from surf_renderer_amd import synthetic
    scene = synthetic.disk_cloud_scene(n, width, height, radius=0.06, seed=int(rng.integers(1, 1 << 30)))
    scene["materials"] = {"albedo": _f32([[0.6, 0.6, 0.6], [0.9, 0.3, 0.2], [0.1, 0.5, 0.8]])}
    scene["objects"]["disk"]["material_idx"] = rng.integers(0, 3, size=n).astype(np.int64)
    return _with_lights(scene, n_lights, rng, phong)


@pytest.mark.parametrize("n_lights", [0, 1, 2, 4, 5, 9])
def test_lambert_light_counts(n_lights):
    _assert_modes_equal_exact(_cloud(n_lights, np.random.default_rng(700 + n_lights)))


@pytest.mark.parametrize("n_lights", [0, 1, 2, 4, 5, 9])
def test_phong_attenuation_ambient_light_counts(n_lights):
    """The torch backend's Phong model with per-light attenuation, an ambient term and specular coefficients."""
    rng = np.random.default_rng(800 + n_lights)
    scene = _cloud(n_lights, rng, phong=True)
    for kw in ({}, {"double_sided": True, "use_quartic": True}):
        _assert_modes_equal_exact(scene, shading="torch", **kw)


@pytest.mark.parametrize("shading", ["numpy", "torch"])
def test_light_exactly_on_a_fragment(shading):
    """65 x 33 pixels: the linspace steps are 2^-5 and 2^-4, the centre pixel's ray is exactly (0, 0, -1), and it meets
    the wall disc z = 0 at exactly t = 4, p = (0, 0, 0) -- where the second light sits: |l| = 0 for that fragment
    (numpy/renderer.py's |l| <= 0 -> 1; the torch backend's eps-free branch)."""
    from surf_renderer_amd import synthetic
    rng = np.random.default_rng(91)
    n = 400
    scene = synthetic.disk_cloud_scene(n, 65, 33, radius=0.05, seed=17)
    pos = np.asarray(scene["objects"]["disk"]["pos"]).copy()
    nrm = np.asarray(scene["objects"]["disk"]["normal"]).copy()
    rad = np.asarray(scene["objects"]["disk"]["radius"]).copy()
    pos[:, 0] = np.where(np.abs(pos[:, 0]) < 0.3, pos[:, 0] + 0.6, pos[:, 0])     # nothing in front of the centre pixel
    pos[0], nrm[0], rad[0] = [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0], 3.0
    scene["objects"]["disk"].update(pos=_f32(pos), normal=_f32(nrm), radius=_f32(rad))
    _with_lights(scene, 3, rng, phong=shading == "torch")
    scene["lights"]["pos"][1] = [0.0, 0.0, 0.0, 1.0]
    ref = _assert_modes_equal_exact(scene, shading=shading)
    assert ref["nearest"][16, 32] == 0 and ref["depth"][16, 32] == 4.0, "the centre pixel must hit the wall at t = 4"


@pytest.mark.parametrize("shading", ["numpy", "torch"])
def test_mixed_scene_all_types_kernel(shading):
    """Planes, discs, spheres and triangles in one scene: the kernel instantiation that selects the batch per lane."""
    from surf_renderer_amd import synthetic
    rng = np.random.default_rng(33)
    scene = synthetic.demo_scene(320, 240, with_planes=True)
    if shading == "torch":
        n = np.asarray(scene["lights"]["pos"]).shape[0]
        scene["lights"]["attenuation"] = _f32(rng.uniform(0.0, 0.05, size=(n, 3)) + [1.0, 0.0, 0.0])
        scene["lights"]["ambient"] = _f32([0.02, 0.02, 0.01])
        n_mat = np.asarray(scene["materials"]["albedo"]).shape[0]
        scene["materials"]["coeffs"] = _f32([[0.8, 0.3, 8.0]] * n_mat)
    _assert_modes_equal_exact(scene, shading=shading)


@pytest.mark.parametrize("shading", ["numpy", "torch"])
def test_render_views_lights_per_view(shading):
    """One call, four views, each with its own light positions and colour table: every view must equal an exact
    render() of the scene with that view's lights."""
    from surf_renderer_amd import render_views, synthetic
    rng = np.random.default_rng(55)
    base = _cloud(4, rng, phong=shading == "torch", n=3000, width=160, height=128)
    cams, overrides, scenes = [], [], []
    for v in range(4):
        sc = synthetic.clone(base)
        lp = np.asarray(base["lights"]["pos"]).copy()
        lp[:, :3] += rng.uniform(-2.0, 2.0, size=(4, 3))
        sc["lights"]["pos"] = _f32(lp)
        sc["colors"] = _f32(rng.uniform(0.05, 0.9, size=np.asarray(base["colors"]).shape))
        sc["camera"]["eye"] = [0.3 * v, -0.2 * v, 4.0, 1.0]
        scenes.append(sc)
        cams.append(sc["camera"])
        overrides.append({"lights.pos": sc["lights"]["pos"], "colors": sc["colors"]})
    refs = [_render(sc, mode="exact", shading=shading) for sc in scenes]
    for mode, wpt in VARIANTS:
        out = render_views(base, cams, device="cuda:0", mode=mode, overrides=overrides, shading=shading,
                           waves_per_tile=wpt)
        torch.cuda.synchronize()
        for v in range(4):
            for k in KEYS:
                got = out[k][v].cpu().numpy()
                assert got.dtype == (np.int32 if k == "nearest" else np.float32), f"render_views {k}: {got.dtype}"
                np.testing.assert_array_equal(got, refs[v][k].astype(got.dtype),
                                              err_msg=f"render_views {mode} (waves_per_tile={wpt}) view {v}: {k}")


@pytest.mark.parametrize("shading", ["numpy", "torch"])
@pytest.mark.parametrize("mode", ["binned", "fast"])
def test_lights_changed_in_place_are_seen(mode, shading):
    """Render, overwrite the light positions and the colour table in place, render again into the same workspace: the
    second frame must be the exact frame of the NEW lights (and differ from the first)."""
    from surf_renderer_amd import ResidentScene, synthetic
    rng = np.random.default_rng(77)
    host = _cloud(4, rng, phong=shading == "torch", n=3000, width=160, height=128)
    scene = synthetic.clone(host)
    lpos = torch.tensor(np.asarray(host["lights"]["pos"]), dtype=torch.float32, device="cuda:0")
    colors = torch.tensor(np.asarray(host["colors"]), dtype=torch.float32, device="cuda:0")
    scene["lights"]["pos"], scene["colors"] = lpos, colors
    rs = ResidentScene(scene, device="cuda:0", shading=shading, mode=mode)
    first = {k: rs.render()[k].cpu().numpy() for k in KEYS}
    ref0 = _render(host, mode="exact", shading=shading)
    for k in KEYS:
        assert first[k].dtype == (np.int32 if k == "nearest" else np.float32), f"ResidentScene {k}: {first[k].dtype}"
        np.testing.assert_array_equal(first[k], ref0[k].astype(first[k].dtype), err_msg=f"first frame: {k}")
    moved = synthetic.clone(host)
    new_pos = np.asarray(host["lights"]["pos"]).copy()
    new_pos[:, :3] = new_pos[:, :3][::-1] * [1.0, -1.0, 1.5]
    moved["lights"]["pos"] = _f32(new_pos)
    moved["colors"] = _f32(np.asarray(host["colors"])[::-1] * 0.7)
    lpos.copy_(torch.tensor(moved["lights"]["pos"], dtype=torch.float32))
    colors.copy_(torch.tensor(moved["colors"], dtype=torch.float32))
    second = {k: rs.render()[k].cpu().numpy() for k in KEYS}
    ref1 = _render(moved, mode="exact", shading=shading)
    assert not np.array_equal(ref0["image"], ref1["image"])
    for k in KEYS:
        np.testing.assert_array_equal(second[k], ref1[k].astype(second[k].dtype), err_msg=f"second frame: {k}")


@pytest.mark.parametrize("schedule", ["frames", "stages"])
def test_lights_changed_between_graph_replays_are_seen(schedule):
    """The benchmark's path: three frames in flight, each a captured graph replayed on its own stream.  The lights are
    overwritten in place between two rounds of replays; every slab of the second round must hold the exact frame of
    the NEW lights."""
    from surf_renderer_amd import renderer, synthetic
    from surf_renderer_amd.pipeline import FramePipeline, slab_views
    rng = np.random.default_rng(78)
    host = _cloud(4, rng, n=3000, width=160, height=128)
    scene = synthetic.clone(host)
    lpos = torch.tensor(np.asarray(host["lights"]["pos"]), dtype=torch.float32, device="cuda:0")
    colors = torch.tensor(np.asarray(host["colors"]), dtype=torch.float32, device="cuda:0")
    scene["lights"]["pos"], scene["colors"] = lpos, colors
    buf = renderer.flatten_scene(scene, "cuda:0")
    pipe = FramePipeline(buf, renderer.camera_struct(scene["camera"]), n_inflight=3, mode="binned", graphs=True,
                         strict_graphs=True, schedule=schedule)
    assert pipe.captured == 3

    def slabs_equal(ref, what):
        pipe.sync()
        for b, slab in enumerate(pipe.slabs):
            image, depth = slab_views(slab, 160)
            np.testing.assert_array_equal(image.cpu().numpy(), ref["image"], err_msg=f"{what}, slab {b}: image")
            np.testing.assert_array_equal(depth.cpu().numpy(), ref["depth"], err_msg=f"{what}, slab {b}: depth")

    for _ in range(6):
        pipe.submit()
    ref0 = _render(host, mode="exact")
    slabs_equal(ref0, "first round")
    moved = synthetic.clone(host)
    new_pos = np.asarray(host["lights"]["pos"]).copy()
    new_pos[:, :3] = new_pos[:, :3][::-1] * [1.0, -1.0, 1.5]
    moved["lights"]["pos"] = _f32(new_pos)
    moved["colors"] = _f32(np.asarray(host["colors"])[::-1] * 0.7)
    lpos.copy_(torch.tensor(moved["lights"]["pos"], dtype=torch.float32))
    colors.copy_(torch.tensor(moved["colors"], dtype=torch.float32))
    torch.cuda.synchronize()
    for _ in range(6):
        pipe.submit()
    ref1 = _render(moved, mode="exact")
    assert not np.array_equal(ref0["image"], ref1["image"])
    slabs_equal(ref1, "second round")
