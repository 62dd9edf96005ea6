"""GPU: render(scene, shading='torch') -- the torch backend's semantics -- against the
reference torch backend's own outputs (tests/golden/t*.npz, float32) and the fp64 oracle of those semantics.

Tolerances: against the float32 reference as in tests/test_oracle_tch.py (<= 0.5 % of pixels may differ in hit /
nearest at silhouettes; depth 2e-5 relative, image / normal 3e-4, pos 2e-4 elsewhere); against the fp64 oracle
`nearest` identical, depth one fp32 ulp, image 2e-7 + 2e-6 |x|."""
import os

import numpy as np
import pytest
import torch

from oracle import np_oracle_tch
from shadow_scenes import shadow_both_ways as _shadow_both_ways
from test_oracle_tch import CASES, assert_tch_parity, load_shadow_case, load_tch_case

pytestmark = pytest.mark.gpu


def _render(scene, **kw):
    from surf_renderer_amd import render
    res = render(scene, device="cuda:0", shading="torch", **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in ("image", "depth", "nearest", "normal", "pos")}


@pytest.mark.parametrize("mode", ["exact", "binned"])
@pytest.mark.parametrize("case", CASES)
def test_torch_shading_matches_reference_torch_backend(case, mode):
    scene, want, kw = load_tch_case(case)
    got = _render(scene, mode=mode, **kw)
    assert_tch_parity(got, want, scene["camera"]["far"])


@pytest.mark.parametrize("case", CASES)
def test_torch_shading_matches_fp64_oracle(case):
    scene, _, kw = load_tch_case(case)
    want = np_oracle_tch.render(scene, **kw)
    got = _render(scene, **kw)
    far = scene["camera"]["far"]
    np.testing.assert_array_equal(got["nearest"], want["nearest"])
    np.testing.assert_allclose(got["depth"], want["depth"], rtol=1.2e-7)
    np.testing.assert_allclose(got["image"], want["image"], rtol=2e-6, atol=2e-7)
    hit = want["depth"] <= far
    np.testing.assert_allclose(got["normal"][hit], want["normal"][hit], atol=2e-7)
    np.testing.assert_allclose(got["pos"][hit], want["pos"][hit], rtol=2e-7, atol=2e-6)
    assert np.all(got["normal"][~hit] == 0) and np.all(got["pos"][~hit] == 0)


def test_torch_shading_modes_identical_and_numpy_default_unchanged():
    from surf_renderer_amd import render, synthetic
    scene = synthetic.splat_basic_scene(200, 150)
    a = _render(scene, mode="exact", double_sided=True)
    b = _render(scene, mode="binned", double_sided=True)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    plain = render(scene, device="cuda:0")
    assert "normal" not in plain and torch.isinf(plain["depth"]).any()
    with pytest.raises(ValueError):
        render(scene, device="cuda:0", shadow=True)              # shadows exist in the torch semantics only


def test_orthographic_projection_rules():
    """proj_type 'ortho' exists in the torch backend only: the numpy shading model refuses it.  Under torch shading the
    frame is covered by the t4 / t5 fixtures above, its gradients by golden g11 (tests/test_hip_backward.py), batched
    views by test_orthographic_views_in_one_call_equal_per_view_render below."""
    from surf_renderer_amd import render
    scene, _, kw = load_tch_case("t4_mixed_ortho_64x48")
    with pytest.raises(ValueError):
        render(scene, device="cuda:0")
    leaf = dict(scene, materials=dict(scene["materials"]))
    leaf["materials"]["albedo"] = torch.tensor(np.asarray(scene["materials"]["albedo"], dtype=np.float32), requires_grad=True)
    res = render(leaf, device="cuda:0", shading="torch")
    res["image"].sum().backward()
    assert torch.isfinite(leaf["materials"]["albedo"].grad).all() and leaf["materials"]["albedo"].grad.abs().sum() > 0
    # a row slab of the orthographic frame equals the rows of the full frame
    full = _render(scene, **kw)
    part = _render(scene, rows=(10, 31), **kw)
    for k in ("image", "depth", "nearest"):
        np.testing.assert_array_equal(part[k], full[k][10:31])


@pytest.mark.parametrize("case", ["t2_mixed_specular_64x48", "t2_mixed_specular_64x48_ds", "t4_mixed_ortho_64x48",
                                  "t3_disk_cloud_64x64_ds"])
def test_shadow_pass_matches_the_oracle(case):
    """shadow=True: the all-pairs shadow-ray pass against the oracle's restatement of torch/renderer.py:291-314 (pinned
    by the reference's own shadow renders, tests/golden/s1*.npz).  Both are fp64: the visibility
    bits must agree except where a shadow ray grazes a primitive's edge (<= 0.2 % of hit pixels x lights), and the
    image must match wherever they do."""
    from surf_renderer_amd import render
    scene, _, kw = load_tch_case(case)
    want = np_oracle_tch.render(scene, shadow=True, **kw)
    res = render(scene, device="cuda:0", shading="torch", shadow=True, **kw)
    torch.cuda.synchronize()
    far = scene["camera"]["far"]
    hit = want["depth"] <= far
    np.testing.assert_array_equal(res["nearest"].cpu().numpy(), want["nearest"])
    bits = res["light_visibility"].cpu().numpy()
    L = want["visibility"].shape[0]
    got_vis = np.stack([(bits >> l) & 1 for l in range(L)]).astype(bool)
    agree = (got_vis == want["visibility"]) | ~hit[None]
    assert agree.mean() > 0.998, f"visibility differs on {1 - agree.mean():.3%}"
    assert (~want["visibility"][:, hit]).mean() > 0.01                       # the scene does cast shadows
    same = agree.all(axis=0)
    np.testing.assert_allclose(res["image"].cpu().numpy()[same], want["image"][same], rtol=2e-6, atol=2e-7)
    # and the unshadowed frame is untouched by the option
    base = render(scene, device="cuda:0", shading="torch", **kw)
    assert not np.array_equal(base["image"].cpu().numpy(), res["image"].cpu().numpy())
    np.testing.assert_array_equal(base["depth"].cpu().numpy(), res["depth"].cpu().numpy())


@pytest.mark.parametrize("case", ["s1a_mixed_shadow_64x48", "s1a_mixed_shadow_64x48_ds", "s1b_disk_cloud_shadow_64x64_ds"])
def test_shadow_pass_matches_reference_torch_backend(case):
    """render(shading='torch', shadow=True) against the reference's own render(shadow=True) (float32, CPU;
    oracle/golden_s1.py): same tolerance as the unshadowed reference cases, a grazing shadow ray may flip on
    <= 0.5 % of the pixels."""
    import json
    from conftest import GOLDEN_DIR
    from oracle.golden_io import unpack_scene
    from surf_renderer_amd import render
    npz = np.load(os.path.join(GOLDEN_DIR, case + ".npz"), allow_pickle=False)
    scene, kw = unpack_scene(npz), json.loads(str(npz["kwargs"]))
    res = render(scene, device="cuda:0", shading="torch", shadow=True, **kw)
    far = scene["camera"]["far"]
    same = (res["nearest"].cpu().numpy() == npz["out/nearest"]) | (npz["out/depth"] > far)
    assert same.mean() >= 0.995
    err = np.abs(res["image"].cpu().numpy() - npz["out/image"]).max(axis=-1)
    assert (err[same] > 3e-4).mean() <= 0.005, f"{(err[same] > 3e-4).mean():.3%} of pixels differ from the reference"


def test_norm_depth_image_only_follows_the_reference_formula():
    """torch/renderer.py:245-249.  Unpinned by a fixture (the reference's own call raises, oracle/check_ref_kwargs.py):
    checked against the oracle's restatement of those lines applied to the oracle's depth."""
    from surf_renderer_amd import render
    for case in ("t2_mixed_specular_64x48", "t3_disk_cloud_64x64"):
        scene, _, kw = load_tch_case(case)
        far = scene["camera"]["far"]
        want_depth = np_oracle_tch.render(scene, **kw)["depth"]
        want = np_oracle_tch.norm_depth_image(want_depth.astype(np.float32), far)
        res = render(scene, device="cuda:0", shading="torch", norm_depth_image_only=True, **kw)
        torch.cuda.synchronize()
        assert set(res.keys()) == {"image", "depth", "nearest"} and res["image"].shape == res["depth"].shape
        got = res["image"].cpu().numpy()
        np.testing.assert_allclose(got, want, atol=2e-6)
        bg = want_depth > far
        # the maximum over ALL pixels is far + 1 as soon as one pixel is background (:249 divides by it), 1.0 otherwise
        assert got.min() == 0.0 and (got.max() == 1.0 if not bg.any() else got.max() < 1.0)
        np.testing.assert_array_equal(got[bg] == 0.0, True)                    # background sits at the minimum
    with pytest.raises(ValueError):
        render(scene, device="cuda:0", norm_depth_image_only=True)              # numpy semantics have no such output


def test_torch_only_keywords_that_change_nothing_and_vis_stat():
    from surf_renderer_amd import render
    scene, _, kw = load_tch_case("t2_mixed_specular_64x48")
    a = render(scene, device="cuda:0", shading="torch", **kw)
    b = render(scene, device="cuda:0", shading="torch", backface_culling=True, tiled=True, tile_size=512, **kw)
    for k in ("image", "depth", "nearest", "normal", "pos"):
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(RuntimeError, match="vis_stat"):
        render(scene, device="cuda:0", shading="torch", vis_stat=True)
    with pytest.raises(TypeError):
        render(scene, device="cuda:0", no_such_keyword=1)


def test_norm_depth_image_is_differentiable_through_depth():
    from surf_renderer_amd import render, synthetic
    scene = synthetic.splat_basic_scene(48, 40)
    pos = torch.tensor(np.asarray(scene["objects"]["disk"]["pos"], dtype=np.float32), device="cuda:0", requires_grad=True)
    scene["objects"]["disk"] = dict(scene["objects"]["disk"], pos=pos)
    res = render(scene, device="cuda:0", shading="torch", norm_depth_image_only=True)
    res["image"].sum().backward()
    assert pos.grad is not None and torch.isfinite(pos.grad).all() and pos.grad.abs().sum() > 0


def _with_torch_inputs(scene):
    n_l = np.asarray(scene["lights"]["pos"]).shape[0]
    n_m = np.asarray(scene["materials"]["albedo"]).shape[0]
    scene["lights"] = dict(scene["lights"], attenuation=np.array([[1, 0, 0]] * n_l, dtype=np.float32),
                           ambient=np.array([0.02, 0.02, 0.02], dtype=np.float32))
    scene["materials"] = dict(scene["materials"], coeffs=np.array([[0.8, 0.2, 6.0]] * n_m, dtype=np.float32))
    return scene


def test_binned_shadow_pass_equals_all_pairs_bit_for_bit():
    """The light-space tile bins only select candidates; every candidate goes through the same fp64 test, so the
    visibility bits and the re-shaded image equal the all-pairs pass exactly: fixtures' scenes, a disc cloud with the
    lights outside (views), a light inside the cloud (no usable view -> that light takes all pairs), a light 0.05 in
    front of an occluder (the near-ball rule), planes as receivers and occluders."""
    from surf_renderer_amd import synthetic
    cases = []
    for name in ("s1a_mixed_shadow_64x48", "s1b_disk_cloud_shadow_64x64_ds"):
        scene, _, kw = load_shadow_case(name)
        cases.append((scene, kw))
    cloud = _with_torch_inputs(synthetic.disk_cloud_scene(6000, 160, 128, radius=0.05, seed=3))
    cases.append((cloud, {}))
    inside = _with_torch_inputs(synthetic.disk_cloud_scene(3000, 96, 80, radius=0.06, seed=4))
    lp = np.asarray(inside["lights"]["pos"], dtype=np.float32).copy()
    lp[0] = [0.1, 0.05, 0.2, 1.0]                                   # inside the cloud
    lp[1] = [0.0, 3.0, 0.0, 1.0]                                    # close above it
    inside["lights"]["pos"] = lp
    cases.append((inside, {"double_sided": True}))
    mixed = _with_torch_inputs(synthetic.demo_scene(144, 112, with_planes=True))
    mixed["camera"]["near"] = 0.5
    # a light 0.05 in front of the first disc, on its normal: the disc is "behind the light" for rays arriving there
    disk = mixed["objects"]["disk"]
    n0 = np.asarray(disk["normal"], dtype=np.float64)[0, :3]
    p0 = np.asarray(disk["pos"], dtype=np.float64)[0, :3]
    lp = np.asarray(mixed["lights"]["pos"], dtype=np.float32).copy()
    lp[0, :3] = (p0 + 0.05 * n0 / np.linalg.norm(n0)).astype(np.float32)
    mixed["lights"]["pos"] = lp
    cases.append((mixed, {}))
    # a crowd: 1000 discs in a patch that covers a few tiles of every light's view -> those bins are full (64 slots
    # for 1500 primitives on 2048^2 light views) and the discs that do not fit go to the frame-wide list
    crowd = _with_torch_inputs(synthetic.disk_cloud_scene(1500, 128, 96, radius=0.01, seed=23))
    rng = np.random.RandomState(5)
    pos = np.asarray(crowd["objects"]["disk"]["pos"], dtype=np.float32).copy()
    pos[:1000, :2] = rng.uniform(-0.03, 0.03, size=(1000, 2)).astype(np.float32)
    pos[:1000, 2] = rng.uniform(-0.5, 0.5, size=1000).astype(np.float32)
    crowd["objects"]["disk"]["pos"] = pos
    cases.append((crowd, {"double_sided": True}))
    shadowed = 0
    for scene, kw in cases:
        (img_b, vis_b, depth), (img_a, vis_a, _) = _shadow_both_ways(scene, **kw)
        assert torch.equal(vis_b, vis_a), f"{int((vis_b != vis_a).sum())} pixels differ in visibility"
        assert torch.equal(img_b.view(torch.int32), img_a.view(torch.int32))
        n_l = np.asarray(scene["lights"]["pos"]).shape[0]
        hit = depth <= float(scene["camera"]["far"])
        shadowed += int(((vis_a[hit] & ((1 << n_l) - 1)) != (1 << n_l) - 1).sum())
    assert shadowed > 1000                                          # the cases do cast shadows


def test_shadow_pass_accepts_the_small_workspace_as_all_pairs():
    """A workspace sized by srh_workspace_bytes (no room for light views) still works: the all-pairs fallback."""
    import ctypes as C
    from surf_renderer_amd import _lib, renderer, synthetic
    scene = _with_torch_inputs(synthetic.demo_scene(64, 48, with_planes=True))
    buf = renderer.flatten_scene(scene, "cuda:0")
    cam = renderer.camera_struct(scene["camera"], "torch")
    lib = _lib.load()
    small = lib.srh_workspace_bytes(C.byref(buf.objects), 64, 48)
    big = lib.srh_shadow_workspace_bytes(C.byref(buf.objects), 64, 48, buf.lights.n_lights)
    assert 0 < small < big
    image, depth, nearest = renderer.render_buffers(buf, cam, shading="torch")
    want = renderer.shadow_pass(buf, cam, None, image.clone(), depth, nearest)
    vis = torch.empty_like(want)
    params = _lib.SrhParams(row0=0, row1=48, mode=0, tonemap_gamma=0 if buf.gamma is None else 1,
                            gamma=1.0 if buf.gamma is None else buf.gamma, shading=_lib.SHADING["torch"])
    ws = torch.empty(small, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.srh_shadow_shade(C.byref(cam), C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials),
                                    C.byref(params), ws.data_ptr(), ws.numel(), nearest.data_ptr(), depth.data_ptr(),
                                    image.data_ptr(), vis.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(vis, want)


def test_orthographic_views_in_one_call_equal_per_view_render():
    from surf_renderer_amd import render, render_views
    scene, _, kw = load_tch_case("t4_mixed_ortho_64x48")
    cams = []
    for k in range(4):
        cam = dict(scene["camera"])
        cam["eye"] = [float(0.4 * k - 0.5), 1.0 + 0.2 * k, 10.0, 1.0]
        cams.append(cam)
    batch = render_views(scene, cams, device="cuda:0", shading="torch", **kw)
    torch.cuda.synchronize()
    for i, cam in enumerate(cams):
        single = render({**scene, "camera": cam}, device="cuda:0", shading="torch", **kw)
        for k in ("image", "depth", "nearest"):
            np.testing.assert_array_equal(batch[k][i].cpu().numpy(), single[k].cpu().numpy(), err_msg=f"view {i} {k}")
    assert (batch["depth"] <= scene["camera"]["far"]).float().mean() > 0.3
