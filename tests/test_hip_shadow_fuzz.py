"""GPU: the light-space shadow pass (srh_shadow_shade with the large workspace: k_scene_bounds, k_light_frames, the
light-view bins, k_shadow_shade_binned) against the all-pairs fp64 pass, bit for bit, and against the fp64 oracle of
torch/renderer.py:291-314 -- random scenes whose lights sit where the light-view path takes its decisions
(tests/shadow_scenes.py), row slabs, 1 to 64 lights, the deterministic edges, batched views and the backward.

Against the all-pairs kernel everything is exact.  Against the oracle the visibility bits are equal outside
`shadow_scenes.undecided` (pairs that flip when the ORACLE's fragment moves by 1e-9, or that hang on a shadow ray inside
a primitive's own plane, whose hit distance is 0 / 0 for kernel, oracle and reference alike: at most 0.5 % of the hit pairs,
asserted here and, for the same seeds, in tests/test_shadow_scenes_cpu.py), and the image is within the project's
IMAGE_RTOL / IMAGE_ATOL wherever all of a pixel's bits agree."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shadow_scenes as S
from oracle import np_oracle_tch, torch_oracle

pytestmark = pytest.mark.gpu

IMAGE_RTOL, IMAGE_ATOL = 2e-6, 2e-7
UNDECIDED_CAP = 0.005


def _blocked_pairs(vis, hit, n_lights):
    """Number of (hit pixel, light) pairs whose bit is clear."""
    words = vis[hit]
    shifts = torch.arange(n_lights, device=words.device, dtype=torch.int64).view(-1, 1)
    return int((((words.view(1, -1) >> shifts) & 1) == 0).sum())


def _assert_same(tag, got, want, n_lights):
    """(image, visibility, depth) of two shadow passes over the same primary frame: identical bits."""
    (img_g, vis_g, _), (img_w, vis_w, _) = got, want
    if not torch.equal(vis_g, vis_w):
        diff = vis_g ^ vis_w
        per_light = {l: int(((diff >> l) & 1).sum()) for l in range(n_lights) if int(((diff >> l) & 1).sum())}
        raise AssertionError(f"{tag}: visibility differs on {int((diff != 0).sum())} pixels, per light {per_light}")
    a, b = img_g.view(torch.int32), img_w.view(torch.int32)                  # NaNs compared as bits
    assert torch.equal(a, b), f"{tag}: image differs on {int((a != b).any(dim=-1).sum())} pixels"


def _fuzz_cases():
    """(index, scene, keywords) of the fuzz: the scenes of shadow_scenes.fuzz_scenes (the stream the CPU test counts
    the structural cases of), double_sided / use_quartic from a stream of their own, one scene in three orthographic."""
    rng = np.random.RandomState(S.FUZZ_SEED + 1)
    for i, scene in enumerate(S.fuzz_scenes(S.FUZZ_SEED, S.FUZZ_COUNT)):
        if i % 3 == 2:
            scene["camera"]["proj_type"] = "ortho"
        yield i, scene, {"double_sided": bool(rng.randint(2)), "use_quartic": bool(rng.randint(2))}


def test_fuzz_binned_shadow_equals_all_pairs():
    """120 random scenes (fuzz_scenes(FUZZ_SEED): rebuild scene i from the seed to reproduce a failure): visibility
    words and re-shaded image of the light-view pass equal the all-pairs pass exactly.  About 1.2 s on an MI355X:
    3.2 M hit (pixel, light) pairs, 31 % of them blocked."""
    pairs = blocked = 0
    for i, scene, kw in _fuzz_cases():
        n_l = len(scene["lights"]["pos"])
        binned, exact = S.shadow_both_ways(scene, **kw)
        _assert_same(f"scene {i} ({n_l} lights, {scene['camera'].get('proj_type', 'perspective')}, {kw})", binned, exact, n_l)
        hit = exact[2] <= float(scene["camera"]["far"])
        pairs += int(hit.sum()) * n_l
        blocked += _blocked_pairs(exact[1], hit, n_l)
    print(f"shadow fuzz: {pairs} hit pairs, {blocked / pairs:.2%} blocked")
    assert blocked > 0.10 * pairs                                            # the set does cast shadows


def test_shadow_row_slabs():
    """Every seventh scene of the fuzz (18 scenes, all structural cases among them): the shadow pass over a row slab,
    rendered with the same rows, equals those rows of the full frame -- both kernels.  First rows that are no multiple
    of 4 (the workgroup's rows) or 16 (a tile), one-row slabs."""
    rng = np.random.RandomState(S.FUZZ_SEED + 2)
    firsts, heights = [], []
    for i, scene, kw in _fuzz_cases():
        if i % 7:
            continue
        n_l, H = len(scene["lights"]["pos"]), scene["camera"]["viewport"][3]
        r0 = int(rng.randint(0, H - 1)) | (1 if len(firsts) % 2 else 0)
        r0 = min(r0, H - 1)
        r1 = r0 + 1 if len(firsts) % 3 == 0 else int(rng.randint(r0 + 1, H + 1))
        firsts.append(r0)
        heights.append(r1 - r0)
        full = S.shadow_both_ways(scene, **kw)
        part = S.shadow_both_ways(scene, rows=(r0, r1), **kw)
        for name, f, p in zip(("binned", "all pairs"), full, part):
            _assert_same(f"scene {i} rows {r0}:{r1} {name}", p, tuple(t[r0:r1] for t in f), n_l)
    assert len(firsts) >= 18 and 1 in heights and max(heights) > 16
    assert any(r % 4 for r in firsts) and any(r % 16 for r in firsts)


@functools.lru_cache(maxsize=None)
def _ladder_oracle():
    """The oracle's frame of the 64-light ladder scene with its undecided mask, computed once.  A light's visibility
    does not depend on the other lights, so the scene truncated to L lights has the first L rows of it."""
    sc = S.oracle_input(S.ladder_scene())
    res = np_oracle_tch.render(sc, shadow=True)
    return res, S.undecided(sc, res)


def _compare_with_oracle(tag, sc, want, und, vis_words, image):
    """Visibility words and image of the device against the oracle's frame `want` of scene `sc` outside `und`."""
    n_l = want["visibility"].shape[0]
    hit = want["depth"] <= sc["camera"]["far"]
    got = S.unpack_bits(vis_words, n_l)
    differ = (got != want["visibility"]) & hit[None] & ~und
    assert not differ.any(), f"{tag}: visibility differs from the oracle on {int(differ.sum())} decided pairs, " \
                             f"lights {sorted(set(np.nonzero(differ)[0]))}"
    same = ((got == want["visibility"]) | ~hit[None]).all(axis=0)
    np.testing.assert_allclose(image[same], want["image"][same], rtol=IMAGE_RTOL, atol=IMAGE_ATOL, err_msg=tag)
    return int(hit.sum()) * n_l, int(und.sum())


@pytest.mark.parametrize("n_lights", [1, 31, 32, 33, 63, 64])
def test_light_count_ladder(n_lights):
    """The ladder scene with its first L lights: bits 31, 32 and 63 of the uint64 word, the sign bit of the int64 tensor
    the Python layer hands out, up to 64 workspace slices."""
    from surf_renderer_amd import _lib, render, renderer
    scene = S.ladder_scene(n_lights)
    binned, exact = S.shadow_both_ways(scene)
    _assert_same(f"{n_lights} lights", binned, exact, n_lights)
    image, vis, depth = binned
    assert vis.dtype == torch.int64
    words = vis.cpu().numpy().view(np.uint64)
    hit = depth.cpu().numpy() <= scene["camera"]["far"]
    assert hit.any() and (~hit).any()
    if n_lights < 64:
        assert not (words[hit] >> np.uint64(n_lights)).any()                 # no bit at or above L on a hit pixel
    assert (words[~hit] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()               # background: every bit set
    on_device = torch.as_tensor(hit, device=vis.device)
    assert (vis[~on_device] == -1).all()
    if n_lights == 64:
        assert (vis[on_device] < 0).any() and (vis[on_device] >= 0).any()    # light 63 seen here, blocked there
    full, und = _ladder_oracle()
    sc = S.oracle_input(scene)
    want = dict(full, visibility=full["visibility"][:n_lights])
    want["image"] = np_oracle_tch.shade(sc, full, want["visibility"].reshape(n_lights, -1))
    _compare_with_oracle(f"{n_lights} lights", sc, want, und[:n_lights], vis.cpu().numpy(), image.cpu().numpy())
    res = render(scene, device="cuda:0", shading="torch", shadow=True)
    assert torch.equal(res["light_visibility"], vis) and torch.equal(res["image"], image)
    # the workspace: 64 lights are accepted, 65 refused with SRH_E_RANGE
    lib = _lib.load()
    buf = renderer.flatten_scene(scene, "cuda:0")
    W, H = scene["camera"]["viewport"][2:]
    need = lib.srh_shadow_workspace_bytes(C.byref(buf.objects), W, H, n_lights)
    most = lib.srh_shadow_workspace_bytes(C.byref(buf.objects), W, H, 64)
    assert 0 < need <= most and (need < most) == (n_lights < 64)
    assert lib.srh_shadow_workspace_bytes(C.byref(buf.objects), W, H, 65) == 0 and b"0..64" in lib.srh_last_error()
    if n_lights == 64:
        print(f"shadow workspace for 64 lights, {S.primitive_count(scene)} primitives, {W} x {H}: {most} bytes")
        cam = renderer.camera_struct(scene["camera"], "torch")
        img2, depth2, nearest2 = renderer.render_buffers(buf, cam, shading="torch")
        ws = buf.ensure_shadow_workspace(W, H)
        assert ws.numel() >= most
        too_many = _lib.SrhLights.from_buffer_copy(buf.lights)
        too_many.n_lights = 65
        params = _lib.SrhParams(row0=0, row1=H, mode=0, tonemap_gamma=0 if buf.gamma is None else 1,
                                gamma=1.0 if buf.gamma is None else buf.gamma, shading=_lib.SHADING["torch"])
        out = torch.empty_like(vis)
        rc = lib.srh_shadow_shade(C.byref(cam), C.byref(buf.objects), C.byref(too_many), C.byref(buf.materials),
                                  C.byref(params), ws.data_ptr(), ws.numel(), nearest2.data_ptr(), depth2.data_ptr(),
                                  img2.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == -2 and b"0..64" in lib.srh_last_error()                  # SRH_E_RANGE


def test_deterministic_edges():
    """The builders of tests/shadow_scenes.py: both kernels exactly, the oracle outside `undecided`, and the outcome each
    is named for at the centre pixel."""
    pairs = flips = 0
    for name, (scene, (light, outcome)) in S.deterministic_scenes().items():
        n_l = len(scene["lights"]["pos"])
        binned, exact = S.shadow_both_ways(scene)
        _assert_same(name, binned, exact, n_l)
        sc = S.oracle_input(scene)
        want = np_oracle_tch.render(sc, shadow=True)
        und = S.undecided(sc, want)
        p, f = _compare_with_oracle(name, sc, want, und, binned[1].cpu().numpy(), binned[0].cpu().numpy())
        pairs, flips = pairs + p, flips + f
        r, c = S.centre_pixel(scene)
        assert bool((int(binned[1][r, c]) >> light) & 1) == (outcome == "lit"), f"{name}: expected {outcome}"
    assert flips <= UNDECIDED_CAP * pairs


def test_fuzz_shadow_against_the_oracle():
    """15 small random scenes in both projections (30 frames) through render(shading='torch', shadow=True): 62 412 hit
    pairs, 0.11 % of them undecided, 36 % shadowed.  About 3.4 s, nearly all of it the numpy oracle, which is why the
    frames stay within 32 x 24 pixels and 400 primitives (16 x 12 with more than 8 lights)."""
    from surf_renderer_amd import render
    rng = np.random.RandomState(S.ORACLE_SEED + 1)
    pairs = flips = 0
    for i, scene in enumerate(S.oracle_scenes(S.ORACLE_SEED, S.ORACLE_COUNT)):
        for proj in ("perspective", "ortho"):
            scene["camera"]["proj_type"] = proj
            kw = {"double_sided": bool(rng.randint(2)), "use_quartic": bool(rng.randint(2))}
            sc = S.oracle_input(scene)
            want = np_oracle_tch.render(sc, shadow=True, **kw)
            und = S.undecided(sc, want)
            res = render(scene, device="cuda:0", shading="torch", shadow=True, **kw)
            tag = f"scene {i} ({proj}, {kw})"
            same = res["nearest"].cpu().numpy() == want["nearest"]
            assert same.all(), f"{tag}: nearest differs on {(~same).sum()} pixels"
            p, f = _compare_with_oracle(tag, sc, want, und, res["light_visibility"].cpu().numpy(),
                                        res["image"].cpu().numpy())
            pairs, flips = pairs + p, flips + f
    print(f"oracle fuzz: {pairs} hit pairs, {flips / pairs:.4%} undecided")
    assert flips <= UNDECIDED_CAP * pairs


def _many_light_scene(n_lights=34):
    """The ladder's cloud over its plane with the first 34 lights of the ring: bits 32 and 33 in use."""
    return S.ladder_scene(n_lights)


def test_views_and_backward_use_the_high_bits():
    from surf_renderer_amd import render, render_views
    scene = _many_light_scene()
    n_l = len(scene["lights"]["pos"])
    # three cameras, every view with its own 34 light positions
    rng = np.random.RandomState(34)
    cams, overrides, scenes = [], [], []
    for v in range(3):
        cams.append(dict(scene["camera"], eye=[0.5 * v - 0.4, -1.0 - 0.3 * v, 6.0, 1.0], far=50.0))
        lpos = np.array(scene["lights"]["pos"], dtype=np.float32, copy=True)
        lpos[:, :3] += rng.uniform(-0.3, 0.3, (n_l, 3)).astype(np.float32)
        overrides.append({"lights.pos": lpos})
        scenes.append(dict(scene, camera=cams[v], lights=dict(scene["lights"], pos=lpos)))
    got = render_views(scene, cams, device="cuda:0", overrides=overrides, shading="torch", shadow=True)
    high = 0
    for v in range(3):
        one = render(scenes[v], device="cuda:0", shading="torch", shadow=True)
        assert torch.equal(got["visibility"][v], one["light_visibility"]), f"view {v}: visibility"
        assert torch.equal(got["image"][v], one["image"]), f"view {v}: image"
        hit = one["depth"] <= 50.0
        high += int((((one["light_visibility"][hit] >> 32) & 3) != 3).sum())
    assert high > 30                                                         # lights 32 and 33 are blocked somewhere

    # one backward: the oracle is fed the kernel's own bits, so it sees the same decisions and the tolerance is the
    # unshadowed one of tests/test_hip_backward.py
    from grad_cases import TCH_KEYS, assert_grads_close, gpu_leaf_scene, leaf_grads
    sc = S.oracle_input(scene)
    ref = np_oracle_tch.render(sc)
    H, W = ref["depth"].shape
    g_img = np.random.RandomState(9).uniform(-1, 1, size=(H, W, 3))
    words = render(scene, device="cuda:0", shading="torch", shadow=True)["light_visibility"].cpu().numpy()
    V = S.unpack_bits(words, n_l)
    leaf_scene, leaves = gpu_leaf_scene(sc, TCH_KEYS)
    res = render(leaf_scene, device="cuda:0", shading="torch", shadow=True)
    assert np.array_equal(res["nearest"].cpu().numpy(), ref["nearest"])
    torch.sum(res["image"] * torch.as_tensor(g_img, dtype=torch.float32, device="cuda:0")).backward()
    want = torch_oracle.gradients_tch(sc, g_img, None, ref=ref, visibility=V)
    plain = torch_oracle.gradients_tch(sc, g_img, None, ref=ref)
    assert_grads_close(leaf_grads(leaves), want, 2e-4, "34 lights", keys=leaves)
    # the shadows on lights >= 32 reach the backward: they move those lights' position gradients by more than that
    w, p = want["lights.pos"].reshape(n_l, -1)[32:], plain["lights.pos"].reshape(n_l, -1)[32:]
    tol = 2e-4 * max(np.abs(want["lights.pos"]).max(), 1e-9) + 1e-6
    assert (np.abs(w - p).max(axis=1) > tol).all(), np.abs(w - p).max(axis=1)
