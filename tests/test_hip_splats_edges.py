"""GPU: the splat kernels (csrc/srh_splat.h) on the scenes of tests/splat_edge_scenes.py -- clamped and origin splats,
sides of length 1 and 2, K = 4 and 8, partial waves and workgroups, lights with w != 1, shininess 0 and 1, a clipping
relu -- against the fp64 oracle; the batch forms at the partial-wave sizes; and what only the C ABI can ask for (NULL
optional arrays, out-of-range indices, gradient buffers that hold garbage before the call).
tests/test_splat_edge_scenes_cpu.py shows that each scene reaches the branch it is named for.

Tolerances are those tests/test_hip_splats.py states and derives, unchanged: outputs rtol 2e-6, atol 2e-7 max(|want|, 1);
gradients |got - want| <= 2e-4 max|want| + 1e-6 per leaf.  At K = 8 a light_vis gradient is a chain of 64 fp32 additions:
64 * 2^-24 = 4e-6 of the running sum, well inside 2e-4."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from splat_edge_scenes import CASES, base_scene, given_normals, reference, surface
from test_hip_splats import DEV, _compare_grads, _compare_outputs, _gpu_scene, _hip

pytestmark = pytest.mark.gpu

OUTPUTS = ("image", "depth", "pos", "normal")


def _z(scene):
    pos = np.asarray(scene["objects"]["disk"]["pos"])
    return pos if pos.ndim == 1 else pos[:, 2]


# ---- a. every case against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_edge_case_matches_the_oracle(name):
    scene, kw, notes, up, want, want_g = reference(name)
    got, got_g = _hip(scene, {k: v.copy() for k, v in up.items()}, **kw)
    _compare_outputs(got, want, name)
    assert set(got_g) == set(want_g)
    if name == "clamped_given_k2":
        # the oracle's d loss / d normal is NaN on the clamped rows (sqrt'(0) * 0 through the depth of an origin splat);
        # the kernels give the depth no gradient there, so theirs is finite
        live = _z(scene) < 0
        assert np.isfinite(got_g["disk.normal"]).all()
        assert np.all(got_g["disk.pos"][~live] == 0)
        full = {k: v for k, v in want_g.items() if k != "disk.normal"}
        _compare_grads(got_g, full, name)
        _compare_grads({"disk.normal": got_g["disk.normal"][live]}, {"disk.normal": want_g["disk.normal"][live]}, name)
    else:
        _compare_grads(got_g, want_g, name)
    if name == "clamped_est":
        assert np.all(got_g["disk.pos"][_z(scene) >= 0] == 0)
        assert np.all(got["depth"].reshape(-1)[_z(scene) >= 0] == 0)


def test_pos_with_three_columns_reads_and_differentiates_column_two_only():
    from surf_renderer_amd import render_splats_along_ray
    scene, kw, notes, up, want, want_g = reference("zpos_cols3")
    got, got_g = _hip(scene, {k: v.copy() for k, v in up.items()}, **kw)
    assert got_g["disk.pos"].shape == (30, 3)
    assert np.all(got_g["disk.pos"][:, :2] == 0) and np.all(got_g["disk.pos"][:, 2] != 0)

    def outputs(pos):
        sc = copy.deepcopy(scene)
        sc["objects"]["disk"]["pos"] = pos
        sc, _ = _gpu_scene(sc)
        with torch.no_grad():
            res = render_splats_along_ray(sc, **kw)
        torch.cuda.synchronize()
        return {k: res[k].cpu().numpy() for k in OUTPUTS}

    pos = scene["objects"]["disk"]["pos"]
    nan_xy = pos.copy()
    nan_xy[:, :2] = np.nan
    three, one, poisoned = outputs(pos), outputs(np.ascontiguousarray(pos[:, 2])), outputs(nan_xy)
    for k in OUTPUTS:
        assert np.array_equal(three[k], got[k].astype(np.float32).reshape(three[k].shape)), k
        assert np.array_equal(three[k], one[k]), k
        assert np.array_equal(three[k], poisoned[k]), k       # bit for bit, and no NaN reaches an output


# ---- b. batch forms at the partial-wave sizes ------------------------------------------------------------------------
def _batch_scene(H, W, given, eye_per_view, B=3):
    """B views: pos (and the given normals) per view, lights.pos shared, camera.eye shared or per view."""
    scene = base_scene(H, W, seed=60, given=False)
    scene["objects"]["disk"]["pos"] = np.stack([surface(H, W, 61 + b) for b in range(B)])
    if given:
        scene["objects"]["disk"]["normal"] = np.stack([given_normals(H, W, 71 + b) for b in range(B)])
    if eye_per_view:
        scene["camera"]["eye"] = np.array([[0.8 + 0.3 * b, 1.5 - 0.2 * b, 6.0, 1.0] for b in range(B)], np.float32)
    return scene


def _view(scene, b):
    sc = copy.deepcopy(scene)
    d = sc["objects"]["disk"]
    d["pos"] = d["pos"][b]
    if "normal" in d:
        d["normal"] = d["normal"][b]
    if np.ndim(sc["camera"]["eye"]) == 2:
        sc["camera"]["eye"] = sc["camera"]["eye"][b]
    return sc


def _loss(res, up):
    return sum((res[k] * torch.as_tensor(up[k], device=DEV)).sum() for k in OUTPUTS)


@pytest.mark.parametrize("eye_per_view", [False, True])
@pytest.mark.parametrize("H,W,given,K", [(2, 2, False, 1), (5, 13, True, 2)])
def test_batch_with_shared_lights_equals_single_calls(H, W, given, K, eye_per_view):
    from surf_renderer_amd import render_splats_along_ray, render_splats_along_ray_batch
    B = 3
    scene = _batch_scene(H, W, given, eye_per_view)
    assert np.ndim(scene["lights"]["pos"]) == 2 and np.ndim(scene["camera"]["eye"]) == 1 + eye_per_view
    rng = np.random.RandomState(12)
    up = {k: rng.uniform(-1, 1, (B, K * H, K * W) + ((3,) if k != "depth" else ())).astype(np.float32) for k in OUTPUTS}
    sc, leaves = _gpu_scene(scene)
    res = render_splats_along_ray_batch(sc, samples=K)
    _loss(res, up).backward()
    torch.cuda.synchronize()
    assert tuple(leaves["lights.pos"].grad.shape) == (2, 4)
    want_lights = np.zeros((2, 4))
    for b in range(B):
        one, one_leaves = _gpu_scene(_view(scene, b))
        r1 = render_splats_along_ray(one, samples=K)
        _loss(r1, {k: v[b] for k, v in up.items()}).backward()
        torch.cuda.synchronize()
        for k in OUTPUTS:
            assert torch.equal(res[k][b], r1[k]), (b, k)
        assert torch.equal(leaves["disk.pos"].grad[b], one_leaves["disk.pos"].grad), b
        if given:
            assert torch.equal(leaves["disk.normal"].grad[b], one_leaves["disk.normal"].grad), b
        want_lights += one_leaves["lights.pos"].grad.cpu().numpy().astype(np.float64)
    # the views' fp32 atomic sums land in one array: equal up to the order of the additions
    _compare_grads({"lights.pos": leaves["lights.pos"].grad.cpu().numpy().astype(np.float64)},
                   {"lights.pos": want_lights}, f"{H}x{W} shared lights", tol=2e-5)
    assert np.abs(want_lights[:, 3]).min() > 0


# ---- c. the C ABI with torch device buffers --------------------------------------------------------------------------
ABI_H, ABI_W, ABI_K = 5, 13, 2


def _abi_scene():
    return base_scene(ABI_H, ABI_W, seed=80, given=True, light_vis=True)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype).contiguous()


class _AbiCall:
    """One view of `scene` through srh_splat_fwd / srh_splat_bwd.  `arrays` replaces optional inputs: attenuation,
    ambient, coeffs, material_idx (None = a NULL pointer) and color_idx."""

    def __init__(self, scene, given=True, pos_cols=1, shade=1, K=ABI_K, **arrays):
        from surf_renderer_amd import _lib
        self.lib = _lib.load()
        self._lib = _lib
        cam, disk, lights = scene["camera"], scene["objects"]["disk"], scene["lights"]
        self.H, self.W, self.K, self.N = ABI_H, ABI_W, K, ABI_H * ABI_W
        self.L = lights["pos"].shape[0]
        z = np.asarray(disk["pos"], np.float32)
        if pos_cols == 3:
            z = np.concatenate([np.random.RandomState(81).uniform(-9, 9, (z.size, 2)).astype(np.float32), z[:, None]], 1)
        opt = {"attenuation": lights["attenuation"], "ambient": lights["ambient"],
               "coeffs": scene["materials"]["coeffs"], "material_idx": disk["material_idx"],
               "color_idx": lights["color_idx"]}
        opt.update(arrays)
        t = self.t = {
            "pos": _dev(z), "normal": _dev(disk["normal"]) if given else None, "light_vis": _dev(disk["light_vis"]),
            "eye": _dev(np.asarray(cam["eye"])[:3]), "lights_pos": _dev(lights["pos"]),
            "color_idx": _dev(opt["color_idx"], torch.int32), "colors": _dev(scene["colors"]),
            "attenuation": _dev(opt["attenuation"]), "ambient": _dev(opt["ambient"]),
            "material_idx": _dev(opt["material_idx"], torch.int32), "albedo": _dev(scene["materials"]["albedo"]),
            "coeffs": _dev(opt["coeffs"])}
        ptr = {k: (v.data_ptr() if v is not None else None) for k, v in t.items()}
        self.p = _lib.SrhSplatParams(n_views=1, width=self.W, height=self.H, samples=K, pos_cols=pos_cols, use_quartic=0,
                                     shade=shade, fovy=float(cam["fovy"]), focal_length=float(cam["focal_length"]))
        self.p.at[:] = [float(v) for v in np.asarray(cam["at"])[:3]]
        self.p.up[:] = [float(v) for v in np.asarray(cam["up"])[:3]]
        self.inp = _lib.SrhSplatInputs(pos=ptr["pos"], pos_view_stride=self.N * pos_cols, normal=ptr["normal"],
                                       normal_view_stride=0, light_vis=ptr["light_vis"], light_vis_view_stride=0,
                                       eye=ptr["eye"], eye_view_stride=0, lights_pos_view_stride=0,
                                       material_idx=ptr["material_idx"])
        self.li = _lib.SrhLights(n_lights=self.L, n_colors=scene["colors"].shape[0], pos=ptr["lights_pos"],
                                 color_idx=ptr["color_idx"], colors=ptr["colors"], attenuation=ptr["attenuation"],
                                 ambient=ptr["ambient"])
        self.ma = _lib.SrhMaterials(n_materials=scene["materials"]["albedo"].shape[0], albedo=ptr["albedo"],
                                    coeffs=ptr["coeffs"])
        self.given, self.pos_cols, self.shade = given, pos_cols, shade

    def _args(self):
        return C.byref(self.p), C.byref(self.inp), C.byref(self.li), C.byref(self.ma)

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def fwd(self, fill=float("nan")):
        KH, KW = self.K * self.H, self.K * self.W
        out = {k: torch.full((KH, KW) + ((3,) if k != "depth" else ()), fill, dtype=torch.float32, device=DEV)
               for k in OUTPUTS if k != "image" or self.shade}
        image = out["image"].data_ptr() if self.shade else None
        self._lib.check(self.lib.srh_splat_fwd(*self._args(), image, out["depth"].data_ptr(), out["pos"].data_ptr(),
                                               out["normal"].data_ptr(), self._stream()))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def bwd(self, ups, fill=float("nan"), scene_grads=()):
        """Written gradients (pos, normal for given normals, light_vis when shading) from buffers pre-filled with
        `fill`, plus the zero-filled atomic ones named in `scene_grads`.  `ups`: upstream arrays by output name."""
        g = {"pos": torch.full((self.N, self.pos_cols), fill, dtype=torch.float32, device=DEV)}
        if self.given:
            g["normal"] = torch.full((self.N, 3), fill, dtype=torch.float32, device=DEV)
        if self.shade:
            g["light_vis"] = torch.full((self.L, self.N), fill, dtype=torch.float32, device=DEV)
        for k in scene_grads:
            g[k] = torch.zeros_like(self.t[k])
        u = {k: _dev(v) for k, v in ups.items()}
        ws_bytes = self.lib.srh_splat_workspace_bytes(C.byref(self.p), C.byref(self.inp))
        assert ws_bytes == (0 if self.given else self.N * 9 * 8)
        ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=DEV)
        sg = self._lib.SrhSplatGrads(**{k: v.data_ptr() for k, v in g.items()})
        self._lib.check(self.lib.srh_splat_bwd(*self._args(), ws.data_ptr(), ws.numel(),
                                               *[u[k].data_ptr() if k in u else None for k in OUTPUTS],
                                               C.byref(sg), self._stream()))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in g.items()}


def _abi_upstream(K=ABI_K):
    rng = np.random.RandomState(13)
    return {k: rng.uniform(-1, 1, (K * ABI_H, K * ABI_W) + ((3,) if k != "depth" else ())).astype(np.float32)
            for k in OUTPUTS}


def _assert_identical(a, b, tag):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (tag, k)


@pytest.mark.parametrize("given", [True, False])
def test_abi_null_optional_arrays_equal_their_documented_defaults(given):
    scene = _abi_scene()
    L, M, N = 2, 2, ABI_H * ABI_W
    explicit = {"attenuation": np.tile(np.array([1.0, 0.0, 0.0], np.float32), (L, 1)), "ambient": np.zeros(3, np.float32),
                "coeffs": np.tile(np.array([1.0, 0.0, 0.0], np.float32), (M, 1)), "material_idx": np.zeros(N, np.int64)}
    null = {k: None for k in explicit}
    up = _abi_upstream()
    a, b = _AbiCall(scene, given=given, **explicit), _AbiCall(scene, given=given, **null)
    fa, fb = a.fwd(), b.fwd()
    _assert_identical(fa, fb, "forward")
    assert all(np.isfinite(v).all() for v in fa.values()) and np.abs(fa["image"]).max() > 0.1
    ga, gb = a.bwd(up, scene_grads=("lights_pos", "colors", "albedo")), b.bwd(up, scene_grads=("lights_pos", "colors", "albedo"))
    _assert_identical({k: ga[k] for k in ("pos", "normal", "light_vis") if k in ga},
                      {k: gb[k] for k in ("pos", "normal", "light_vis") if k in gb}, "written gradients")
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in ga.values())
    # the atomic sums agree up to the order of their additions
    _compare_grads({k: gb[k].astype(np.float64) for k in ("lights_pos", "colors", "albedo")},
                   {k: ga[k].astype(np.float64) for k in ("lights_pos", "colors", "albedo")}, "NULL", tol=2e-5)
    # and the defaults are not those of the scene: the explicit call differs from the scene's own arrays
    assert not np.array_equal(_AbiCall(scene, given=given).fwd()["image"], fa["image"])


def test_abi_material_and_colour_indices_are_clamped():
    scene = _abi_scene()
    N = ABI_H * ABI_W
    mat = np.random.RandomState(14).choice([-3, 0, 1, 7], N)
    mat[:4] = [-3, 0, 1, 7]
    cidx = np.array([-1, 5])
    up = _abi_upstream()
    grads = ("colors", "albedo", "coeffs")
    raw = _AbiCall(scene, material_idx=mat, color_idx=cidx)
    clamped = _AbiCall(scene, material_idx=np.clip(mat, 0, 1), color_idx=np.clip(cidx, 0, 2))
    fr, fc = raw.fwd(), clamped.fwd()
    _assert_identical(fr, fc, "forward")
    gr, gc = raw.bwd(up, scene_grads=grads), clamped.bwd(up, scene_grads=grads)
    _assert_identical({k: gr[k] for k in ("pos", "normal", "light_vis")}, {k: gc[k] for k in ("pos", "normal", "light_vis")},
                      "written gradients")
    _compare_grads({k: gr[k].astype(np.float64) for k in grads}, {k: gc[k].astype(np.float64) for k in grads},
                   "clamped indices", tol=2e-5)
    assert np.all(gr["colors"][1] == 0) and np.abs(gr["colors"][[0, 2]]).min() > 0     # rows 0 and 2 are the lights'
    assert np.abs(gr["albedo"]).min() > 0 and np.abs(gr["coeffs"]).min() > 0
    # the clamp matters: the in-range scene indices give another picture
    assert not np.array_equal(_AbiCall(scene).fwd()["image"], fr["image"])


@pytest.mark.parametrize("only", ["image", "depth"])
@pytest.mark.parametrize("pos_cols", [1, 3])
@pytest.mark.parametrize("given", [True, False])
def test_abi_backward_overwrites_every_element_of_the_written_gradients(given, pos_cols, only):
    """splats.py hands srh_splat_bwd torch.empty buffers for pos, normal and light_vis: whatever they held must be gone
    after the call, also when a single output has an upstream gradient."""
    call = _AbiCall(_abi_scene(), given=given, pos_cols=pos_cols)
    up = {only: _abi_upstream()[only]}
    poisoned, clean = call.bwd(up, fill=float("nan")), call.bwd(up, fill=0.0)
    assert set(poisoned) == {"pos", "light_vis"} | ({"normal"} if given else set())
    for k, v in poisoned.items():
        assert not np.isnan(v).any(), k
    _assert_identical(poisoned, clean, f"{only} alone")
    assert poisoned["pos"].shape == (ABI_H * ABI_W, pos_cols) and np.all(poisoned["pos"][:, :pos_cols - 1] == 0)
    assert np.abs(poisoned["pos"][:, -1]).min() > 0
    if only == "depth":                                       # the depth does not depend on light_vis: written zeros
        assert np.all(poisoned["light_vis"] == 0)
    else:
        assert np.abs(poisoned["light_vis"]).max() > 0


@pytest.mark.parametrize("shade", [1, 0])
@pytest.mark.parametrize("given", [True, False])
def test_abi_forward_overwrites_every_output_element(given, shade):
    call = _AbiCall(_abi_scene(), given=given, shade=shade)
    poisoned, clean = call.fwd(fill=float("nan")), call.fwd(fill=0.0)
    assert set(poisoned) == ({"image"} if shade else set()) | {"depth", "pos", "normal"}
    for k, v in poisoned.items():
        assert not np.isnan(v).any(), k
    _assert_identical(poisoned, clean, f"shade = {shade}")
    assert poisoned["depth"].shape == (ABI_K * ABI_H, ABI_K * ABI_W) and poisoned["depth"].min() > 3
