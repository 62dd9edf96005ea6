"""GPU: render_splats_NDC / render_splats_NDC_batch on the edge inputs of tests/splats_ndc_edge_cases.py against the fp64
restatement tests/splats_ndc_oracle.py, which tests/test_splats_ndc_edge_cases_cpu.py ties to the reference on these very
cases (tests/golden/splats_ndc/sn2_*.npz) and which it shows to reach the branches the cases are named for: the
wave-uniform material reduction of k_splat_ndc_bwd with m0 != 0, with dead lanes, next to a divergent wave and in a batch;
sgn == 0, relu(0) and 0 ** 0 on zero normals.  And through the C ABI at 5 x 13: NULL optional arrays and the clamps on
material_idx / color_idx.

Tolerances are the ones tests/test_hip_splats_ndc.py states, unchanged: outputs and written gradients rtol 2e-6, atol
2e-7 max(max|want|, 1); the fp32 atomic sums |got - want| <= 2e-4 max|want| + 1e-6; against the float32 reference
outputs atol 2e-5 max(max|want|, 1) and gradients atol 3e-3 max(max|want|, 1e-6).  No element is excluded: at a kink the
restatement, the reference and the kernels take the same side (sign(0) = 0, relu'(0) = 0, 0 ** 0 = 1)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import splats_ndc_edge_cases as edges
import splats_ndc_oracle as oracle
from conftest import GOLDEN_DIR
from test_hip_splats_ndc import DEV, _atomic_close, _close, _hip

pytestmark = pytest.mark.gpu

DIR = os.path.join(GOLDEN_DIR, "splats_ndc")


@pytest.mark.parametrize("name", edges.NAMES)
def test_forward_and_gradients_match_the_restatement_and_the_reference(name):
    c = edges.case(name)
    got, got_g = _hip(c["scene"], c["upstream"], **c["kwargs"])
    want, want_g = edges.expected(name)
    for k in oracle.OUTPUTS:
        _close(got[k], want[k], f"{name} {k}")
    for k in oracle.LEAVES:
        print(f"{name} d/d {k}: max err {np.abs(got_g[k] - want_g[k]).max():.3g}, max|want| {np.abs(want_g[k]).max():.3g}")
        (_close if k in oracle.WRITTEN else _atomic_close)(got_g[k], want_g[k], f"{name} d/d {k}")
    npz = np.load(os.path.join(DIR, f"sn2_{name}.npz"), allow_pickle=False)           # the float32 reference itself
    for k in oracle.OUTPUTS:
        w = npz["ref32/" + k].astype(np.float64)
        np.testing.assert_allclose(got[k], w, rtol=0, atol=2e-5 * max(np.abs(w).max(), 1.0), err_msg=f"{name} ref32 {k}")
    for k in oracle.LEAVES:
        w = npz["grad32/" + k].astype(np.float64)
        np.testing.assert_allclose(got_g[k], w, rtol=0, atol=3e-3 * max(np.abs(w).max(), 1e-6),
                                   err_msg=f"{name} grad32 {k}")
    if c["at_kink"]:
        at = list(c["at_kink"])
        assert np.all(np.isfinite(got_g["disk.normal"][at])) and np.all(np.isfinite(got_g["disk.pos"][at]))
        # the shading sends a zero normal exactly nothing (both dots vanish, the specular one to second order): what is
        # left is the `normal` output's own upstream gradient
        want_n = c["upstream"]["normal"].reshape(-1, 3).astype(np.float64)[at]
        assert np.array_equal(got_g["disk.normal"][at], want_n)


def test_the_uniform_batch_equals_the_loop_over_its_views():
    c = edges.case("uniform_b3")
    scene, up, kw = c["scene"], c["upstream"], c["kwargs"]
    got, got_g = _hip(scene, up, **kw)
    loop = [_hip(oracle.view(scene, b), {k: g[b] for k, g in up.items()}, **kw) for b in range(3)]
    for k in oracle.OUTPUTS:
        np.testing.assert_array_equal(got[k], np.stack([r[0][k] for r in loop]), err_msg=k)
    for k in oracle.LEAVES:
        if k in oracle.WRITTEN:                            # written by the lane that owns the splat: bit-identical
            np.testing.assert_array_equal(got_g[k], np.stack([r[1][k] for r in loop]), err_msg=k)
        elif k == "lights.pos":
            _atomic_close(got_g[k], np.stack([r[1][k] for r in loop]), k)
        else:                                              # a shared leaf: the sum over the views
            _atomic_close(got_g[k], sum(r[1][k] for r in loop), k)


# ---- the C ABI with torch device buffers, 5 x 13 ---------------------------------------------------------------------
def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype).contiguous()


class _AbiCall:
    """The scene of edges.abi_scene() through srh_splat_ndc_fwd / srh_splat_ndc_bwd.  `arrays` replaces optional inputs:
    attenuation, ambient, coeffs, material_idx (None = a NULL pointer) and color_idx."""
    SUMS = ("lights_pos", "colors", "attenuation", "ambient", "albedo", "coeffs")

    def __init__(self, **arrays):
        from surf_renderer_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        c = edges.abi_scene()
        scene = c["scene"]
        cam, disk, lights = scene["camera"], scene["objects"]["disk"], scene["lights"]
        self.W, self.H = oracle.grid(cam)
        self.N = self.W * self.H
        opt = {"attenuation": lights["attenuation"], "ambient": lights["ambient"], "coeffs": scene["materials"]["coeffs"],
               "material_idx": disk["material_idx"], "color_idx": lights["color_idx"]}
        opt.update(arrays)
        t = self.t = {"pos": _dev(disk["pos"]), "normal": _dev(disk["normal"][:, :3]), "eye": _dev(cam["eye"][:3]),
                      "lights_pos": _dev(lights["pos"]), "color_idx": _dev(opt["color_idx"], torch.int32),
                      "colors": _dev(scene["colors"]), "attenuation": _dev(opt["attenuation"]),
                      "ambient": _dev(opt["ambient"]), "material_idx": _dev(opt["material_idx"], torch.int32),
                      "albedo": _dev(scene["materials"]["albedo"]), "coeffs": _dev(opt["coeffs"])}
        ptr = {k: (v.data_ptr() if v is not None else None) for k, v in t.items()}
        self.p = _lib.SrhSplatNdcParams(n_views=1, width=self.W, height=self.H, pos_cols=3, shade=1, fovy=cam["fovy"],
                                        near_clip=cam["near"], far_clip=cam["far"])
        self.p.at[:] = [float(v) for v in cam["at"][:3]]
        self.p.up[:] = [float(v) for v in cam["up"][:3]]
        self.inp = _lib.SrhSplatNdcInputs(pos=ptr["pos"], pos_view_stride=self.N * 3, normal=ptr["normal"],
                                          normal_view_stride=self.N * 3, eye=ptr["eye"], material_idx=ptr["material_idx"])
        self.li = _lib.SrhLights(n_lights=lights["pos"].shape[0], n_colors=scene["colors"].shape[0], pos=ptr["lights_pos"],
                                 color_idx=ptr["color_idx"], colors=ptr["colors"], attenuation=ptr["attenuation"],
                                 ambient=ptr["ambient"])
        self.ma = _lib.SrhMaterials(n_materials=scene["materials"]["albedo"].shape[0], albedo=ptr["albedo"],
                                    coeffs=ptr["coeffs"])
        self.ups = [_dev(c["upstream"][k]) for k in ("image", "depth", "pos")]

    def _args(self):
        return C.byref(self.p), C.byref(self.inp), C.byref(self.li), C.byref(self.ma)

    def fwd(self):
        """Outputs from buffers prefilled with NaN."""
        H, W = self.H, self.W
        out = {"image": (H, W, 3), "depth": (H, W), "pos": (H, W, 3)}
        out = {k: torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for k, s in out.items()}
        self._lib.check(self.lib.srh_splat_ndc_fwd(*self._args(), out["image"].data_ptr(), out["depth"].data_ptr(),
                                                   out["pos"].data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def bwd(self):
        """(written gradients from buffers prefilled with NaN, the atomic sums from zero-filled ones of the arrays that
        are there)."""
        g = {"pos": torch.full((self.N, 3), float("nan"), dtype=torch.float32, device=DEV),
             "normal": torch.full((self.N, 3), float("nan"), dtype=torch.float32, device=DEV)}
        for k in self.SUMS:
            if self.t[k] is not None:
                g[k] = torch.zeros_like(self.t[k])
        sg = self._lib.SrhSplatNdcGrads(**{k: v.data_ptr() for k, v in g.items()})
        self._lib.check(self.lib.srh_splat_ndc_bwd(*self._args(), *[u.data_ptr() for u in self.ups], C.byref(sg),
                                                   torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in g.items()}
        return {k: g.pop(k) for k in ("pos", "normal")}, g


def _assert_identical(a, b, tag):
    assert set(a) == set(b)
    for k in a:
        assert not np.isnan(a[k]).any() and not np.isnan(b[k]).any(), (tag, k)
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (tag, k)


def _sums_close(got, want, tag):
    for k in set(got) & set(want):
        _atomic_close(got[k].astype(np.float64), want[k].astype(np.float64), f"{tag} {k}")


def test_abi_null_optional_arrays_equal_their_documented_defaults():
    L, M, N = 2, 2, 65
    explicit = {"attenuation": np.tile(np.array([1.0, 0.0, 0.0], np.float32), (L, 1)), "ambient": np.zeros(3, np.float32),
                "coeffs": np.tile(np.array([1.0, 0.0, 0.0], np.float32), (M, 1)), "material_idx": np.zeros(N, np.int64)}
    a, b = _AbiCall(**explicit), _AbiCall(**{k: None for k in explicit})
    assert a.N == N and a.li.n_lights == L and a.ma.n_materials == M
    fa, fb = a.fwd(), b.fwd()
    _assert_identical(fa, fb, "forward")
    assert all(np.isfinite(v).all() for v in fa.values()) and np.abs(fa["image"]).max() > 0.1
    (wa, sa), (wb, sb) = a.bwd(), b.bwd()
    _assert_identical(wa, wb, "written gradients")
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in wa.values())
    assert set(sb) == {"lights_pos", "colors", "albedo"} and set(sa) == set(_AbiCall.SUMS)
    _sums_close(sb, sa, "NULL")                            # the atomic sums agree up to the order of their additions
    assert all(np.abs(sa[k]).max() > 0 for k in sb)
    assert np.all(sa["albedo"][1] == 0) and np.all(sb["albedo"][1] == 0)              # material 0 throughout
    # and the defaults are not those of the scene: the scene's own arrays give another picture
    assert not np.array_equal(_AbiCall().fwd()["image"], fa["image"])


def test_abi_material_and_colour_indices_are_clamped():
    N = 65
    mat = np.random.RandomState(15).choice([-1, 0, 1, 2, 100], N)
    mat[:5], mat[64] = [-1, 0, 1, 2, 100], 100             # n = 2 materials: -1, n and 100 are out of range
    cidx = np.array([-1, 100])                             # n = 3 colours
    raw, clamped = _AbiCall(material_idx=mat, color_idx=cidx), _AbiCall(material_idx=np.clip(mat, 0, 1),
                                                                        color_idx=np.clip(cidx, 0, 2))
    fr, fc = raw.fwd(), clamped.fwd()
    _assert_identical(fr, fc, "forward")
    (wr, sr), (wc, sc) = raw.bwd(), clamped.bwd()
    _assert_identical(wr, wc, "written gradients")
    _sums_close(sr, sc, "clamped indices")
    assert np.all(sr["colors"][1] == 0) and np.abs(sr["colors"][[0, 2]]).min() > 0    # rows 0 and 2 are the lights'
    assert np.abs(sr["albedo"]).min() > 0 and np.abs(sr["coeffs"]).min() > 0
    for cidx_n in (np.array([3, 3]), ):                    # n itself
        _assert_identical(_AbiCall(color_idx=cidx_n).fwd(), _AbiCall(color_idx=np.array([2, 2])).fwd(), "color_idx = n")
    # the clamp matters: the in-range scene indices give another picture
    assert not np.array_equal(_AbiCall().fwd()["image"], fr["image"])


def test_abi_results_match_the_restatement():
    """The ABI call of the scene as it is, against the restatement: what the two tests above compare with each other is
    itself right."""
    c = edges.abi_scene()
    want, want_g = oracle.gradients(c["scene"], {k: c["upstream"][k] for k in ("image", "depth", "pos")}, **c["kwargs"])
    call = _AbiCall()
    f, (w, s) = call.fwd(), call.bwd()
    for k in ("image", "depth", "pos"):
        _close(f[k].astype(np.float64), want[k], k)
    _close(w["pos"].astype(np.float64), want_g["disk.pos"], "g_pos")
    _close(w["normal"].astype(np.float64), want_g["disk.normal"], "g_normal")
    for k, leaf in (("lights_pos", "lights.pos"), ("colors", "colors"), ("attenuation", "lights.attenuation"),
                    ("ambient", "lights.ambient"), ("albedo", "materials.albedo"), ("coeffs", "materials.coeffs")):
        _atomic_close(s[k].astype(np.float64), want_g[leaf], k)
