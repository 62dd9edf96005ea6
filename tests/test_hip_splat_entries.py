"""GPU: every forward output element and every gradient entry of the splat kernels (csrc/srh_splat.h: k_splat_fwd,
k_splat_bwd, k_splat_gather) held to its OWN rounding bound against the fp64 oracle (tests/splat_oracle.py), on every case
of tests/splat_edge_scenes.py and every p1_ fixture.  tests/splat_entry_bounds.py states and derives the bounds:

  written (outputs, disk.pos, disk.normal, light_vis at K = 1)   2^-24 |want| + C64 scale
  light_vis at K > 1                                              K^2 2^-24 absolute
  atomic leaves                                                   (1 + 6 + adds) 2^-24 absolute
each times (1 + 2^-20); `absolute` is the oracle's sum of the |terms| in the kernel's own grouping
(splat_oracle.gradient_terms), `adds` is counted from the case (splat_entry_bounds.add_counts), and an entry whose
absolute is 0 -- unused colour and material rows, columns 0 and 1 of a three-column pos, splats with z >= 0, the
attenuation of a light whose denominator is 0 -- must be exactly 0.  tests/test_splat_entry_bounds_cpu.py pins the
counts, the oracle's terms and the distance of every relu from its threshold.

Two runs: written values (light_vis chains included, their order is fixed) are bit-identical, atomic leaves differ by at
most their bound (which is all accumulation).  At K > 1 the light_vis chain is also replayed from the oracle's fp64
terms, one rounding per step, and must agree within K^2 2^-36 absolute -- the cap of the fp64 floor, a fraction of an
ulp: the K^2 2^-24 bound is a worst case that a chain rounding twice per step stays inside, the replay is not.

Two places where the bound needs a word:
  clamped_given_k2   the oracle's d loss / d normal is NaN on the rows with z >= 0 (sqrt'(0) * 0 through the depth of an
                     origin splat); the depth of such a splat is 0 whatever its normal (d0 = P . n with P = 0), so `want`
                     there is the sum of the other three outputs' gradients, which are finite.
  p1_norm_depth      its image is the normalised depth, made by torch in fp32 from the kernel's depth: it is no kernel
                     output and its upstream reaches the kernel through fp32 arithmetic, so the per-entry test drives
                     this fixture with the upstreams of depth, normal and pos (tests/test_hip_splats.py keeps the image).

The tolerances of tests/test_hip_splats.py and tests/test_hip_splats_edges.py stay: at D = 71 and absolute / |want| = 111
(k8_est, a lights.attenuation entry) the bound here is above theirs."""
import copy
import functools

import numpy as np
import pytest
import torch

import splat_entry_bounds as EB
import splat_oracle
from grad_cases import assert_entries_close
from splat_edge_scenes import CASES, base_scene, given_normals, reference, surface, terms
from test_hip_splats import CASES as FIXTURES, DEV, _gpu_scene, _hip, _load

pytestmark = pytest.mark.gpu

ALL = tuple(CASES) + tuple(FIXTURES)
WORST = {}
EXCESS = {}


def _leaf_class(key, K=1):
    if key in EB.ATOMIC:
        return "atomic " + key
    return key + (" (chain)" if key == "disk.light_vis" and K > 1 else " (written)")


def _note(cls, ratio):
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for cls, ratio in sorted(WORST.items()):
        print(f"[splat entries] worst error / bound of {cls}: {ratio:.3g}")
    if EXCESS:
        tag, worst = max(EXCESS.items(), key=lambda kv: kv[1])
        print(f"[splat entries] C64 measurement: {worst:.4g} at {tag}; in use {EB.C64:.4g} = {EB.C64_FACTOR} x "
              f"{EB.C64_MEASURED:.4g}, cap {EB.C64_CAP:.4g}")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(scene, kwargs, upstream, oracle outputs, want gradients, absolute) of an edge case or a p1_ fixture."""
    if name in CASES:
        scene, kw, notes, up, out, grads = reference(name)
        total, absolute = terms(name)
    else:
        npz, scene, kw = _load(name)
        up = {k: npz["grad_in/" + k] for k in splat_oracle.OUTPUTS if k != "image" or not kw.get("norm_depth_image_only")}
        out = splat_oracle.gradients(scene, up, **kw)[0]
        total, absolute = splat_oracle.gradient_terms(scene, up, **kw)
    want = dict(total)
    for k, w in total.items():
        if not np.isfinite(w).all():
            parts = splat_oracle.per_output_gradients(scene, up, **kw)
            want[k] = np.where(np.isfinite(w), w, sum(np.where(np.isfinite(p[k]), p[k], 0.0) for p in parts.values()))
    return scene, kw, up, out, want, absolute


def _run(name):
    scene, kw, up, *_ = _reference(name)
    return _hip(scene, {k: np.array(v) for k, v in up.items()}, **kw)


def _kernel_outputs(kw):
    return [k for k in splat_oracle.OUTPUTS if k != "image" or not kw.get("norm_depth_image_only")]


def _check_outputs(tag, got, want, kw, c64=None):
    for k in _kernel_outputs(kw):
        _note("output " + k, assert_entries_close(got[k], want[k], EB.output_bound(want[k], c64), f"{tag} {k}"))


def _check_leaf(tag, key, got, want, absolute, counts, K, c64=None):
    bound = EB.leaf_bound(key, want, absolute, counts, K, c64)
    _note(_leaf_class(key, K), assert_entries_close(got, want, bound, f"{tag} {key}"))
    assert not np.asarray(got).reshape(absolute.shape)[absolute == 0].any(), f"{tag} {key}: an entry with no term"
    return bound


def _replay_chain(scene, up, kw):
    """disk.light_vis as k_splat_bwd's chain leaves it, from the oracle's fp64 terms: (float) of the first, then
    (float)((double) sum + term) per sub-pixel."""
    t = splat_oracle.light_vis_terms(scene, up, **kw)
    acc = t[..., 0].astype(np.float32)
    for s in range(1, t.shape[-1]):
        acc = (acc.astype(np.float64) + t[..., s]).astype(np.float32)
    return acc.astype(np.float64)


# ---- a. every leaf of every case, twice ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_every_output_element_and_gradient_entry(name):
    scene, kw, up, want_out, want, absolute = _reference(name)
    K = int(kw.get("samples", 1))
    got_out, got = _run(name)
    again_out, again = _run(name)
    assert set(got) == set(want)
    _check_outputs(name, got_out, want_out, kw)
    counts = EB.add_counts(scene, kw)
    for key in want:
        bound = _check_leaf(name, key, got[key], want[key], absolute[key], counts, K)
        if key in EB.ATOMIC:
            assert_entries_close(again[key], got[key], bound, f"{name} {key} run to run")
        else:
            assert np.array_equal(again[key], got[key]), f"{name} {key}: a written gradient differs between two runs"
    for k in _kernel_outputs(kw):
        assert np.array_equal(again_out[k], got_out[k]), f"{name} {k}: an output differs between two runs"
    if K > 1 and "disk.light_vis" in want:
        a = absolute["disk.light_vis"]
        assert_entries_close(got["disk.light_vis"], _replay_chain(scene, up, kw).reshape(a.shape), K * K * EB.C64_CAP * a,
                             f"{name} light_vis chain replayed")


def test_named_zero_entries_exist():
    """The exact zeros the bounds demand are there to be demanded."""
    absolute = {name: _reference(name)[5] for name in ("materials_by_wave", "zpos_cols3", "clamped_est", "zero_attenuation")}
    assert not absolute["materials_by_wave"]["materials.albedo"][2].any() and absolute["materials_by_wave"]["materials.albedo"][:2].all()
    assert not absolute["materials_by_wave"]["colors"][0].any()
    assert not absolute["zpos_cols3"]["disk.pos"][:, :2].any() and absolute["zpos_cols3"]["disk.pos"][:, 2].all()
    assert (absolute["clamped_est"]["disk.pos"] == 0).sum() == 10
    assert not absolute["zero_attenuation"]["lights.attenuation"][1].any()
    assert absolute["zero_attenuation"]["lights.attenuation"][2].all() and absolute["zero_attenuation"]["lights.pos"][1, :3].all()


# ---- b. the fp64 floor ---------------------------------------------------------------------------------------------------
def test_fp64_floor_is_measured_and_under_its_cap():
    """C64: the largest (|got - want| - 2^-24 |want|) / scale over the written entries of all cases, times C64_FACTOR."""
    nonzero = {}
    for name in ALL:
        scene, kw, up, want_out, want, absolute = _reference(name)
        K = int(kw.get("samples", 1))
        got_out, got = _run(name)
        for k in _kernel_outputs(kw):
            EXCESS[f"{name} {k}"] = EB.written_excess(got_out[k], want_out[k], np.abs(want_out[k]).max())
            nonzero[f"{name} {k}"] = EB.written_excess(got_out[k], want_out[k], np.abs(want_out[k]).max(), nonzero=True)
        for key in want:
            if key in EB.WRITTEN or (key == "disk.light_vis" and K == 1):
                EXCESS[f"{name} {key}"] = EB.written_excess(got[key], want[key], absolute[key])
                nonzero[f"{name} {key}"] = EB.written_excess(got[key], want[key], absolute[key], nonzero=True)
    tag, worst = max(EXCESS.items(), key=lambda kv: kv[1])
    print(f"[splat entries] largest fp64 excess {worst:.4g} ({tag})")
    for t, v in sorted(nonzero.items(), key=lambda kv: -kv[1])[:8]:
        print(f"[splat entries]   over the entries with want != 0, {t}: {v:.4g}")
    assert EB.C64 <= EB.C64_CAP, "a constant above the cap: a finding to explain from the code"
    assert EB.C64 == EB.C64_FACTOR * EB.C64_MEASURED
    assert worst <= EB.C64_MEASURED * 1.01, "the recorded measurement no longer holds"


# ---- c. the batch forms ----------------------------------------------------------------------------------------------------
BATCH_B, BATCH_H, BATCH_W, BATCH_K = 3, 5, 13, 2


def _batch_scene(shared):
    """B = 3 views on 5 x 13: pos per view; normals, light_vis and lights.pos per view, or shared."""
    B, H, W = BATCH_B, BATCH_H, BATCH_W
    scene = base_scene(H, W, seed=90)
    d = scene["objects"]["disk"]
    d["pos"] = np.stack([surface(H, W, 91 + b) for b in range(B)])
    normal = np.stack([given_normals(H, W, 94 + b) for b in range(B)])
    vis = np.random.RandomState(97).uniform(0.1, 1.0, (B, 2, H * W)).astype(np.float32)
    lpos = np.stack([scene["lights"]["pos"] + np.float32(0.5 * b) * np.array([[1, 0, -1, 0], [0, 1, 0, 0]], np.float32)
                     for b in range(B)])
    d["normal"], d["light_vis"], scene["lights"]["pos"] = (normal[0], vis[0], lpos[0]) if shared else (normal, vis, lpos)
    return scene


def _view(scene, b, shared):
    sc = copy.deepcopy(scene)
    d = sc["objects"]["disk"]
    d["pos"] = d["pos"][b]
    if not shared:
        d["normal"], d["light_vis"], sc["lights"]["pos"] = d["normal"][b], d["light_vis"][b], sc["lights"]["pos"][b]
    return sc


@pytest.mark.parametrize("shared", [False, True], ids=["per-view", "shared"])
def test_batch_entries(shared):
    """Each view's rows against the one-view oracle; a leaf the views share against the sum of the views' oracles, with
    B times the additions where the views add into one buffer and B - 1 more where splats.py sums over the views."""
    from surf_renderer_amd import render_splats_along_ray_batch
    B, H, W, K = BATCH_B, BATCH_H, BATCH_W, BATCH_K
    scene = _batch_scene(shared)
    kw = {"samples": K}
    rng = np.random.RandomState(98)
    up = {k: rng.uniform(-1, 1, (B, K * H, K * W) + ((3,) if k != "depth" else ())).astype(np.float32)
          for k in splat_oracle.OUTPUTS}
    sc, leaves = _gpu_scene(scene)
    res = render_splats_along_ray_batch(sc, **kw)
    sum((res[k] * torch.as_tensor(up[k], device=DEV)).sum() for k in up).backward()
    torch.cuda.synchronize()
    got_out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in res.items()}
    got = {k: t.grad.cpu().numpy().astype(np.float64) for k, t in leaves.items()}
    per_view = ("disk.pos",) if shared else ("disk.pos", "disk.normal", "disk.light_vis", "lights.pos")
    one_counts = EB.add_counts(_view(scene, 0, shared), kw)
    all_counts = EB.add_counts(_view(scene, 0, shared), kw, views=B)
    wants, bounds, absolutes = {}, {}, {}
    for b in range(B):
        one = _view(scene, b, shared)
        up_b = {k: v[b] for k, v in up.items()}
        want_out = splat_oracle.gradients(one, up_b, **kw)[0]
        want, absolute = splat_oracle.gradient_terms(one, up_b, **kw)
        _check_outputs(f"batch view {b}", {k: v[b] for k, v in got_out.items()}, want_out, kw)
        for key in want:
            if key in per_view:
                _check_leaf(f"batch view {b}", key, got[key][b], want[key], absolute[key], one_counts, K)
            else:
                wants.setdefault(key, []).append(want[key])
                absolutes.setdefault(key, []).append(absolute[key])
                if key not in EB.ATOMIC:
                    bounds.setdefault(key, []).append(EB.leaf_bound(key, want[key], absolute[key], one_counts, K))
    assert set(wants) == set(EB.ATOMIC[1:] if not shared else EB.ATOMIC + ("disk.normal", "disk.light_vis"))
    for key in wants:
        want, absolute = sum(wants[key]), sum(absolutes[key])
        assert got[key].shape == want.shape, key
        if key in EB.ATOMIC:                                  # the views add into one buffer: B times the additions
            bound = EB.atomic_bound(absolute, all_counts[key])[0]
        else:                                                 # written per view, then g.sum(0): B - 1 more additions
            bound = EB.shared_written_bound(wants[key], bounds[key])
        _note("batch shared " + key, assert_entries_close(got[key], want, bound, f"batch shared {key}"))
        assert not got[key][absolute == 0].any(), key
