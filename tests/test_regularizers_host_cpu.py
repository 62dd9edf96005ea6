"""The per-pixel arithmetic of srh_regularizers.h (reg_pixel_fwd, reg_finish, reg_pixel_bwd), which is host-callable,
built for the host (tests/host/regularizers_host.hip: a stand-alone program, no HIP call, no GPU) and held to the fp64
restatement on every seeded case (tests/regularizer_cases.py) and every edge case (tests/regularizer_edge_cases.py).

Tolerance.  Both sides are fp64 evaluations of the same formulas in another summation order: over the 8 x 16 512 pair
terms of the largest case the worst case is n 2^-53 = 1.5e-11, so values are held to rtol 1e-10 before the float cast
(the stored float is the cast of that double, bit for bit) and every gradient array to 1e-10 max|want|; the one-hot
cases make that per term.  `-s` prints the worst ratio per case; DESIGN.md 4c records the largest.  That is four
orders below what the fp32 stores let the GPU comparison hold (2e-7), on a machine where the kernels cannot run: a
wrong epsilon, multiplicity or sign shows here.

Poisoned batches: the class of every term equals the restatement's; gradients are compared where the restatement's are
finite (edge.finite_mask, pinned by tests/test_regularizer_edge_cases_cpu.py) and must be finite there.

Two builds, the same cases: plain, and with -fsanitize=address,undefined on the host side (any report fails: the
reflected indexing at H = 2 / W = 2, the corners, the last ragged pixel).  The sanitized build is for machines
without a GPU and is skipped where there is one.  The sanitizer is linked into the program; nothing is preloaded."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import regularizer_cases as cases
import regularizer_edge_cases as edge
import regularizer_oracle as ro
from conftest import REPO

SRC = os.path.join(REPO, "tests", "host", "regularizers_host.hip")
FLAGS = ["--offload-arch=gfx950", "-O1", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(REPO, "include"),
         "-I", os.path.join(REPO, "surf_renderer_amd", "csrc")]
SANITIZE = ["-g", "-Xarch_host", "-fsanitize=address,undefined"]
SETTINGS = ((1, 1), (1, 0), (0, 1))                      # (want_geo, want_img): all that do any work
RTOL = 1e-10
ALL_NAMES = tuple(("seeded", n) for n in cases.NAMES) + tuple(("edge", n) for n in edge.NAMES)
_IDS = [f"{m}-{n}" for m, n in ALL_NAMES]


def _case(which):
    return (cases if which[0] == "seeded" else edge).case(which[1])


def _expected(which):
    return (cases if which[0] == "seeded" else edge).expected(which[1])


class Driver:
    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.n = exe, tmp, 0
        self.run = functools.lru_cache(maxsize=None)(self._run_named)
        self.worst = {}

    def __call__(self, c, geo=1, img=1):
        """({term: (B,)} before the cast, the same after it, stats (B, 4), {input: gradient}) of a case dict."""
        B, H, W = c["depth"].shape
        self.n += 1
        src, dst = os.path.join(self.tmp, f"in{self.n}.bin"), os.path.join(self.tmp, f"out{self.n}.bin")
        with open(src, "wb") as f:
            f.write(np.array([B, H, W], dtype=np.int32).tobytes())
            f.write(np.array([c["z_min"], c["z_max"], c["z_scale"], c["unit_normal_scale"]], dtype=np.float64).tobytes())
            for k in ro.INPUTS + ("weights",):
                assert c[k].dtype == np.float32
                f.write(np.ascontiguousarray(c[k]).tobytes())
        r = subprocess.run([self.exe, src, dst, str(geo), str(img)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", f"exit {r.returncode}\n{r.stderr}"      # a sanitizer report is stderr
        out = np.fromfile(dst, dtype=np.float64)
        os.remove(src), os.remove(dst)
        assert out.size == B * 18 + B * H * W * 8
        head, g = out[:B * 18].reshape(B, 18), out[B * 18:].reshape(B, H, W, 8)
        grads = {"pos": g[..., 0:3], "normal": g[..., 3:6], "image": np.repeat(g[..., 6:7] / 3.0, 3, axis=-1),
                 "depth": g[..., 7]}
        return ({t: head[:, k] for k, t in enumerate(ro.TERMS)}, {t: head[:, 7 + k] for k, t in enumerate(ro.TERMS)},
                head[:, 14:], grads)

    def _run_named(self, which, geo=1, img=1):
        return self(_case(which), geo, img)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    if request.param == "sanitized" and torch.cuda.is_available():
        pytest.skip("sanitizer builds are for machines without a GPU")
    tmp = str(tmp_path_factory.mktemp("reg_host_" + request.param))
    exe = os.path.join(tmp, "regularizers_host")
    r = subprocess.run([hipcc, *FLAGS, *(SANITIZE if request.param == "sanitized" else []), SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return Driver(exe, tmp)


def _ratio(got, want, mask=None):
    """max |got - want| / max |want| over the mask; 0 for an empty or all-zero-and-equal comparison."""
    if mask is not None:
        got, want = got[mask], want[mask]
    if want.size == 0:
        return 0.0
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    err, top = np.abs(got - want).max(), np.abs(want).max()
    return 0.0 if err == 0.0 else err / top


def _check(driver, which, c, want_v, want_g, pre, post, stats, got_g, masks=None):
    tag = "-".join(which)
    worst_v = worst_g = 0.0
    for t in ro.TERMS:
        assert list(edge.classify(pre[t])) == list(edge.classify(want_v[t])), (tag, t, pre[t], want_v[t])
        fin = np.isfinite(want_v[t])
        rel = np.abs(pre[t][fin] - want_v[t][fin]) / np.maximum(np.abs(want_v[t][fin]), 1e-300)
        rel[pre[t][fin] == want_v[t][fin]] = 0.0
        worst_v = max(worst_v, rel.max(initial=0.0))
        np.testing.assert_allclose(pre[t][fin], want_v[t][fin], rtol=RTOL, atol=0, err_msg=f"{tag} {t}")
        with np.errstate(over="ignore"):
            assert np.array_equal(pre[t].astype(np.float32).astype(np.float64), post[t], equal_nan=True), (tag, t)
    fin = np.isfinite(want_v["spatial_var"])
    pos = c["pos"].astype(np.float64).reshape(c["pos"].shape[0], -1, 3)
    np.testing.assert_allclose(stats[fin, :3], pos[fin].mean(axis=1), rtol=0, atol=RTOL * np.abs(pos[fin]).max(initial=0))
    np.testing.assert_allclose(1.0 / (stats[fin, 3] + 1e-4), want_v["spatial_var"][fin], rtol=RTOL)
    for k in ro.INPUTS:
        m = None if masks is None else masks[k]
        r = _ratio(got_g[k], want_g[k], m)
        worst_g = max(worst_g, r)
        assert r <= RTOL, (tag, k, r)
    driver.worst[tag] = (worst_v, worst_g)
    print(f"{tag}: worst value rel err {worst_v:.3g}, worst gradient err / max|want| {worst_g:.3g}")
    return worst_v, worst_g


@pytest.mark.parametrize("which", ALL_NAMES, ids=_IDS)
def test_values_and_gradients_match_the_restatement(driver, which):
    c = _case(which)
    want_v, want_g = _expected(which)
    pre, post, stats, got_g = driver.run(which)
    masks = {k: edge.finite_mask(which[1], k) for k in ro.INPUTS} if which[0] == "edge" else None
    if which[0] == "seeded":
        assert all(np.all(np.isfinite(want_g[k])) for k in ro.INPUTS)                # nothing left out
    _check(driver, which, c, want_v, want_g, pre, post, stats, got_g, masks)
    if which[1] in edge.ONEHOT_NAMES:
        term = ro.TERMS[edge.ONEHOT_NAMES.index(which[1])]
        for k in ro.INPUTS:
            assert (k in edge.REACH[term]) == bool(np.any(got_g[k] != 0.0)), (which, k)
    if which[1] == "huge_pos":               # the other pixels against their own largest entry, not the huge pixel's
        far = ~edge.block(c, *edge.PIXEL)
        for k in ro.INPUTS:
            assert _ratio(got_g[k][0], want_g[k][0], far) <= RTOL, k


@pytest.mark.parametrize("which", ALL_NAMES, ids=_IDS)
def test_each_half_alone_is_that_half_of_the_whole(driver, which):
    _, _, _, both = driver.run(which)
    pre, _, _, geo = driver.run(which, 1, 0)
    pre2, _, _, img = driver.run(which, 0, 1)
    for t in ro.TERMS:
        assert np.array_equal(pre[t], pre2[t], equal_nan=True)
    for k in ("pos", "normal"):
        assert np.array_equal(geo[k], both[k], equal_nan=True), k
        assert np.all(img[k] == 0.0), k
    for k in ("image", "depth"):
        assert np.array_equal(img[k], both[k], equal_nan=True), k
        assert np.all(geo[k] == 0.0), k


@pytest.mark.parametrize("spec", edge.EXACT_ZEROS, ids=[f"{s[0]}-{s[1]}-{s[3]}" for s in edge.EXACT_ZEROS])
def test_the_conventions_are_exact_zeros(driver, spec):
    name, term, keys, mark = spec
    c = edge.one_hot(edge.case(name), term)
    pixels = c["marks"][mark]
    assert len(pixels) > 0
    _, _, _, g = driver(c)
    for k in keys:
        for (i, j) in pixels:
            assert np.all(g[k][0, i, j] == 0.0), (name, term, k, (i, j), g[k][0, i, j])
        if len(pixels) < c["depth"][0].size:
            assert np.any(g[k] != 0.0), (name, term, k)                              # the term is not switched off


def test_a_zero_normal_gets_no_unit_normal_gradient(driver):
    c = dict(cases.case("5x3"))
    c["normal"] = c["normal"].copy()
    c["normal"][0, 2, 1] = 0.0
    _, _, _, g = driver(edge.one_hot(c, "unit_normal"))
    assert np.all(g["normal"][0, 2, 1] == 0.0)
    assert np.count_nonzero(g["normal"]) == g["normal"].size - 3
    pre, _, _, g = driver(c)                                                         # all seven terms: finite
    assert all(np.all(np.isfinite(v)) for v in pre.values()) and all(np.all(np.isfinite(v)) for v in g.values())
    _, want_g = ro.gradients({k: c[k] for k in ro.INPUTS}, c["weights"], c["z_min"], c["z_max"], c["z_scale"],
                             c["unit_normal_scale"])
    keep = np.ones((1, 5, 3), dtype=bool)
    keep[0, 2, 1] = False
    assert not np.all(np.isfinite(want_g["normal"][~keep]))                          # autograd's 0 / 0
    for k in ro.INPUTS:
        assert _ratio(g[k], want_g[k], keep) <= RTOL, k


@pytest.mark.parametrize("name", edge.POISONED_NAMES)
def test_poison_stays_in_its_view(driver, name):
    c = edge.case(name)
    pre, post, _, g = driver.run(("edge", name))
    for t in ro.TERMS:
        assert list(edge.classify(post[t])) == ["finite", edge.PINS[name]["terms"][t], "finite"], t
    for b in (0, 2):
        pre1, post1, _, g1 = driver(edge.view(c, b))
        for t in ro.TERMS:
            assert pre1[t][0] == pre[t][b] and post1[t][0] == post[t][b], (b, t)
        for k in ro.INPUTS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)


def test_huge_and_tiny_positions_keep_their_results(driver):
    tiny = float(np.finfo(np.float32).tiny)
    for name in ("huge_pos", "tiny_pos"):
        want_v, want_g = edge.expected(name)
        _, post, _, g = driver.run(("edge", name))
        for t in ro.TERMS:
            normal = (np.abs(want_v[t]) >= tiny) & (np.abs(want_v[t]) <= 3e38)
            assert np.all(np.isfinite(post[t])) and np.all(post[t][normal] != 0.0), (name, t)
        for k in ro.INPUTS:
            normal = np.abs(want_g[k]) >= tiny
            assert np.all(np.isfinite(g[k])) and np.all(g[k][normal] != 0.0), (name, k)


def test_report_the_worst_ratios(driver):
    """Runs last in the module: the largest figures of the comparison above (`-s` shows them)."""
    if not driver.worst:                                 # selected alone: nothing was compared, nothing to report
        return
    v = max(driver.worst.items(), key=lambda kv: kv[1][0])
    g = max(driver.worst.items(), key=lambda kv: kv[1][1])
    print(f"worst value rel err {v[1][0]:.3g} ({v[0]}); worst gradient err / max|want| {g[1][1]:.3g} ({g[0]})")
    assert v[1][0] <= RTOL and g[1][1] <= RTOL
