"""GPU: the occlusion fields of the disc reject record, record by record.  The library exports no offset of a frame's
rec32, so tests/occl_record_probe.hip -- compiled here against the library's own srh_reject.h -- runs
disk_reject_record on 2 000 random discs and hands back the records with V (the stored word [10]).  For every fp64 hit on
a 32 x 32 pixel sample:  V <= 1 / t <= U.  V is 1e30 exactly for the discs without certain hits (s_in = -1e30), among
them discs whose ball crosses near or far, discs seen edge-on and non-finite ones."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 192
EYE = np.array([0.0, 0.0, 4.0])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from surf_renderer_amd import build
    exe = str(tmp_path_factory.mktemp("probe") / "occl_record_probe")
    cmd = [build.hipcc(), "-O2", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I", build.INCLUDE, "-I",
           build.CSRC, os.path.join(REPO, "tests", "occl_record_probe.hip"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    return exe


def _records(probe, tmp_path, discs, near, far):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(discs, np.float64).tofile(src)
    proc = subprocess.run([probe, src, dst, str(W), str(H), repr(near), repr(far)], capture_output=True, text=True,
                          timeout=120)
    assert proc.returncode == 0, proc.stderr
    return np.fromfile(dst, np.float32).reshape(len(discs), 13)


def _discs(rng, n):
    """centres, unit normals, radii as the library sees them: float32 values"""
    pos = rng.uniform(-1.0, 1.0, (n, 3))
    pos[:, 2] = rng.uniform(-1.5, 2.5, n)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[: n // 20] = [1.0, 0.0, 0.0]                        # seen edge-on or nearly so at the image's centre column
    nrm[: n // 40, 2] = 1e-3
    rad = rng.choice([0.02, 0.05, 0.2, 0.5, 1.5], n)
    d = np.concatenate([pos, nrm, rad[:, None]], axis=1).astype(np.float32).astype(np.float64)
    d[:, 3:6] /= np.linalg.norm(d[:, 3:6], axis=1, keepdims=True)     # k_prep normalises in fp64
    return d


def _hits(d, near, far):
    """1 / t (discs, pixels) of every valid fp64 hit on the pixel sample, nan elsewhere"""
    hh = np.tan(np.deg2rad(45.0) / 2.0)
    ww = hh * W / H
    c, r = np.meshgrid(np.linspace(0, W - 1, 32).round(), np.linspace(0, H - 1, 32).round())
    D = np.stack([(2.0 * c / (W - 1) - 1.0) * ww, (1.0 - 2.0 * r / (H - 1)) * hh, -np.ones(c.shape)], axis=-1).reshape(-1, 3)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    pos, nrm, rad = d[:, 0:3], d[:, 3:6], d[:, 6]
    k = np.einsum("ij,ij->i", pos - EYE, nrm)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = k[:, None] / (nrm @ D.T)
        q = EYE + t[..., None] * D[None] - pos[:, None]
        ok = (np.einsum("ijk,ijk->ij", q, q) <= rad[:, None] ** 2) & (t >= near) & (t <= far)
        return np.where(ok, 1.0 / t, np.nan)


@pytest.mark.parametrize("near,far", [(0.1, 1000.0), (2.5, 5.0)])
def test_v_and_u_bound_every_hit(probe, tmp_path, near, far):
    rng = np.random.RandomState(5)
    d = _discs(rng, 2000)
    rec = _records(probe, tmp_path, d, near, far)
    U, s_in, V = rec[:, 8].astype(np.float64), rec[:, 11], rec[:, 12].astype(np.float64)
    inv = _hits(d, near, far)
    assert np.isfinite(inv).sum() > 20000                   # the sample does see the discs
    sure = s_in > np.float32(-1.0e30)
    assert sure.sum() > 200 and (~sure).sum() >= 10         # both kinds are there
    assert (V[~sure] == np.float64(np.float32(1.0e30))).all()    # a disc without certain hits never lowers the minimum
    assert (V[sure] > 0.0).all() and (V[sure] < 1.0).all()
    with np.errstate(invalid="ignore"):                     # (nan = no hit at that pixel: compares false)
        assert not ((inv < V[:, None]) & sure[:, None]).any()    # V <= 1 / t for every hit of a disc that has certain hits
        assert not (inv > U[:, None]).any()                 # 1 / t <= U for every hit of every disc
    # the bound is the ball's, tight to its margins: (1 - 2^-19.9) / (l + r) <= V <= 1 / (l + r)
    l = np.linalg.norm(d[:, 0:3] - EYE, axis=1)
    exact = 1.0 / (l + d[:, 6])
    assert (V[sure] <= exact[sure]).all() and (V[sure] >= exact[sure] * (1.0 - 2.5e-6)).all()


def test_non_finite_and_huge_discs_are_never_sure(probe, tmp_path):
    d = _discs(np.random.RandomState(6), 64)
    d[0, 0] = np.nan
    d[1, 1] = np.inf
    d[2, 6] = 2.0 ** 30
    d[3, 0:3] = [0.0, -1e20, 0.0]
    d[3, 6] = 1e20
    d[4, 6] = 0.0
    d[5, 0:3] = EYE                                          # the eye at the centre
    rec = _records(probe, tmp_path, d, 0.1, 1000.0)
    for i in (0, 1, 2, 3, 5):
        assert rec[i, 11] == np.float32(-1.0e30) and rec[i, 12] == np.float32(1.0e30), (i, rec[i])
    assert not np.isnan(rec[:, 12]).any()
