#!/usr/bin/env python3
"""Generate tests/golden/sh_lighting/sh1_*.npz: the reference's OWN SH9 lighting (diffrend/numpy/sph.py) and probe loader
(diffrend/utils/lightprobe.py), imported UNMODIFIED and run on the cases of tests/sh9_cases.py.  The reference is numpy
on the host and takes one probe or one normal set per call, so every view is recorded on its own, on the view's float32
values widened to float64 -- the values the kernels compute on.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.

Stored per projection fixture: in/envmap [B, H, W, C] float32, ref/L [B, C, 9] = radiance_SH9, ref/M [B, 4, 4, C] =
RealSH9_ZonalMatrix of it, and for every dim of cases.GRID_DIMS ref/irrad_Z_<H>x<W> and ref/reconstruct_<H>x<W>
[B, H, W, C] of that L.  Per irradiance fixture: in/M, in/normal, in/L (what a zonal M was made of), ref/E [B, N, C] =
irradiance(M, normal) and, for a zonal case, ref/M = RealSH9_ZonalMatrix(in/L) before its rounding to float32.
sh1_lightprobe: in/bytes, the raw file, and per call of cases.LIGHTPROBE_CALLS ref/data_<k> and ref/processed_<k>.  The
subfolder keeps the fixtures out of the top-level globs (the golden drift check, conftest.golden_cases)."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import sh9_cases as cases  # noqa: E402

with R.quiet():
    import diffrend.numpy.sph as ref_sph  # noqa: E402
    import diffrend.utils.lightprobe as ref_probe  # noqa: E402


def emit_projection(k):
    c = cases.projection(k)
    flat = {"in/envmap": c["envmap"]}
    L = [ref_sph.radiance_SH9(e.astype(np.float64)) for e in c["envmap"]]
    flat["ref/L"] = np.stack(L)
    flat["ref/M"] = np.stack([ref_sph.RealSH9_ZonalMatrix(x) for x in L])
    for dim in cases.GRID_DIMS:
        flat["ref/irrad_Z_%dx%d" % dim] = np.stack([ref_sph.irrad_Z(x, dim) for x in L])
        flat["ref/reconstruct_%dx%d" % dim] = np.stack([ref_sph.reconstruct_SH9(x, dim) for x in L])
    R.write("sh1_" + cases.projection_tag(k), flat)


def emit_irradiance(k):
    c = cases.irradiance(k)
    flat = {"in/M": c["M"], "in/normal": c["normal"], "in/L": c["L"]}
    flat["ref/E"] = np.stack([ref_sph.irradiance(cases.view_M(c, b).astype(np.float64), c["normal"][b].astype(np.float64))
                              for b in range(cases.VIEWS)])
    if cases.IRRADIANCE[k][2] == "zonal":
        L = c["L"].astype(np.float64)
        flat["ref/M"] = ref_sph.RealSH9_ZonalMatrix(L) if L.ndim == 2 else np.stack([ref_sph.RealSH9_ZonalMatrix(x) for x in L])
    R.write("sh1_" + cases.irradiance_tag(k), flat)


def emit_lightprobe():
    raw = cases.lightprobe_bytes()
    flat = {"in/bytes": np.frombuffer(raw, np.uint8)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "probe.float")
        with open(path, "wb") as fh:
            fh.write(raw)
        for k, kw in enumerate(cases.LIGHTPROBE_CALLS):
            data, processed = ref_probe.load_lightprobe(path, **kw)
            flat["ref/data_%d" % k], flat["ref/processed_%d" % k] = np.ascontiguousarray(data), processed
    R.write("sh1_lightprobe", flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("sh_lighting")
    for k in range(len(cases.PROJECTION)):
        emit_projection(k)
    for k in range(len(cases.IRRADIANCE)):
        emit_irradiance(k)
    emit_lightprobe()
