#!/usr/bin/env python3
"""Generate tests/golden/splats_ndc/sn1_*.npz: the reference's OWN render_splats_NDC (diffrend/torch/renderer.py:
358-474), running UNMODIFIED on the CPU under autograd, in float64 (oracle.ref_harness.precision) and in float32, one view
at a time for the batched cases (a shared leaf's gradient is the sum over the views).

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.  The inputs are the seeded cases of tests/splats_ndc_cases.py.  Stored per fixture: in/* (float32 inputs,
camera scalars as float64), kwargs, grad_in/<output> (upstreams in (-1, 1)), ref64/<output> and grad64/<leaf> (float64),
ref32/<output> (float32) and grad32/<leaf>, and meta: the largest |ref32 - ref64| per array, with its tolerance.  Before
anything is written the generator asserts the cases' kink margins and both-sides coverage, and that for every array the
reference's own float32-float64 disagreement is at most a quarter of the float32 tolerance the GPU tests use (outputs
2e-5 max(max|want|, 1); gradients 3e-3 max(max|want|, 1e-6)).  sn2_*.npz are the edge cases of tests/
splats_ndc_edge_cases.py (wave-uniform materials, zero normals), recorded the same way.  The subfolder keeps the
fixtures out of the top-level globs (the golden drift check, conftest.golden_cases)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import splats_ndc_cases as cases  # noqa: E402
import splats_ndc_edge_cases as edges  # noqa: E402
import splats_ndc_oracle as oracle  # noqa: E402


def reference(c, dtype):
    """({output: (B, ...) array}, {leaf: gradient}) of the reference for case c in `dtype`."""
    scene, kw, ups = c["scene"], c["kwargs"], c["upstream"]
    B = oracle.n_views(scene)
    outs, grads = {k: [] for k in oracle.OUTPUTS}, {}
    for b, sc in enumerate(cases.views(scene)):
        tsc, leaves = R.torch_scene(sc, dtype=dtype)
        with R.precision(dtype), R.quiet():
            res = R.ref_tch.render_splats_NDC(tsc, **kw)
            loss = 0.0
            for k in oracle.OUTPUTS:
                assert res[k].dtype == dtype, (k, res[k].dtype)
                g = ups[k][b] if B else ups[k]
                assert tuple(res[k].shape) == g.shape, (k, tuple(res[k].shape), g.shape)
                loss = loss + torch.sum(res[k] * torch.tensor(g, dtype=dtype))
                outs[k].append(res[k].detach().numpy())
            loss.backward()
        for k, t in leaves.items():
            g = t.grad.numpy().astype(np.float64) if t.grad is not None else np.zeros(tuple(t.shape))
            grads.setdefault(k, []).append(g)
    outs = {k: (np.stack(v) if B else v[0]) for k, v in outs.items()}
    disk = scene["objects"]["disk"]
    per_view = {"disk.pos": B > 0, "disk.normal": np.ndim(disk["normal"]) == 3,
                "lights.pos": np.ndim(scene["lights"]["pos"]) == 3}
    return outs, {k: (np.stack(v) if per_view.get(k) else sum(v)) for k, v in grads.items()}


def emit(name, all_margins):
    c = cases.case(name)
    m = cases.margins(c["scene"], **c["kwargs"])
    assert all(v[0] >= cases.MARGIN for v in m.values()), (name, m)
    cases.check_special(c)
    all_margins.append(m)
    record("sn1_" + name, c)


def emit_edge(name):
    """sn2_<name>: a case of tests/splats_ndc_edge_cases.py.  Its at_kink splats sit on a kink on purpose -- where a
    restatement can drift from the function it restates -- and every other splat is held to the margins."""
    c = edges.case(name)
    m = edges.margins(c)
    assert all(v[0] >= cases.MARGIN for v in m.values()), (name, m)
    record("sn2_" + name, c)


def record(fixture, c):
    name = c["name"]
    ref64, grad64 = reference(c, torch.float64)
    ref32, grad32 = reference(c, torch.float32)
    out = oracle.pack(c["scene"])
    out["kwargs"] = np.asarray(json.dumps(c["kwargs"]))
    meta = {}
    for k, g in c["upstream"].items():
        out["grad_in/" + k] = g
        out["ref64/" + k], out["ref32/" + k] = ref64[k], ref32[k]
        err = float(np.abs(ref32[k].astype(np.float64) - ref64[k]).max())
        tol = 2e-5 * max(float(np.abs(ref64[k]).max()), 1.0)
        meta["ref/" + k] = {"err": err, "tol": tol, "max": float(np.abs(ref64[k]).max())}
        assert err <= tol / 4, (name, k, err, tol)
    for k in grad64:
        out["grad64/" + k], out["grad32/" + k] = grad64[k], grad32[k]
        err = float(np.abs(grad32[k] - grad64[k]).max())
        tol = 3e-3 * max(float(np.abs(grad64[k]).max()), 1e-6)
        meta["grad/" + k] = {"err": err, "tol": tol, "max": float(np.abs(grad64[k]).max())}
        assert err <= tol / 4, (name, k, err, tol)
    out["meta"] = np.asarray(json.dumps(meta, sort_keys=True))
    for k, v in out.items():
        assert v.dtype.kind not in "fc" or np.all(np.isfinite(v)), (name, k)
    R.write(fixture, out)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("splats_ndc")
    seen = []
    for n in cases.NAMES:
        emit(n, seen)
    cov = cases.coverage(seen)
    assert all(cov.values()), cov
    for n in edges.RECORDED:                   # a list of their own: the seeded fixtures above stay as they are
        emit_edge(n)
