#!/usr/bin/env python3
"""Generate tests/golden/pointsets/ps1_*.npz: the reference's OWN hausdorff (diffrend/torch/ops.py:112-125), imported
UNMODIFIED and run on the CPU under autograd, on the regular cases of tests/pointsets_cases.py -- once in float64 and
once in float32.  The reference is unbatched, so every view is recorded on its own.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.

Stored per fixture: in/u [B, N, D], in/v [B, M, D], grad_in/g [B, 3] (the case's upstream gradient of (sym, uv, vu)),
grad_in/g_u, grad_in/g_v (the case's upstream gradients of dist_u and dist_v, for the tests against the oracle), and for
P in (ref64, ref32): P/out [B, 3] = (sym, uv, vu) and P/grad/u, P/grad/v = d sum(out * g) / d u, d v, in that precision.
The subfolder keeps the fixtures out of the top-level globs (the golden drift check, conftest.golden_cases)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import pointsets_cases as cases  # noqa: E402

with R.quiet():
    import diffrend.torch.ops as ref_ops  # noqa: E402


def record(c, dtype):
    out, grad_u, grad_v = [], [], []
    for b in range(cases.VIEWS):
        u = torch.tensor(c["u"][b], dtype=dtype, requires_grad=True)
        v = torch.tensor(c["v"][b], dtype=dtype, requires_grad=True)
        with R.quiet():
            res = torch.stack(ref_ops.hausdorff(u, v))
        assert res.dtype == dtype and res.shape == (3,)
        torch.sum(res * torch.tensor(c["g"][b], dtype=dtype)).backward()
        out.append(res.detach().numpy())
        grad_u.append(u.grad.numpy())
        grad_v.append(v.grad.numpy())
    return {"out": np.stack(out), "grad/u": np.stack(grad_u), "grad/v": np.stack(grad_v)}


def emit(k):
    c = cases.regular(k)
    flat = {"in/u": c["u"], "in/v": c["v"], "grad_in/g": c["g"], "grad_in/g_u": c["g_u"], "grad_in/g_v": c["g_v"]}
    for prefix, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
        for key, val in record(c, dtype).items():
            flat[prefix + "/" + key] = val
    R.write("ps1_" + c["name"], flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("pointsets")
    for k in range(len(cases.REGULAR)):
        emit(k)
