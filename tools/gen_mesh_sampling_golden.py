#!/usr/bin/env python3
"""Generate tests/golden/mesh_sampling/ms1_*.npz: the reference's OWN uniform_sample_mesh
(diffrend/utils/sample_generator.py:157-194), imported UNMODIFIED and run on the regular cases of
tests/mesh_sampling_cases.py.  The reference is numpy on the host and takes one mesh per call, so every view is recorded
on its own: np.random.seed(the view's seed), then the call, on the view's float32 vertices widened to float64 -- the
values the kernels compute on.

Test infrastructure; needs the reference checkout (oracle/ref_harness.py locates it) and is run by hand -- no test reads
the reference.

Stored per fixture: in/v [B, V, 3] float32, in/f [F, 3] or [B, F, 3], in/eye ([3] or [B, 3]; absent without a camera),
in/seeds [B], in/uniforms [B, S, 3] (what the reference drew: the same seed replayed through random_sample(S) and
rand(S, 2)), ref/pos and ref/normal [B, S, 3] float64 as the reference returned them, and ref/face [B, S]: the
reference returns no face, so its choice is replayed with its own functions -- np.random.choice over its
triangle_double_area of its backface_culling's faces under the same seed -- and mapped back to the caller's f through
the cull's condition, which is recomputed from the reference's compute_face_normal and normalize and asserted to select
exactly the faces backface_culling kept.  The subfolder keeps the fixtures out of the top-level globs (the golden drift
check, conftest.golden_cases)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_harness as R  # noqa: E402

sys.path.insert(0, os.path.join(R.REPO, "tests"))
import mesh_sampling_cases as cases  # noqa: E402

with R.quiet():
    import diffrend.model as ref_model  # noqa: E402
    import diffrend.numpy.ops as ref_ops  # noqa: E402
    import diffrend.utils.sample_generator as ref_gen  # noqa: E402


def record_view(v, f, uniforms, eye, seed):
    obj = {"v": v.astype(np.float64), "f": np.array(f)}
    camera = None if eye is None else {"eye": np.array(eye, np.float64)}
    n_samples = len(uniforms)
    np.random.seed(seed)
    with R.quiet():
        pos, normal = ref_gen.uniform_sample_mesh(obj, n_samples, camera=camera)
    pos, normal = np.reshape(pos, (n_samples, 3)), np.reshape(normal, (n_samples, 3))      # S = 1 comes back squeezed
    # the face behind every sample: the reference's own choice, replayed
    kept = np.arange(len(f))
    seen = obj
    if camera is not None:
        seen = ref_ops.backface_culling(obj, camera=camera, copy=True)
        facing = np.sum(ref_model.compute_face_normal(obj) * ref_ops.normalize(camera["eye"] - obj["v"][obj["f"][:, 0]]), axis=-1)
        kept = np.flatnonzero(facing >= 0)
        assert np.array_equal(obj["f"][kept], seen["f"])
    area = ref_gen.triangle_double_area(seen)
    np.random.seed(seed)
    idx = np.random.choice(seen["f"].shape[0], n_samples, p=area / np.sum(area))
    drawn = np.concatenate([np.random.RandomState(seed).random_sample(n_samples)[:, None], np.zeros((n_samples, 2))], 1)
    assert np.array_equal(drawn[:, 0], uniforms[:, 0])                 # the case's r0 are what choice() consumed
    assert np.array_equal(ref_model.compute_face_normal(seen)[idx], normal)
    return pos, normal, kept[idx].astype(np.int64)


def emit(k):
    c = cases.regular(k)
    flat = {"in/v": c["v"], "in/f": c["f"], "in/seeds": c["seeds"], "in/uniforms": c["uniforms"]}
    if c["eye"] is not None:
        flat["in/eye"] = c["eye"]
    rows = [record_view(*cases.view_of(c, b), int(c["seeds"][b])) for b in range(cases.VIEWS)]
    for key, col in (("ref/pos", 0), ("ref/normal", 1), ("ref/face", 2)):
        flat[key] = np.stack([r[col] for r in rows])
    R.write("ms1_" + c["name"], flat)


if __name__ == "__main__":
    R.OUT = R.fixture_dir("mesh_sampling")
    for k in range(len(cases.REGULAR)):
        emit(k)
