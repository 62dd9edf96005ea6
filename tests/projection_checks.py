"""What the GPU tests of the three re-projection layers (tests/test_hip_projection.py, test_hip_dense_projection.py,
test_hip_reverse_projection.py) share: the comparison against the fp64 restatement under the layers' stated tolerances
(rtol 2e-6; atol 2e-7 max(|want|, 1) for values and 2e-7 max|want| per input array for gradients), one view of a batched
case as a case of its own, and the bit-for-bit comparison."""
import numpy as np

RTOL, ATOL_SCALE = 2e-6, 2e-7


def to_np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def compare_values(got, want, tag, rtol=RTOL, atol_scale=ATOL_SCALE, exact=()):
    """Every output of `want`, and no other, within the tolerance; those named in `exact` bit for bit."""
    assert set(got) == set(want), tag
    for k, w in want.items():
        assert got[k].shape == w.shape and np.all(np.isfinite(w)), (tag, k)
        if k in exact:
            assert np.array_equal(got[k], w), (tag, k)
        print(f"{tag} {k}: max err / max(|want|, 1) {np.abs(got[k] - w).max() / max(np.abs(w).max(), 1.0):.3g}")
        np.testing.assert_allclose(got[k], w, rtol=rtol, atol=atol_scale * max(np.abs(w).max(), 1.0), err_msg=f"{tag} {k}")


def compare_grads(got, want, tag, rtol=RTOL, atol_scale=ATOL_SCALE, nonzero=True):
    """Every gradient of `want` within the tolerance, atol following the array's own scale max|want|.  `nonzero`: the
    oracle's gradient must not vanish (a layer with inputs the loss may not reach passes False: the scale is then 0 and
    the comparison exact)."""
    for k, w in want.items():
        assert np.all(np.isfinite(w)) and got[k] is not None and got[k].shape == w.shape, (tag, k)
        scale = np.abs(w).max()
        assert scale > 0 or not nonzero, (tag, k)
        print(f"{tag} grad {k}: max err {np.abs(got[k] - w).max():.3g}, max|want| {scale:.3g}")
        np.testing.assert_allclose(got[k], w, rtol=rtol, atol=atol_scale * scale, err_msg=f"{tag} grad {k}")


def one_view(c, b, input_keys, camera_keys=("camera",)):
    """View b of a case as a case of its own."""
    one = dict(c, **{k: (c[k][b:b + 1] if c[k] is not None else None) for k in input_keys},
               upstream={k: u[b:b + 1] for k, u in c["upstream"].items()}, shape=(1, *c["shape"][1:]))
    for cam in camera_keys:
        one[cam] = dict(c[cam], **{k: c[cam][k][b:b + 1] for k in ("eye", "at", "up")})
    return one


def assert_bit_identical(a, b, rows=slice(None)):
    """Two (values, gradients) pairs of dicts of arrays agree exactly: `rows` of the first with the whole second."""
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(x[k][rows], y[k]), k
