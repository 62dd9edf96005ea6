"""CPU: a numpy model of the coverage rule of the binned disc kernel's sorted sweep (srh_binned.h, sweep_sorted) on random
tiles.  Per disc U = 1 / (l - r) and V = 1 / (l + r) from its bounding ball (l = distance of the centre from the eye); the
list is swept by descending U in pairs, a pixel is covered once a swept disc hits it, and the first time every pixel of the
tile is covered the sweep stops at the first entry with U < min V of the entries swept so far.  The set of skipped entries
must never hold the winner (smallest t, then lowest index) of the all-pairs fp64 intersection at any pixel -- nor a tie."""
import numpy as np
import pytest

EYE = np.array([0.0, 0.0, 4.0])


def _rays(c0, r0, width=256, height=192):
    hh = np.tan(np.deg2rad(45.0) / 2.0)
    ww = hh * width / height
    c, r = np.meshgrid(np.arange(c0, c0 + 16), np.arange(r0, r0 + 16))
    d = np.stack([(2.0 * c / (width - 1) - 1.0) * ww, (1.0 - 2.0 * r / (height - 1)) * hh, -np.ones(c.shape)], axis=-1)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)


def _hits(pos, nrm, rad, rays):
    """t (discs, pixels) of the ray-disc intersection, inf where the ray misses"""
    k = np.einsum("ij,ij->i", pos - EYE, nrm)
    nd = nrm @ rays.T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = k[:, None] / nd
    q = EYE + t[..., None] * rays[None] - pos[:, None]
    ok = (np.einsum("ijk,ijk->ij", q, q) <= rad[:, None] ** 2) & (t > 0.1) & np.isfinite(t)
    return np.where(ok, t, np.inf)


def _swept(t, U, V):
    """number of entries of the sorted list the coverage rule evaluates"""
    n = len(U)
    order = np.argsort(-U, kind="stable")
    cov = np.zeros(t.shape[1], bool)
    vmin, stop, closed, i = np.inf, n, False, 0
    while i < stop:
        for e in order[i:min(i + 2, stop)]:
            cov |= np.isfinite(t[e])
            vmin = min(vmin, V[e])
        i += 2
        if not closed and i < stop and cov.all():
            closed = True
            below = np.nonzero(U[order] < vmin)[0]
            stop = min(stop, below[0] if len(below) else n)
    return order, min(stop, n)


@pytest.mark.parametrize("seed", range(12))
def test_skipped_entries_never_hold_a_winner(seed):
    rng = np.random.RandomState(seed)
    rays = _rays(128, 96)
    centre = EYE + 3.5 * rays[8 * 16 + 8]
    n = int(rng.choice([9, 24, 64, 128]))
    pos = centre + np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n), rng.uniform(-1.0, 1.0, n)], axis=1)
    nrm = rng.normal(scale=0.5, size=(n, 3)) + [0.0, 0.0, 1.0]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rad = rng.choice([0.02, 0.05, 0.2, 0.4], n)
    t = _hits(pos, nrm, rad, rays)
    l = np.linalg.norm(pos - EYE, axis=1)
    U, V = 1.0 / (l - rad), 1.0 / (l + rad)
    hit = np.isfinite(t)
    assert (1.0 / t[hit] <= np.broadcast_to(U[:, None], t.shape)[hit]).all()      # V <= 1 / t <= U for every hit
    assert (1.0 / t[hit] >= np.broadcast_to(V[:, None], t.shape)[hit]).all()
    order, stop = _swept(t, U, V)
    skipped = order[stop:]
    best = t.min(axis=0)
    if len(skipped):
        assert (t[skipped] > best[None]).all()             # strictly behind the winner at every pixel: no win, no tie
    assert np.array_equal(t[order[:stop]].min(axis=0), best)


def test_the_model_does_skip_entries():
    """A facing disc over the whole tile in front of a cloud: the rule stops right after the cover's pair."""
    rng = np.random.RandomState(99)
    rays = _rays(128, 96)
    centre = EYE + 3.5 * rays[8 * 16 + 8]
    n = 40
    pos = centre + np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-1.5, -0.5, n)], axis=1)
    pos[0] = centre
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))
    rad = np.full(n, 0.03)
    rad[0] = 0.3
    t = _hits(pos, nrm, rad, rays)
    l = np.linalg.norm(pos - EYE, axis=1)
    order, stop = _swept(t, 1.0 / (l - rad), 1.0 / (l + rad))
    assert order[0] == 0 and stop == 2
