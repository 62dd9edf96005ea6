"""Discs on the edges that k_prep's record arithmetic guards (srh_reject.h): the reciprocals and roots of the reject
record, the depth estimate, the ball bound and the tile box are Newton-refined hardware seeds, each under a stated
margin.  Whatever they round to, the record must stay conservative -- so `binned` and `fast` must reproduce the all-pairs
fp64 mode bit for bit on scenes whose discs sit exactly where a margin is the only thing between a record and a lost hit.

Every scene holds 2000-3000 discs: ordinary filler plus the named groups of `edge_groups`.  The CPU test restates the
record's screen-space quantities in numpy (camera from the oracle's own lookat_inv) and asserts that every group
reaches the branch it is named for; the GPU tests compare the modes."""
import functools

import numpy as np
import pytest

from oracle import np_oracle

TWO20 = 1048576.0


def f32(a):
    return np.asarray(a, dtype=np.float32)


def _ulps(x, j):
    x = np.float32(x)
    for _ in range(abs(j)):
        x = np.nextafter(x, np.float32(np.inf if j > 0 else -np.inf))
    return float(x)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _camera(W, H, eye, at, fovy_deg=45.0, near=1.0, far=50.0):
    return {"viewport": [0, 0, W, H], "fovy": float(np.deg2rad(fovy_deg)), "focal_length": 1.0,
            "eye": [*map(float, eye), 1.0], "at": [*map(float, at), 1.0], "up": [0.0, 1.0, 0.0, 0.0],
            "near": float(near), "far": float(far)}


def pixel_basis(cam):
    """eye and the columns D0, Dc, Dr of the un-normalised ray direction D(c, r) = D0 + c Dc + r Dr, from the oracle's
    camera matrix (np_oracle.generate_rays builds the same grid)"""
    vp = cam["viewport"]
    W, H = vp[2] - vp[0], vp[3] - vp[1]
    focal = cam["focal_length"]
    h = np.tan(cam["fovy"] / 2) * 2 * focal
    w = h * (W / float(H))
    m = np_oracle.lookat_inv(eye=np.array(cam["eye"]), at=cam["at"], up=cam["up"])[:3, :3]
    sx = 2.0 / (W - 1) if W > 1 else 0.0
    sy = -2.0 / (H - 1) if H > 1 else 0.0
    D0 = m @ np.array([-w / 2, h / 2, -focal])
    return np.array(cam["eye"][:3], dtype=np.float64), D0, m @ np.array([sx * w / 2, 0, 0]), m @ np.array([0, sy * h / 2, 0]), m


def edge_groups(cam, unit=1.0, full=True):
    """name -> list of (pos, normal, radius).  `unit` scales every length (the far-away cameras look at far-away discs);
    full=False leaves out the groups that are tied to the near / far planes and the 2^20-pixel limit."""
    eye, D0, Dc, Dr, m = pixel_basis(cam)
    xh, yh, fwd = m[:, 0] / np.linalg.norm(m[:, 0]), m[:, 1], -m[:, 2]
    near, far = cam["near"], cam["far"]
    g = {}
    # seen 0.1 .. 1 degree from edge-on: the axis ratio of the image is about 1 / sin(angle), 512 at 0.112 degrees
    lo, hi = [], []
    for i, deg in enumerate([0.1, 0.104, 0.108, 0.111, 0.113, 0.116, 0.125, 0.15, 0.2, 0.35, 0.5, 0.7, 1.0]):
        for sgn in (-1.0, 1.0):
            p = eye + unit * (3.0 * fwd + 0.15 * (i % 3 - 1) * xh + 0.1 * sgn * yh)
            v = _unit(p - eye)
            wv = _unit(np.cross(v, yh))
            a = np.deg2rad(deg)
            (hi if deg < 0.112 else lo).append((p, sgn * np.sin(a) * v + np.cos(a) * wv, 0.3 * unit))
    g["edge_on_ratio_above_512"], g["edge_on_ratio_below_512"] = hi, lo
    # a disc as large as its distance, facing the eye, hides the whole scene: those are seen at a slant of 0.005, each
    # from another side, and cover a narrow band across the image instead
    def slant(i, p):
        v = _unit(p - eye)
        w1 = _unit(np.cross(v, yh))
        return np.cos(2.4 * i) * w1 + np.sin(2.4 * i) * np.cross(v, w1) - 0.005 * v
    # radii 1e-6 .. 1e3, facing the eye from behind the other discs
    g["radii_1e-6_to_1e3"] = [(eye + unit * (7.0 * fwd + 0.2 * np.cos(i) * xh + 0.2 * np.sin(i) * yh), -fwd + 0.3 * np.sin(2.0 * i) * xh,
                               unit * r) for i, r in enumerate(np.geomspace(1e-6, 1e3, 19))]
    # the eye inside the disc's ball, and within a few float32 steps outside it (|oc| - r against 2^-22 (|oc| + r))
    inside, outside = [], []
    for i, fac in enumerate([1.001, 1.5, 10.0]):
        p = f32(eye + unit * (2.0 * fwd + 0.1 * i * xh)).astype(np.float64)
        inside.append((p, slant(i, p), np.linalg.norm(p - eye) * fac))
    for i, j in enumerate([1, 2, 3, 4, 6, 8, 16, 64]):
        p = f32(eye + unit * (2.0 * fwd - 0.1 * i * xh)).astype(np.float64)
        outside.append((p, slant(i + 3, p), _ulps(np.linalg.norm(p - eye), -j)))
    g["eye_inside_ball"], g["eye_just_outside_ball"] = inside, outside
    # plane through the eye: n.pos - n.eye is exactly zero (normal (1, -2, 0) against an offset of (2, 1, z) halves), or
    # one float32 step of the position away from it
    e32 = f32(eye).astype(np.float64)
    thr = [(e32 + 0.5 * (np.array(cam["at"][:3]) - e32), [1.0, -2.0, 0.0], 0.4 * unit)]
    for j in (-1, 1):
        p = e32 + unit * np.array([1.5, -0.75, 0.0])
        p[2] = _ulps(p[2], j)
        thr.append((p, [0.0, 0.0, 1.0], 0.5 * unit))
    thr.append((e32 + unit * np.array([1.5, -0.75, 0.0]), [0.0, 0.0, 1.0], 0.5 * unit))
    g["plane_through_eye"] = thr
    # zero and non-finite normals and radii
    p0 = eye + unit * 3.0 * fwd
    g["zero_or_nonfinite"] = [(p0, [0, 0, 0], 0.3 * unit), (p0, [np.nan, 0, 1], 0.3 * unit), (p0, [np.inf, 0, 0], 0.3 * unit),
                              (p0, -fwd, 0.0), (p0 + 0.1 * unit * xh, -fwd, np.nan), (p0 + 5 * unit * fwd, -fwd, np.inf),
                              (p0 - 0.1 * unit * xh, -fwd, -0.3 * unit)]
    if not full:
        return g
    # balls touching the near and the far plane: |oc| -+ r within float32 steps of the clip distance (the certain-hit
    # test keeps 2^-20 (|oc| + r) away from either)
    nt, ft = [], []
    for i, j in enumerate([-40, -12, -4, -1, 0, 1, 4, 12, 40]):
        p = f32(eye + 3.0 * fwd + 0.05 * (i - 4) * xh).astype(np.float64)
        nt.append((p, slant(i + 11, p), _ulps(np.linalg.norm(p - eye) - near, j)))
        p = f32(eye + 30.0 * fwd + 0.5 * (i - 4) * xh).astype(np.float64)
        ft.append((p, -fwd + 0.2 * yh, _ulps(far - np.linalg.norm(p - eye), j)))
    g["ball_touches_near_plane"], g["ball_touches_far_plane"] = nt, ft
    # parallel to the image plane a disc projects to a circle wherever it is: centres 2^19 .. 2^21 pixels off-screen
    pitch = np.linalg.norm(Dc) if np.linalg.norm(Dc) > 0 else 1.0
    g["centre_2^20_pixels_off"] = [(eye + 2.0 * fwd + sgn * 2.0 * pitch * TWO20 * f * xh, fwd, 2.0 * pitch * 40.0 * f)
                                   for f in (0.5, 0.9, 0.999, 1.001, 1.1, 2.0) for sgn in (-1.0, 1.0)]
    return g


def build_scene(cam, n_total, seed, unit=1.0, full=True):
    rng = np.random.RandomState(seed)
    groups = edge_groups(cam, unit, full)
    special = [d for grp in groups.values() for d in grp]
    n = n_total - len(special)
    at = np.array(cam["at"][:3])
    pos = at + unit * rng.uniform(-1.5, 1.5, (n, 3))
    nrm = rng.normal(size=(n, 3))
    rad = unit * np.exp(rng.uniform(np.log(0.02), np.log(0.3), n))
    pos = np.concatenate([pos, [d[0] for d in special]])
    nrm = np.concatenate([nrm, [np.asarray(d[1], dtype=np.float64) for d in special]])
    rad = np.concatenate([rad, [d[2] for d in special]])
    order = rng.permutation(n_total)
    where, first = {}, n
    for name, grp in groups.items():
        where[name] = np.array([int(np.nonzero(order == first + i)[0][0]) for i in range(len(grp))])
        first += len(grp)
    disk = {"pos": f32(np.concatenate([pos, np.ones((n_total, 1))], 1)[order]),
            "normal": f32(np.concatenate([nrm, np.zeros((n_total, 1))], 1)[order]), "radius": f32(rad[order]),
            "material_idx": rng.randint(0, 3, n_total)}
    scene = {"camera": cam, "lights": {"pos": f32([[*(at + unit * np.array(l)), 1.0] for l in ([3, 4, 5], [-4, 2, 3])]), "color_idx": np.array([1, 2])},
             "colors": f32([[0, 0, 0], [.8, .5, .4], [.3, .6, .9]]),
             "materials": {"albedo": f32([[.5, .5, .5], [.9, .3, .2], [.2, .7, .4]])},
             "objects": {"disk": disk}, "tonemap": {"type": "gamma", "gamma": 0.8}}
    return scene, where


EYE, AT = (0.5, 0.25, 4.0), (0.0, 0.0, 0.0)
# name -> (camera, discs, seed, unit, full, rows)
SCENES = {
    "discs_64x64": (_camera(64, 64, EYE, AT), 2400, 1, 1.0, True, None),
    "discs_256x256": (_camera(256, 256, EYE, AT), 3000, 2, 1.0, True, None),
    "frame_7x1": (_camera(7, 1, EYE, AT), 2000, 3, 1.0, True, None),
    "slab_rows_16_48": (_camera(64, 64, EYE, AT), 2400, 4, 1.0, True, (16, 48)),
    # |eye| / (size of the scene) beyond 2^24: only the coordinate ALONG the offset is coarse in float32, so the camera
    # looks across it at discs 4 units away, one unit = 2^-26 of the offset
    "camera_1e6_away": (_camera(64, 64, (1e6, 0.0, 4 * 2.0 ** -6), (1e6, 0.0, 0.0), near=2.0 ** -6, far=1e30), 2000, 5, 2.0 ** -6,
                        False, None),
    "camera_1e10_away": (_camera(64, 64, (1e10, 0.0, 4 * 128.0), (1e10, 0.0, 0.0), near=128.0, far=1e30), 2000, 6, 128.0, False,
                         None),
}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    cam, n, seed, unit, full, rows = SCENES[name]
    scene, where = build_scene(cam, n, seed, unit, full)
    return scene, where, rows


def screen_quantities(scene):
    """Per disc, in fp64 from the fp32 inputs, what disk_reject_record derives: k, |oc|, r, the trust test, and the
    ellipse of the image (centre in pixels, semi-axes) where the conic is one."""
    cam, d = scene["camera"], scene["objects"]["disk"]
    eye, D0, Dc, Dr, _ = pixel_basis(cam)
    P = [D0, Dc, Dr]
    n_all = len(d["radius"])
    out = {k: np.full(n_all, np.nan) for k in ("k", "l", "r", "c0", "r0", "smin", "smax")}
    out["trusted"] = np.zeros(n_all, dtype=bool)
    isl = [1.0 / np.linalg.norm(p) if np.linalg.norm(p) > 0 else 0.0 for p in P]
    with np.errstate(all="ignore"):
        for i in range(n_all):
            v = d["normal"][i].astype(np.float64)
            ln = np.sqrt(np.sum(v * v))
            n = v[:3] / (ln if abs(ln) > 0 else 1.0)
            p = d["pos"][i, :3].astype(np.float64)
            k = np.dot(p, n) - np.dot(n, eye)
            oc = eye - p
            r2 = float(d["radius"][i]) ** 2
            out["k"][i], out["l"][i], out["r"][i] = k, np.sqrt(np.dot(oc, oc)), np.sqrt(r2)
            nu = [np.dot(n, pj) for pj in P]
            u = [oc * nu[j] + k * P[j] for j in range(3)]
            mu = [np.sum(np.abs(oc * nu[j]) + np.abs(k * P[j])) + np.sum(np.abs(eye)) * abs(nu[j]) for j in range(3)]
            au = [np.sum(np.abs(u[j])) for j in range(3)]
            T = np.zeros((3, 3))
            tmax = emax = 0.0
            for a in range(3):
                for b in range(a, 3):
                    T[a, b] = T[b, a] = np.dot(u[a], u[b]) - r2 * nu[a] * nu[b]
                    s = isl[a] * isl[b]
                    tmax = np.fmax(tmax, abs(T[a, b]) * s)
                    emax = np.fmax(emax, (mu[a] * au[b] + mu[b] * au[a] + np.sum(np.abs(u[a] * u[b])) + abs(r2 * nu[a] * nu[b])) * s)
            out["trusted"][i] = bool(np.isfinite(emax) and tmax * 16777216.0 > emax)
            det = T[1, 1] * T[2, 2] - T[1, 2] ** 2
            if not (T[1, 1] > 0 and det > 0 and np.isfinite(T).all()):
                continue
            c0 = -(T[2, 2] * T[0, 1] - T[1, 2] * T[0, 2]) / det
            r0 = -(T[1, 1] * T[0, 2] - T[1, 2] * T[0, 1]) / det
            F0 = T[0, 0] + T[0, 1] * c0 + T[0, 2] * r0
            if not F0 < 0:
                continue
            lam = np.linalg.eigvalsh(T[1:, 1:] / -F0)
            if not lam[0] > 0:
                continue
            out["c0"][i], out["r0"][i], out["smin"][i], out["smax"][i] = c0, r0, 1 / np.sqrt(lam[1]), 1 / np.sqrt(lam[0])
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_every_group_reaches_its_branch(name):
    scene, where, rows = scene_of(name)
    cam, d = scene["camera"], scene["objects"]["disk"]
    assert 2000 <= len(d["radius"]) <= 3000
    q = screen_quantities(scene)
    ratio = q["smax"] / q["smin"]
    near, far = cam["near"], cam["far"]

    w = where["edge_on_ratio_below_512"]
    if name.startswith("camera_1e"):
        # |eye| joins the terms the coefficients are measured against, and here it is 2^26 times the size of the scene:
        # no conic is trusted (a handful of discs whose own terms are huge -- radius 1e3 units -- aside)
        assert q["trusted"].mean() < 0.05 and np.abs(np.array(cam["eye"][:3])).max() in (1e6, 1e10), q["trusted"].mean()
    elif name != "frame_7x1":               # (one row: Dr = 0, the conic of every disc is degenerate in r)
        assert q["trusted"][w].all() and (ratio[w] <= 512).all() and (ratio[w] > 50).any(), ratio[w]
        assert ratio[w].max() > 400, ratio[w]                                   # right up to the switch
        w = where["edge_on_ratio_above_512"]
        assert (~(ratio[w] <= 512)).all(), ratio[w]                             # beyond it, or no ellipse at all
        assert np.nanmin(ratio[w]) < 650, ratio[w]
    w = where["radii_1e-6_to_1e3"]
    unit = SCENES[name][3]
    assert d["radius"][w].min() <= 1.01e-6 * unit and d["radius"][w].max() >= 990.0 * unit
    if name in ("discs_64x64", "discs_256x256", "slab_rows_16_48"):
        assert np.nanmin(q["smax"][w]) < 1e-3 and (q["l"][w] < q["r"][w]).any()  # far below a pixel .. the eye inside
    w = where["eye_inside_ball"]
    assert (q["l"][w] < q["r"][w]).all()
    w = where["eye_just_outside_ball"]
    gap = (q["l"][w] - q["r"][w]) / (q["l"][w] + q["r"][w])
    assert (gap > 0).all() and (gap < 2.0 ** -22).any() and (gap > 2.0 ** -22).any(), gap   # both sides of the bound's own slack
    w = where["plane_through_eye"]
    assert (q["k"][w] == 0).sum() >= 2 and (q["k"][w] != 0).sum() >= 2 and (np.abs(q["k"][w]) < 1e-5 * unit).all(), q["k"][w]
    w = where["zero_or_nonfinite"]
    bad = ~np.isfinite(d["normal"][w]).all(axis=1) | ~np.isfinite(d["radius"][w]) | (d["radius"][w] == 0) | \
        (d["normal"][w] == 0).all(axis=1) | (d["radius"][w] < 0)
    assert bad.all()
    if SCENES[name][4]:
        for key, edge in (("ball_touches_near_plane", q["l"] - q["r"] - near), ("ball_touches_far_plane", far - q["l"] - q["r"])):
            w = where[key]
            rel = edge[w] / (q["l"][w] + q["r"][w])
            # on both sides of the plane, inside and outside the 2^-20 (|oc| + r) the certain-hit test keeps clear
            assert (rel > 2.0 ** -20).any() and (rel < -(2.0 ** -20)).any() and (np.abs(rel) < 2.0 ** -20).sum() >= 3, (key, rel)
        if name != "frame_7x1":
            w = where["centre_2^20_pixels_off"]
            off = np.abs(q["c0"][w])
            assert (off < TWO20).sum() >= 4 and (off > TWO20).sum() >= 4 and (off > 0.4 * TWO20).all(), off
            assert (np.abs(off / TWO20 - 1) < 0.01).sum() >= 4, off


@functools.lru_cache(maxsize=None)
def _exact(name):
    return _render(name, "exact")


def _render(name, mode):
    import torch
    from surf_renderer_amd import render
    scene, _, rows = scene_of(name)
    kw = {} if rows is None else {"rows": rows}
    res = render(scene, device="cuda:0", mode=mode, **kw)
    torch.cuda.synchronize()
    return {k: res[k].clone() for k in ("image", "depth", "nearest")}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["binned", "fast"])
@pytest.mark.parametrize("name", list(SCENES))
def test_modes_equal_exact(name, mode):
    import torch
    ref, got = _exact(name), _render(name, mode)
    hit = int((ref["depth"] < 3e38).sum())
    print(f"{name} {mode}: {hit} of {ref['depth'].numel()} pixels hit")
    assert hit > 0
    for k in ("nearest", "depth", "image"):
        assert torch.equal(got[k], ref[k]), f"{name} {mode}: {k} differs on {int((got[k] != ref[k]).sum())} values"
