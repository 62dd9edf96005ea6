"""Scenes that drive the three fp32 power functions of the kernels off their everyday operating point (gamma 0.8, pixel
values of order one): tonemap_f32 / tonemap_zero / spec_pow_f32 (csrc/srh_device.h) and tonemap_slope
(csrc/srh_backward.h).  Each of them evaluates x ** e as exp2(e * log2 x) on the hardware while |e * log2 x| <= 12 and
calls a library pow outside that range, so a test only sees both branches if its pixel values straddle the switch.

``ladder_scene``  pixel values from 1e-31 to 1e15 (and exact zeros) under any gamma: the tonemap and its slope.
``lobe_scene``    one sphere per specular exponent, the reflected ray sweeping [0, 1]: the Phong lobe.

tests/test_pow_scenes_cpu.py asserts, with the CPU oracles alone, that the scenes reach every branch; the GPU tests in
tests/test_hip_pow_paths.py then compare the kernels with the oracles on them.
"""
import copy

import numpy as np

from oracle import np_oracle_tch

GAMMAS = (0.25, 1 / 2.2, 0.8, 1.0, 1.5, 2.2, 4.0)
EXPONENTS = (0, 0.5, 1, 5, 20, 64, 200, 1000)
SWITCH = 12.0                        # |e * log2 x| above which the kernels leave the hardware log2 / exp2 path


def _f32(a):
    """float64 array holding fp32-representable values (what the device arrays will hold)."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def without_tonemap(scene):
    sc = copy.deepcopy(scene)
    sc.pop("tonemap", None)
    return sc


# ---- the ladder --------------------------------------------------------------------------------------------------------
LADDER_W, LADDER_H, LADDER_NX, LADDER_NY = 64, 48, 16, 12


def ladder_scene(gamma, lo=None, hi=None, shading="numpy", light_colour=1.0):
    """64 x 48 frame, eye (0, 0, 4) looking down -z at a 16 x 12 grid of camera-facing discs on z = 0.  Disc m sits on
    the ray of pixel (4i + 1, 4j + 1) and covers that pixel's 3 x 3 neighbourhood; the fourth row and column of every
    4 x 4 block stay background (7/16 of the frame).  One white light, one material per disc:
    albedo[m] = 10 ** e_m * (1, 0.5, 0.25), e_m evenly spaced over [lo, hi], albedo[0] = 0 exactly.  With n.l between
    0.78 and 0.98 the pixel values before the tonemap therefore run from 2e-31 to 1e15 at the defaults lo = -30 and
    hi = min(15, 30 / gamma) (x ** gamma stays finite in fp32), plus 27 exact zeros.
    shading='torch' adds coeffs (1, 0, 0), attenuation (1, 0, 0) and a zero ambient term: the same pixel values
    through the Phong path.  ``gamma=None`` leaves the tonemap out."""
    if lo is None:
        lo = -30.0
    if hi is None:
        hi = min(15.0, 30.0 / gamma) if gamma is not None and gamma > 0 else 15.0
    W, H = LADDER_W, LADDER_H
    fovy = float(np.deg2rad(45.0))
    half_h = np.tan(fovy / 2) * 4.0                       # half extent of the frame on the plane z = 0
    half_w = half_h * W / float(H)
    xs = np.linspace(-1, 1, W) * half_w
    ys = np.linspace(1, -1, H) * half_h
    n = LADDER_NX * LADDER_NY
    pos = np.zeros((n, 4))
    for m in range(n):
        i, j = m % LADDER_NX, m // LADDER_NX
        pos[m] = [xs[4 * i + 1], ys[4 * j + 1], 0.0, 1.0]
    step = min(xs[1] - xs[0], ys[0] - ys[1])
    e = np.linspace(lo, hi, n)
    albedo = (10.0 ** e)[:, None] * np.array([1.0, 0.5, 0.25])[None, :]
    albedo[0] = 0.0
    scene = {
        "camera": {"proj_type": "perspective", "viewport": [0, 0, W, H], "fovy": fovy, "focal_length": 1.0,
                   "eye": [0.0, 0.0, 4.0, 1.0], "up": [0.0, 1.0, 0.0, 0.0], "at": [0.0, 0.0, 0.0, 1.0],
                   "near": 0.1, "far": 1000.0},
        "lights": {"pos": _f32([[1.0, 2.0, 6.0, 1.0]]), "color_idx": np.array([1], dtype=np.int64)},
        "colors": _f32([[0, 0, 0], [light_colour] * 3]),
        "materials": {"albedo": _f32(albedo)},
        "objects": {"disk": {"pos": _f32(pos), "normal": _f32(np.tile([[0.0, 0.0, 1.0, 0.0]], (n, 1))),
                             "radius": _f32(np.full(n, 1.8 * step)),      # pixels at distance 1 and sqrt 2, not 2
                             "material_idx": np.arange(n, dtype=np.int64)}},
    }
    if gamma is not None:
        scene["tonemap"] = {"type": "gamma", "gamma": float(gamma)}
    if shading == "torch":
        scene["lights"]["attenuation"] = _f32([[1, 0, 0]])
        scene["lights"]["ambient"] = _f32([0, 0, 0])
        scene["materials"]["coeffs"] = _f32(np.tile([[1.0, 0.0, 0.0]], (n, 1)))
    else:
        assert shading == "numpy", shading
    return scene


# ---- the lobes ---------------------------------------------------------------------------------------------------------
LOBE_W, LOBE_H, LOBE_RADIUS = 128, 96, 0.4


def _rdotc(eye, d, centre, radius, light):
    """The Phong lobe's base for the ray eye + t d on a sphere, as np_oracle_tch._fragment_shader forms it (fp64)."""
    oc = eye - centre
    b = 2.0 * np.dot(oc, d)
    disc = b * b - 4.0 * np.dot(d, d) * (np.dot(oc, oc) - radius * radius)
    t = (-b - np.sqrt(disc)) / (2.0 * np.dot(d, d))
    p = eye + t * d
    fn = np_oracle_tch.unit3(p - centre)
    ldir = light - p
    ldir = ldir / np.sqrt(np.sum(ldir ** 2))
    refl = -2.0 * np.sum(-ldir * fn) * fn - ldir
    return float(np.sum(np_oracle_tch.unit3(eye - p) * refl))


def _bisect(f, a, b, target):
    """x in [a, b] with f(x) = target for a continuous f with f(a) - target and f(b) - target of opposite signs."""
    fa = f(a) - target
    assert fa * (f(b) - target) < 0
    for _ in range(200):
        mid = 0.5 * (a + b)
        fm = f(mid) - target
        if fa * fm <= 0:
            b = mid
        else:
            a, fa = mid, fm
    return 0.5 * (a + b)


def lobe_scene(exponents=EXPONENTS):
    """128 x 96 frame, shading='torch', eye (0, 0, 4): one sphere of radius 0.4 (about 400 pixels) per specular exponent
    in a grid of four columns, centred ON the ray of a pixel, material m with coeffs (0.5, 0.5, exponents[m]).
    Light 0 sits exactly at the eye: its reflected ray meets the view direction (rdotc = 1) at each sphere's centre pixel
    and leaves it (rdotc = 0 after the relu) 45 degrees further out.  Light 1 is off-axis.  Gamma 0.8.

    The lobe switches to the library powf below rdotc = 2 ** (-12 / n): 6e-8 at n = 0.5 and 2.4e-4 at n = 1, intervals no
    pixel of a 400-pixel sphere lands in by chance.  So the x coordinate of light 1 (near 0, where fp32 resolves 1e-10) is
    solved for rdotc = 3e-8 at one pixel of the n = 0.5 sphere, and the radius of the n = 1 sphere for rdotc = 1e-4 at one
    of its pixels; the larger exponents reach both sides on their own (tests/test_pow_scenes_cpu.py checks all of them)."""
    W, H = LOBE_W, LOBE_H
    cols = 4
    rows = (len(exponents) + cols - 1) // cols
    camera = {"proj_type": "perspective", "viewport": [0, 0, W, H], "fovy": float(np.deg2rad(45.0)), "focal_length": 1.0,
              "eye": [0.0, 0.0, 4.0, 1.0], "up": [0.0, 1.0, 0.0, 0.0], "at": [0.0, 0.0, 0.0, 1.0],
              "near": 0.1, "far": 1000.0}
    eye, rays, _, _ = np_oracle_tch.generate_rays(camera)              # rays (3, H * W), unit
    pix = []
    pos = np.zeros((len(exponents), 4))
    for m in range(len(exponents)):
        c = (W // cols) * (m % cols) + W // (2 * cols)
        r = (H // rows) * (m // cols) + H // (2 * rows)
        d = rays[:, r * W + c]
        pos[m] = [*(eye + d * (4.0 / -d[2])), 1.0]                      # where the pixel's ray meets z = 0
        pix.append((c, r))
    pos = _f32(pos)
    radius = _f32(np.full(len(exponents), LOBE_RADIUS))
    light1 = _f32([0.0, 3.0, 2.0])

    def tune(m, offsets, f_of, a, b, target):
        """Solve f_of(pixel ray)(x) = target on [a, b] at the pixel of sphere m (given as offsets from its centre pixel)
        that is closest to the target at the middle of the interval, among those that bracket it."""
        best = None
        for dc, dr in offsets:
            f = f_of(rays[:, (pix[m][1] + dr) * W + pix[m][0] + dc])
            if (f(a) - target) * (f(b) - target) < 0:
                miss = abs(f(0.5 * (a + b)) - target)
                if best is None or miss < best[0]:
                    best = (miss, f)
        assert best is not None, f"no pixel of sphere {m} brackets rdotc = {target}"
        x = float(np.float32(_bisect(best[1], a, b, target)))
        return x, best[1](x)

    ring = [(dc, dr) for dr in range(-10, 11) for dc in range(-10, 11) if 3 <= np.hypot(dc, dr) <= 10]
    for m, n in enumerate(exponents):
        if n == 0.5:
            x, got = tune(m, ring, lambda d: (lambda x: _rdotc(eye, d, pos[m, :3], radius[m], np.array([x, *light1[1:]]))),
                          -0.1, 0.1, 3e-8)
            assert 0 < got < 2.0 ** (-SWITCH / n), got
            light1[0] = x
    for m, n in enumerate(exponents):                                   # after light 1 has its final place
        if n == 1:
            r_m, got = tune(m, ring, lambda d: (lambda r: _rdotc(eye, d, pos[m, :3], r, light1)),
                            0.9 * LOBE_RADIUS, 1.1 * LOBE_RADIUS, 1e-4)
            assert 0 < got < 2.0 ** (-SWITCH / n), got
            radius[m] = r_m
    return {
        "camera": camera,
        "lights": {"pos": _f32([[0.0, 0.0, 4.0, 1.0], [*light1, 1.0]]), "color_idx": np.array([1, 2], dtype=np.int64),
                   "attenuation": _f32([[1, 0, 0], [1, 0, 0]]), "ambient": _f32([0.01, 0.01, 0.01])},
        "colors": _f32([[0, 0, 0], [0.6, 0.5, 0.4], [0.3, 0.4, 0.5]]),
        "materials": {"albedo": _f32(np.tile([[0.8, 0.6, 0.5]], (len(exponents), 1))),
                      "coeffs": _f32([[0.5, 0.5, float(n)] for n in exponents])},
        "objects": {"sphere": {"pos": pos, "radius": radius, "material_idx": np.arange(len(exponents), dtype=np.int64)}},
        "tonemap": {"type": "gamma", "gamma": 0.8},
    }


def lobe_rdotc(scene, res, double_sided=False):
    """rdotc (L, H, W) after the relu, recomputed from np_oracle_tch.render's `normal` and `pos` outputs with the
    formulas of its fragment shader; NaN where nothing is hit."""
    far = scene["camera"]["far"]
    hit = res["depth"] <= far
    eye = np_oracle_tch.cam_vec(scene["camera"]["eye"])[:3]
    p, fn = res["pos"], res["normal"]
    lpos = np.asarray(scene["lights"]["pos"], dtype=np.float64)[:, :3]
    ldir = lpos[:, None, None, :] - p[None]
    ldir = ldir / np.sqrt(np.sum(ldir ** 2, axis=-1))[..., None]
    refl = -2 * np.sum(-ldir * fn[None], axis=-1)[..., None] * fn[None] - ldir
    cdir = np_oracle_tch.unit3(eye - p)
    rdotc = np.sum(cdir[None] * refl, axis=-1)
    if double_sided:
        rdotc = np.sign(np.sum(cdir * fn, axis=-1))[None] * rdotc
    return np.where(hit[None], np.maximum(rdotc, 0.0), np.nan)
