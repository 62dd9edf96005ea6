"""GPU: the key confirmation of the binned finish rounds (srh_binned.h, render_binned_body).  A round confirms its 64
pixels' FRONT key as straight-line code for the whole wave -- a queued pixel has one, nothing is confirmed yet and every
key reaches -- and runs the second and third keys only when a ballot says that some lane's second key still reaches the
depth its front key confirmed.  The fourth key is a bound: where it reaches, the pixel goes to the slow path (one or two
pixels of a round) or the lane-parallel re-sweep (more).

Every case compares mode="binned" with mode="exact" bit for bit on image, depth and nearest, with one wave per tile and
with four.  The scenes are aimed at each way through the round: nobody needs a second key; some lanes do and others do
not; a third key; a front candidate that misses in fp64 with something or nothing behind it; five candidates within the
keys' resolution; rounds with dead lanes; near <= 0 (no candidate carries a depth estimate); row slabs; the render stage
alone; and the other primitive types' kernels, which share the body.  What a scene claims about depths is checked on the
CPU with the numpy oracle's own intersection.

The camera of every disc scene is synthetic.disk_cloud_scene's: eye (0, 0, 4) looking down -z, fovy 45 degrees."""
import numpy as np
import pytest
import torch

from test_hip_finish_tables import check, frames, one_type

pytestmark = pytest.mark.gpu

EYE = np.array([0.0, 0.0, 4.0])
CLOSE = 2.0 ** -18                     # relative depth difference the keys cannot tell apart (16-21 mantissa bits + margins)
WPTS = (1, 4)


def _at(c, r, z, width, height):
    """world point at depth z on the ray of pixel (c, r) (fractional pixels allowed)"""
    hh = np.tan(np.deg2rad(45.0) / 2.0)
    ww = hh * width / height
    s = EYE[2] - np.asarray(z, np.float64)
    x = (2.0 * np.asarray(c, np.float64) / (width - 1) - 1.0) * ww
    y = (1.0 - 2.0 * np.asarray(r, np.float64) / (height - 1)) * hh
    return np.stack(np.broadcast_arrays(s * x, s * y, EYE[2] - s), axis=-1)


def _pitch(z, width, height):
    """world size of one pixel at depth z"""
    return 2.0 * np.tan(np.deg2rad(45.0) / 2.0) * width / height / (width - 1) * (EYE[2] - z)


def _scene(pos, nrm, rad, width, height, near=0.1, far=1000.0):
    from surf_renderer_amd import synthetic
    scene = synthetic.disk_cloud_scene(4, width, height)
    n = len(rad)
    scene["camera"]["near"], scene["camera"]["far"] = near, far
    scene["objects"]["disk"] = {
        "pos": np.concatenate([np.asarray(pos, np.float64).reshape(n, 3), np.ones((n, 1))], axis=1).astype(np.float32),
        "normal": np.concatenate([np.asarray(nrm, np.float64).reshape(n, 3), np.zeros((n, 1))], axis=1).astype(np.float32),
        "radius": np.asarray(rad, np.float32),
        "material_idx": np.zeros(n, dtype=np.int64)}
    return scene


def disc_depths(scene):
    """(M, H, W) fp64 ray distance of every disc at every pixel as the reference computes it; inf where it misses or is clipped"""
    from oracle import np_oracle
    from surf_renderer_amd.scene import scene_to_numpy
    sc = scene_to_numpy(scene, round_fp32=True)
    eye, d, height, width = np_oracle.generate_rays(sc["camera"])
    g = sc["objects"]["disk"]
    with np.errstate(all="ignore"):
        t = np_oracle.hit_disk(eye, d, g["pos"], g["normal"], g["radius"])
        t[~((sc["camera"]["near"] <= t) & (t <= sc["camera"]["far"]))] = np.inf
    return t.reshape(-1, height, width)


def _equal(scene, rows=None):
    """binned == exact bit for bit, one wave per tile and four; returns the exact outputs"""
    want = None
    for wpt in WPTS:
        got, want = frames(scene, rows=rows, wpt=wpt)
        check(got, want, all_hit=False)
    return want


def _facing(n):
    return np.tile([0.0, 0.0, 1.0], (n, 1))


# ---- 1. plain: nobody needs a second key ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16), (48, 48), (37, 29)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_disc_over_the_whole_frame(size):
    scene = _scene([[0.0, 0.0, 0.5]], [[0.1, 0.2, 1.0]], [6.0], *size)
    image, depth, nearest = _equal(scene)
    assert np.isfinite(depth).all() and (nearest == 0).all()


# ---- 2. crossing discs: some lanes of a round need the second (third) key, others do not ----------------------------------
def crossing_scene(n_discs, size):
    """Discs through ONE point on the ray of the middle pixel of a tile, turned +-2e-3 about y (and, the third, about x):
    discs 0 and 1 meet along that pixel's column, all three at the pixel itself; one column away they are 2^-12 apart."""
    width, height = size
    c, r = (7, 8) if width == 16 else (23, 24)
    p = _at(c, r, 0.5, width, height)
    nrm = [[2e-3, 0.0, 1.0], [-2e-3, 0.0, 1.0], [0.0, 2e-3, 1.0]][:n_discs]
    return _scene(np.tile(p, (n_discs, 1)), nrm, [6.0] * n_discs, width, height), (c, r)


def check_crossing(scene, n_discs, pix):
    t = disc_depths(scene)
    assert np.isfinite(t).all()
    c, r = pix
    rel01 = np.abs(t[0] - t[1]) / t[0]
    assert (rel01[:, c] < CLOSE).all()                     # the whole column needs the second confirmation
    assert (rel01[:, c + 1] > 2.0 ** -14).all() and (rel01[:, c - 1] > 2.0 ** -14).all()   # its neighbours do not
    if n_discs == 3:
        spread = (t.max(axis=0) - t.min(axis=0)) / t.min(axis=0)
        assert spread[r, c] < CLOSE                        # three candidates within the keys' resolution: q = 2 runs
        assert (spread[r, :c] > 2.0 ** -14).all()


@pytest.mark.parametrize("size", [(16, 16), (48, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n_discs", [2, 3])
def test_discs_crossing_inside_a_tile(n_discs, size):
    scene, pix = crossing_scene(n_discs, size)
    check_crossing(scene, n_discs, pix)
    image, depth, nearest = _equal(scene)
    assert len(np.unique(nearest)) == n_discs              # each disc is in front somewhere


# ---- 3. near miss: the front candidate misses in fp64 ---------------------------------------------------------------------
def _half_wall(width, height, z=-1.0):
    """a facing disc behind everything that covers the upper rows of the frame only"""
    centre = _at((width - 1) / 2.0, -20.0, z, width, height)
    return centre, (20.0 + height / 2.0 - 0.3) * _pitch(z, width, height)


def huge_rim_scene(size):
    """The adversarial scenes' recipe: a slanted disc with centre (R, 0, 0.5) and radius R = 2^40, whose rim passes
    through the view along x = 0.  |p - c|^2 and r^2 agree to 2^-36 at every pixel of the frame, far inside what an fp32
    reject record can decide, so every pixel keeps the disc as a candidate and fp64 decides: the left half misses.
    Behind it a wall over the upper rows only: a miss finds the wall, or nothing."""
    width, height = size
    R = 2.0 ** 40
    wc, wr = _half_wall(width, height)
    return _scene([[R, 0.0, 0.5], wc], [[0.0, 0.3, 1.0], [0.0, 0.0, 1.0]], [R, wr], width, height)


def thin_rim_scene(size):
    """A disc seen almost edge-on (normal (1, 0, 0.1)): a sliver about one pixel wide down the middle columns, whose two
    rims pass within a few hundredths of a pixel of the pixel centres; in front of the same half wall."""
    width, height = size
    c = (width - 1) / 2.0
    wc, wr = _half_wall(width, height)
    return _scene([_at(c, (height - 1) / 2.0, 0.5, width, height), wc], [[1.0, 0.0, 0.1], [0.0, 0.0, 1.0]], [1.0, wr],
                  width, height)


def check_near_miss(scene, huge):
    t = disc_depths(scene)
    hit0, hit1 = np.isfinite(t[0]), np.isfinite(t[1])
    assert hit0.any() and (hit0 & hit1).any()
    assert (~hit0 & hit1).any() and (~hit0 & ~hit1).any()  # a miss with the wall behind it, and with nothing
    assert (t[0][hit0 & hit1] < t[1][hit0 & hit1]).all()  # where the front disc hits, it is in front
    if huge:
        # every pixel's plane hit lies within 2^-36 (relative, squared) of the rim: 2 |x| / R with |x| < 4
        from oracle import np_oracle
        from surf_renderer_amd.scene import scene_to_numpy
        sc = scene_to_numpy(scene, round_fp32=True)
        eye, d, _, _ = np_oracle.generate_rays(sc["camera"])
        g = sc["objects"]["disk"]
        tp = np_oracle.hit_plane(eye, d, g["pos"][:1], g["normal"][:1])
        q = (eye[None, :] + tp[0][:, None] * d.T) - g["pos"][0][None, :]
        assert (np.abs(np.sum(q * q, axis=1) / g["radius"][0] ** 2 - 1.0) < 2.0 ** -36).all()


@pytest.mark.parametrize("size", [(16, 16), (40, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["huge", "thin"])
def test_front_candidate_misses_in_fp64(kind, size):
    scene = huge_rim_scene(size) if kind == "huge" else thin_rim_scene(size)
    check_near_miss(scene, kind == "huge")
    _equal(scene)


# ---- 4. five candidates: the sentinel reaches ------------------------------------------------------------------------------
STACK_PIXELS = [(5, 5), (9, 6), (12, 7)]                    # one round of the one-wave kernel (tile rows 4-7)


def stack_scene(n_stacks, radius_px, size=(16, 16)):
    """Per stack five facing discs on one pixel's ray, one fp32 step (2^-24) apart in z: 2^-26 relative in depth.  A wall
    behind, so every other pixel of the tile takes the straight path in the same rounds."""
    width, height = size
    pos, rad = [], []
    for c, r in STACK_PIXELS[:n_stacks]:
        for k in range(5):
            z = 0.5 + k * 2.0 ** -24
            pos.append(_at(c, r, z, width, height))
            rad.append(radius_px * _pitch(z, width, height))
    pos.append([0.0, 0.0, -3.0])
    rad.append(60.0)
    return _scene(np.array(pos), _facing(len(rad)), rad, width, height)


def stacked_pixels(scene):
    """pixels where five or more discs lie within CLOSE of the nearest"""
    t = disc_depths(scene)
    return ((t - t.min(axis=0)) <= CLOSE * t.min(axis=0)).sum(axis=0) >= 5


@pytest.mark.parametrize("n_stacks,radius_px,pixels", [(1, 0.4, 1), (2, 0.4, 2), (3, 0.4, 3), (1, 3.0, None)],
                         ids=["one-pixel", "two-pixels", "three-pixels", "blob"])
def test_five_candidates_over_a_pixel(n_stacks, radius_px, pixels):
    """1 and 2 undecided pixels in a round: the wave-serial slow path.  3, and the 25-pixel blob: the re-sweep."""
    scene = stack_scene(n_stacks, radius_px)
    many = stacked_pixels(scene)
    if pixels is None:
        assert many[4:8].sum() > 2 and many[0:4].sum() > 2   # more than kSerialSlowMax in two rounds at least
    else:
        assert many.sum() == pixels and all(many[r, c] for c, r in STACK_PIXELS[:n_stacks])
    image, depth, nearest = _equal(scene)
    # ties and near-ties go to the fp64 minimum, the lowest index among equals: the stack's nearest disc is its LAST
    for i, (c, r) in enumerate(STACK_PIXELS[:n_stacks]):
        assert nearest[r, c] == 5 * i + 4


# ---- 5. other round shapes ---------------------------------------------------------------------------------------------------
def cloud_scene(size, near=0.1, n=120, seed=3):
    from surf_renderer_amd import synthetic
    from test_hip_finish_tables import wall
    scene = wall(synthetic.disk_cloud_scene(n, *size, radius=0.3, seed=seed))
    scene["camera"]["near"] = near
    return scene


@pytest.mark.parametrize("near", [0.0, -1.0])
def test_near_not_positive_confirms_every_candidate(near):
    """near <= 0: no pretest, every candidate carries kNoEstimate and every key reaches"""
    image, depth, nearest = _equal(cloud_scene((33, 20), near=near))
    assert np.isfinite(depth).all() and len(np.unique(nearest)) > 20


def dots_scene(n, size=(16, 16), seed=5):
    """n facing discs of 0.3 pixel radius, each on its own pixel's ray: a tile with exactly n hit pixels"""
    width, height = size
    rng = np.random.RandomState(seed)
    pix = rng.permutation(width * height)[:n]
    c, r = pix % width, pix // width
    z = rng.uniform(0.0, 1.0, n)
    return _scene(_at(c, r, z, width, height), _facing(n), 0.3 * _pitch(z, width, height), width, height), (c, r)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_rounds_with_dead_lanes(n):
    """1 and 63 queued pixels: one round with dead lanes; 65: a full round and a round of one"""
    scene, (c, r) = dots_scene(n)
    t = disc_depths(scene)
    assert np.isfinite(t).sum() == n and all(np.isfinite(t[i, r[i], c[i]]) for i in range(n))
    image, depth, nearest = _equal(scene)
    assert np.isfinite(depth).sum() == n


def test_row_slab():
    """rows 7-30 of the 48 x 48 crossing scene and of a 40 x 33 cloud: the slab starts and ends inside tile rows"""
    scene, _ = crossing_scene(3, (48, 48))
    _equal(scene, rows=(7, 30))
    _equal(cloud_scene((40, 33)), rows=(7, 30))


def test_render_stage_alone():
    from surf_renderer_amd import _lib, renderer
    scene = stack_scene(3, 0.4)
    buf = renderer.flatten_scene(scene, "cuda:0")
    cam = renderer.camera_struct(scene["camera"])
    want = [t.cpu().numpy() for t in renderer.render_buffers(buf, cam, mode="exact")]
    ws = buf.new_workspace(16, 16)
    for wpt in WPTS:
        out = renderer.render_buffers(buf, cam, mode="binned", workspace=ws, stages=_lib.STAGE_BIN, waves_per_tile=wpt)
        for t in out:
            t.fill_(-7)
        got = renderer.render_buffers(buf, cam, mode="binned", workspace=ws, out=out, stages=_lib.STAGE_RENDER,
                                      waves_per_tile=wpt)
        torch.cuda.synchronize()
        check([t.cpu().numpy() for t in got], want)


# ---- 6. the other kernels share the body -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shading", ["numpy", "torch"], ids=["lambert", "phong"])
@pytest.mark.parametrize("wpt", WPTS)
@pytest.mark.parametrize("kind", ["plane", "sphere", "triangle"])
def test_other_primitive_types(kind, wpt, shading):
    got, want = frames(one_type(kind, 16, 16), shading=shading, wpt=wpt)
    check(got, want)


# ---- 7. the ray's square root with and without its range guards ------------------------------------------------------------
@pytest.mark.parametrize("guards", [False, True], ids=["bounded-root", "guarded-root"])
def test_binned_equals_exact_with_either_square_root(guards):
    """The host sets bit 1 of the camera's ray flags (|D|^2 bounded: srh_device.h, sqrt_bounded) for this camera;
    SRH_ROOT_GUARDS in the environment clears it.  Both forms at 16 x 16, each against exact, bit for bit."""
    import ctypes as C
    import os
    from surf_renderer_amd import _lib, renderer
    scene = cloud_scene((16, 16), n=60)
    cam = renderer.camera_struct(scene["camera"])
    flags = C.c_int32(-1)
    if guards:
        os.environ["SRH_ROOT_GUARDS"] = "1"
    try:
        _lib.check(_lib.load().srh_camera_ray_flags(C.byref(cam), 0, C.byref(flags)))
        assert flags.value == (1 if guards else 3)
        image, depth, nearest = _equal(scene)
        for shading in ("numpy", "torch"):
            for wpt in WPTS:
                got, want = frames(one_type("disk", 16, 16), shading=shading, wpt=wpt)
                check(got, want)
    finally:
        os.environ.pop("SRH_ROOT_GUARDS", None)
    assert np.isfinite(depth).all()
