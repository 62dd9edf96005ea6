"""Seeded inputs for the tests of the frame transforms and the point projection (tests/test_hip_frames.py on the GPU,
tests/test_frames_oracle_cpu.py here) and for tools/gen_frames_golden.py, which records the reference on them.

N is free in these layers, so it is chosen directly, at the sizes at which the kernels can break:
    1        a single lane
    153      a partial wave
    192      three full waves
    1728     seven workgroups: the finish kernel adds more than one partial
    16896    66 workgroups: a finish row adds a second partial before its tree
B is in {1, 2, 3}; 3 is the size at which the reference's torch.cross quirk appears (oracle/ref_harness.run_views).

A transform case (TRANSFORM) is a dict: `pos` [B, N, 3|4] and `normal` [B, N', 3|4] fp32, either None; `camera` (eye /
at / up, [B, 3] or [B, 4]); `upstream` {'pos': [B, N, 4], 'normal': [B, N', 3]} for the inputs that are there.  It is
used in both directions (frames_oracle.TRANSFORMS).  The fourth column of a position is drawn from [0.5, 2]; the fourth
column of a normal is not read.

A projection case (PROJECT) is a dict: `surfels` [B, N, 3|4], the full pinhole `camera`, `upstream` {'plane', 'px_coord'}
[B, N, 3] for project_surfels and project_image_coordinates.  The frames are 5x3, 16x12 and 48x36 (W x H).  Each surfel
is aimed at a pixel coordinate; of every 16 surfels (N >= 16) two are aimed outside the frame on each of its four sides
and two lie behind the camera.  A surfel with w != 1 is moved so that [R | t] [p, w] still is the aimed point.

Rounding boundaries: px_coord - 0.5 from the fp64 oracle (of the fp32 inputs) is kept at least 1e-3 px away from every
k + 0.5, k an integer (the frame's edges -0.5 and W - 0.5 / H - 0.5 are such values) -- a surfel closer than that is
drawn again.  Float32 evaluation moves a coordinate of magnitude <= 60 px by about 1e-5, so the reference's float32
and float64 indices and the oracle's agree on every surfel; tests/test_frames_oracle_cpu.py asserts that on the
fixtures.

GOLDEN_* list the cases the reference is recorded on: those of up to 192 points.  A fixture of 1728 points or more,
with its float64 values and gradients, would be several times the size the largest fixture of the sibling layers has
(tests/test_frames_oracle_cpu.py holds them to that), and more points exercise nothing in the reference's arithmetic
that 192 do not: the larger sizes are there for the kernels' reduction."""
import functools

import numpy as np
import torch

import frames_oracle as fo
import projection_cases as pc

_T_SPEC = {  # B, n_pos, n_normal (None = absent), pos columns, normal columns, homogeneous camera
    "t1": (1, 1, 1, 3, 3, False),
    "t153_192": (2, 153, 192, 4, 4, False),
    "t192_pos": (1, 192, None, 3, 3, False),
    "t153_normal": (1, None, 153, 3, 3, False),
    "t153_b3": (3, 153, 153, 4, 3, True),
    "t1728": (1, 1728, 1728, 3, 4, False),
    "t16896": (2, 16896, 16896, 4, 3, True),
}
_P_SPEC = {  # B, N, W, H, columns, homogeneous camera
    "p1_5x3": (1, 1, 5, 3, 3, False),
    "p153_5x3": (2, 153, 5, 3, 4, False),
    "p192_16x12": (3, 192, 16, 12, 3, True),
    "p1728_48x36": (1, 1728, 48, 36, 3, False),
    "p16896_16x12": (2, 16896, 16, 12, 4, False),
}
TRANSFORM, PROJECT = tuple(_T_SPEC), tuple(_P_SPEC)
DIRECTIONS = tuple(fo.TRANSFORMS)
GOLDEN_TRANSFORM = tuple(n for n in TRANSFORM if n not in ("t1728", "t16896"))
GOLDEN_PROJECT = tuple(n for n in PROJECT if n not in ("p1728_48x36", "p16896_16x12"))
MARGIN = 1e-3          # px, from every rounding boundary


def camera_vectors(rng, B, hom):
    """eye / at / up [B, 3], or [B, 4] under the reference's w conventions with w values that are not 1: the w column is
    dropped without dividing."""
    eye, at, up = pc.draw_camera(rng, B)
    if hom:
        eye = np.concatenate((eye, np.full((B, 1), 2.0, np.float32)), -1)
        at = np.concatenate((at, np.full((B, 1), 0.5, np.float32)), -1)
        up = np.concatenate((up, np.zeros((B, 1), np.float32)), -1)
    return {"eye": eye, "at": at, "up": up}


@functools.lru_cache(maxsize=None)
def transform_case(name):
    B, n_pos, n_normal, pos_cols, normal_cols, hom = _T_SPEC[name]
    rng = np.random.RandomState(9100 + TRANSFORM.index(name))
    c = {"camera": camera_vectors(rng, B, hom), "pos": None, "normal": None, "upstream": {}}
    if n_pos is not None:
        pos = rng.uniform(-2.0, 2.0, (B, n_pos, pos_cols))
        if pos_cols == 4:
            pos[..., 3] = rng.uniform(0.5, 2.0, (B, n_pos))
        c["pos"] = pc.f32(pos)
        c["upstream"]["pos"] = pc.f32(rng.uniform(-1, 1, (B, n_pos, 4)))
    if n_normal is not None:
        c["normal"] = pc.f32(rng.uniform(-1.0, 1.0, (B, n_normal, normal_cols)))
        c["upstream"]["normal"] = pc.f32(rng.uniform(-1, 1, (B, n_normal, 3)))
    return c


def transform_inputs(c):
    return {k: c[k] for k in ("pos", "normal")}


def _aimed(rng, cam3, W, H, n, kind, w):
    """fp32 surfels [n, 3|4] of one view, aimed by `kind` (0-1 left, 2-3 right, 4-5 above, 6-7 below the frame, 8-9
    behind the camera, else inside) at a pixel coordinate, with fourth column `w` (None = three columns)."""
    eye, at, up = (cam3[k][None] for k in ("eye", "at", "up"))
    px, py = rng.uniform(0.0, W, (1, n)), rng.uniform(0.0, H, (1, n))
    out = rng.uniform(0.6, 0.25 * max(W, 4), (1, n))
    px = np.where(kind < 2, -out, np.where(kind < 4, W + out, px))
    py = np.where((kind >= 4) & (kind < 6), -out, np.where((kind >= 6) & (kind < 8), H + out, py))
    z = rng.uniform(1.5, 3.0, (1, n)) * np.where((kind >= 8) & (kind < 10), -1.0, 1.0)
    p = pc.lift(px, py, z, eye, at, up, W, H)[0]
    if w is None:
        return pc.f32(p)
    p = p + (w[:, None] - 1.0) * eye[0].astype(np.float64)          # [R | t] [p, w] = R q + t for the aimed point q
    return pc.f32(np.concatenate((p, w[:, None]), -1))


def boundary_distance(surfels, camera):
    """[B, N]: the distance in px of (px_coord - 0.5)'s x and y from the nearest k + 0.5, by the fp64 oracle."""
    _, px = fo.project_image_coordinates(torch.as_tensor(np.asarray(surfels, dtype=np.float64)), camera)
    t = px[..., :2].numpy() - 0.5
    return np.abs((t - 0.5) - np.round(t - 0.5)).min(-1)


@functools.lru_cache(maxsize=None)
def project_case(name):
    B, N, W, H, cols, hom = _P_SPEC[name]
    rng = np.random.RandomState(9200 + PROJECT.index(name))
    cam = camera_vectors(rng, B, hom)
    camera = dict(cam, viewport=[0, 0, W, H], fovy=float(pc.FOVY), focal_length=pc.FOCAL)
    kind = (np.arange(N) % 16) if N >= 16 else np.full(N, 15)
    surfels = np.zeros((B, N, cols), np.float32)
    for b in range(B):
        cam3 = {k: v[b, :3] for k, v in cam.items()}
        todo = np.arange(N)
        for _ in range(64):
            w = rng.uniform(0.5, 2.0, len(todo)) if cols == 4 else None
            surfels[b, todo] = _aimed(rng, cam3, W, H, len(todo), kind[todo][None], w)
            one = dict(camera, **{k: v[b:b + 1] for k, v in cam.items()})
            todo = np.nonzero(boundary_distance(surfels[b:b + 1], one)[0] < MARGIN)[0]
            if not len(todo):
                break
        else:
            raise RuntimeError(f"{name}: no draw is clear of every rounding boundary")
    return {"surfels": surfels, "camera": camera, "frame": (W, H),
            "upstream": {"plane": pc.f32(rng.uniform(-1, 1, (B, N, 3))), "px_coord": pc.f32(rng.uniform(-1, 1, (B, N, 3)))}}


@functools.lru_cache(maxsize=None)
def transform_expected(name, direction):
    """(values, gradients, camera gradients) from the fp64 oracle, computed once."""
    c = transform_case(name)
    return fo.transform_gradients(direction, transform_inputs(c), c["camera"], c["upstream"])


@functools.lru_cache(maxsize=None)
def project_expected(name, coords):
    c = project_case(name)
    key = "px_coord" if coords else "plane"
    return fo.project_gradients(coords, c["surfels"], c["camera"], {key: c["upstream"][key]})


@functools.lru_cache(maxsize=None)
def transform_magnitudes(name, direction):
    """The oracle's sums of |terms| per entry of transform_expected (tests/entry_checks.py), computed once."""
    c = transform_case(name)
    return fo.transform_magnitudes(direction, transform_inputs(c), c["camera"], c["upstream"])


@functools.lru_cache(maxsize=None)
def project_magnitudes(name, coords):
    c = project_case(name)
    key = "px_coord" if coords else "plane"
    return fo.project_magnitudes(coords, c["surfels"], c["camera"], {key: c["upstream"][key]})
