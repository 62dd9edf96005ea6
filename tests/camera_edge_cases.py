"""Which edge inputs the camera gradients (camera_grad=True, the kView kernels) are held on, and what the fp64
restatements with camera leaves say about them: tests/test_camera_edge_cases_cpu.py here, tests/test_hip_camera_edges.py
on the GPU.  A thin module: the inputs are the existing edge dicts (surfels_edge_cases, dense_projection_edge_cases,
normals_edge_cases, splat_edge_scenes, splats_ndc_edge_cases), the expected values come from camera_chain_oracle,
dense_camera_oracle, splat_camera_oracle and frames_oracle.  What is drawn here, deterministically: special_finite_3x3,
the dense zdepth_9x7,
the frame cases (there is no edge module for the frame transforms and the point projection) and the poisoned batches.

    case(layer, name, variant=None)       the input dict, in the layout of the layer's own case module
    expected(layer, name, variant=None)   (values, gradients, camera gradients {'eye', 'at', 'up'}) of the restatement
    second(layer, name, variant=None)     the camera gradients again, summed in another order (see below)

Layers and variants
    lift        LIFT; world frame
    dense       DENSE: name with (layout, rotated) as the variant
    normals     NORMALS: every normals_edge_cases name with frame 'world'
    along_ray   all 24 of splat_edge_scenes.CASES with upstream(scene, kwargs)['image']; values and gradients are
    ndc         splats_ndc_edge_cases.NAMES                    None (the camera enters through the image alone)
    transform   TRANSFORM, variant 'to_cam' / 'to_world' (frames_cases' dict layout)
    project     PROJECT, variant False / True (project_surfels / project_image_coordinates)
    poisoned    POISONED: B = 3, view 1 non-finite, views 0 and 2 ordinary with their own cameras, at least two
                workgroups per view; case() gives the layer's dict, poisoned_layer(name) the layer it belongs to

Frame cases
    counts_1_257, counts_257_1   B = 2, n_pos != n_normal: one half is a single lane, the other a second workgroup with
                                 one live lane
    b5_n1                        five views of one point and one normal
    w0_153                       B = 2, four-column points whose w is exactly 0 in every eighth row (W0_ROWS): such a row
                                 brings nothing to column 3 of d loss / d view_pos
    zdepth_9x7 (dense)           see _dense_zdepth: the one dense case with surfels at Z = 0, which the edge module
                                 keeps away from
    zdepth_16x12                 B = 1, N = 192 on 16 x 12: eye (0, 0, 4), at the origin, up (0, 1, 0), and every 16th
                                 surfel (ZDEPTH_ROWS) with z = 4, so that its camera-space Z is exactly 0 in fp64 (the row
                                 of the matrix is (0, 0, s) and s * 4 is exact).  Every surfel, the named ones included,
                                 keeps frames_cases.MARGIN from the rounding boundaries

The second summation order.  A camera gradient is a sum over the points; whether an entry of it is more than the
rounding noise of that sum is decided here, from the restatement alone: second() evaluates the same function with the
points in reversed order -- lift: the pixel grid, depths and upstream reversed; dense, transform, project: the surfels /
points reversed; normals: the map turned by 180 degrees, which maps the stencil onto itself.  The two splat renderers
tie a splat to its pixel's ray and cannot be reordered without restating them, so for them the upstream image is split
into its first and second half of the pixels and the two camera gradients are added: linear in the upstream, another
order of the same sum.  noise(layer, name, variant) lists the entries whose two values differ by more than 1e-7
relative."""
import functools
from unittest import mock

import numpy as np

import camera_chain_oracle as co
import dense_camera_oracle as dco
import dense_projection_edge_cases as de
import dense_projection_oracle as do
import frames_cases as fc
import frames_oracle as fo
import normals_cases as nc
import normals_edge_cases as ne
import normals_oracle as no
import projection_cases as pc
import splat_camera_oracle as sco
import splat_edge_scenes as se
import splats_ndc_edge_cases as sne
import surfels_edge_cases as su
import surfels_oracle as so

KEYS = co.CAMERA_KEYS
LIFT = ("row_1x300", "column_300x1", "b5_1x1", "special_3x3", "special_finite_3x3")
DENSE = [(n, "grid", False) for n in de.NAMES] + \
    [(n, layout, rotated) for n in ("row_1x5", "far_9x7", "sigma_0p03_9x7")
     for layout, rotated in (("flat", False), ("grid", True), ("flat", True))] + [("zdepth_9x7", "grid", False)]
NORMALS = ne.NAMES
ALONG_RAY = se.CASES
NDC = sne.NAMES
TRANSFORM = ("counts_1_257", "counts_257_1", "b5_n1", "w0_153")
PROJECT = ("zdepth_16x12",)
POISONED = ("poisoned_lift", "poisoned_dense", "poisoned_normals", "poisoned_transform")
ALL = ([("lift", n, None) for n in LIFT] + [("dense", n, (layout, rotated)) for n, layout, rotated in DENSE] + [("normals", n, None) for n in NORMALS]
       + [("along_ray", n, None) for n in ALONG_RAY] + [("ndc", n, None) for n in NDC]
       + [("transform", n, d) for n in TRANSFORM for d in fc.DIRECTIONS] + [("project", n, c) for n in PROJECT for c in (False, True)]
       + [("poisoned", "poisoned_transform", d) for d in fc.DIRECTIONS]
       + [("poisoned", n, None) for n in POISONED if n != "poisoned_transform"])
# the restatement's camera gradient is non-finite in every entry (of view 1 for a poisoned batch)
NONFINITE = {("lift", "special_3x3"), ("normals", "nan_7x7"), ("normals", "inf_7x7"), ("normals", "big_7x7")}
# exactly zero by construction: both pixel scales of a 1 x 1 frame are 0; n = (0, 0, s) meets only the z column of the
# rotation, which does not depend on `up`
EXACT_ZERO = {("dense", "one_1x1"): KEYS, ("normals", "constant_4x4"): ("up",), ("normals", "vertical_plane_5x6"): ("up",)}
W0_ROWS = tuple(range(0, 153, 8))
ZDEPTH_ROWS = tuple(range(0, 192, 16))
DENSE_ZDEPTH_ROWS = (10, 40)
POISONED_VIEW = 1


def tag(layer, name, variant=None):
    if layer == "dense":
        return "dense " + de.tag(name, *variant)
    return f"{layer} {name}" + ("" if variant is None else f" {variant}")


def poisoned_layer(name):
    return name[len("poisoned_"):]


def _pinhole(eye, at, up, W, H):
    return {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY), "focal_length": pc.FOCAL}


# ---- the cases drawn here --------------------------------------------------------------------------------------------
def _special_finite():
    c = su.case("special_3x3")
    depth = c["depth"].copy()
    assert np.isinf(depth[0, 4]) and np.isnan(depth[0, 7])
    depth[0, 4], depth[0, 7] = 2.5, 1.75
    return dict(c, depth=depth)


def _dense_zdepth():
    """9 x 7, D = 3, sigma 0.9 under zdepth_16x12's camera; surfels DENSE_ZDEPTH_ROWS have z = 4, so Z is exactly 0 and
    k_dproj_surfel_bwd's `Q.Z != 0` decides their g_Z; every other surfel keeps Z_MARGIN."""
    B, H, W, D, sigma = 1, 9, 7, 3, 0.9
    rng = np.random.RandomState(9760)
    eye, at, up = pc.f32([[0.0, 0.0, 4.0]]), pc.f32([[0.0, 0.0, 0.0]]), pc.f32([[0.0, 1.0, 0.0]])
    px, py = pc.jittered_grid(rng, B, H, W, 1.2)
    surfels = pc.f32(pc.lift(px, py, rng.uniform(1.5, 3.0, (B, H * W)), eye, at, up, W, H))
    camera = _pinhole(eye, at, up, W, H)
    assert do.z_margin(surfels, camera) >= de.Z_MARGIN
    surfels[0, list(DENSE_ZDEPTH_ROWS)] = pc.f32([[0.05, -0.04, 4.0], [-0.08, 0.06, 4.0]])
    return {"surfels": surfels, "rgb": pc.f32(rng.uniform(0, 1, (B, H, W, D))), "rotated_image": None, "named": DENSE_ZDEPTH_ROWS,
            "camera": camera, "blur_size": float(np.float32(6 * sigma / W)), "shape": (B, H, W, D), "layout": "grid",
            "upstream": {"out": pc.f32(rng.uniform(-1, 1, (B, H, W, D))), "mask": pc.f32(rng.uniform(-1, 1, (B, H, W, 1)))}}


def _transform_case(name):
    B, n_pos, n_normal = {"counts_1_257": (2, 1, 257), "counts_257_1": (2, 257, 1), "b5_n1": (5, 1, 1),
                          "w0_153": (2, 153, 153)}[name]
    rng = np.random.RandomState(9700 + TRANSFORM.index(name))
    pos = rng.uniform(-2.0, 2.0, (B, n_pos, 4))
    pos[..., 3] = rng.uniform(0.5, 2.0, (B, n_pos))
    if name == "w0_153":
        pos[:, list(W0_ROWS), 3] = 0.0
    return {"camera": fc.camera_vectors(rng, B, False), "pos": pc.f32(pos),
            "normal": pc.f32(rng.uniform(-1.0, 1.0, (B, n_normal, 3))),
            "upstream": {"pos": pc.f32(rng.uniform(-1, 1, (B, n_pos, 4))), "normal": pc.f32(rng.uniform(-1, 1, (B, n_normal, 3)))}}


def _zdepth_case():
    W, H, N = 16, 12, 192
    rng = np.random.RandomState(9750)
    cam = {"eye": pc.f32([[0.0, 0.0, 4.0]]), "at": pc.f32([[0.0, 0.0, 0.0]]), "up": pc.f32([[0.0, 1.0, 0.0]])}
    camera = dict(cam, viewport=[0, 0, W, H], fovy=float(pc.FOVY), focal_length=pc.FOCAL)
    named = np.zeros(N, bool)
    named[list(ZDEPTH_ROWS)] = True
    kind = np.arange(N) % 16                 # the others as frames_cases aims them: outside on four sides, behind, inside
    surfels = np.zeros((1, N, 3), np.float32)
    todo = np.arange(N)
    for _ in range(64):
        drawn = fc._aimed(rng, {k: v[0] for k, v in cam.items()}, W, H, len(todo), kind[todo][None], None)
        flat = pc.f32(np.stack((rng.uniform(-0.3, 0.3, len(todo)), rng.uniform(-0.2, 0.2, len(todo)), np.full(len(todo), 4.0)), -1))
        surfels[0, todo] = np.where(named[todo][:, None], flat, drawn)
        todo = np.nonzero(fc.boundary_distance(surfels, camera)[0] < fc.MARGIN)[0]
        if not len(todo):
            break
    else:
        raise RuntimeError("zdepth_16x12: no draw is clear of every rounding boundary")
    return {"surfels": surfels, "camera": camera, "frame": (W, H),
            "upstream": {"plane": pc.f32(rng.uniform(-1, 1, (1, N, 3))), "px_coord": pc.f32(rng.uniform(-1, 1, (1, N, 3)))}}


def _poisoned(name):
    """B = 3; view POISONED_VIEW holds the layer's non-finite input."""
    layer = poisoned_layer(name)
    rng = np.random.RandomState(9800 + POISONED.index(name))
    B = 3
    if layer == "lift":                      # 1 x 300: two workgroups of 256; the specials in view 1's first nine pixels
        H, W = 1, 300
        depth = rng.uniform(1.5, 3.0, (B, H * W))
        depth[:, 16::8] = 0.0
        depth[:, 20::16] = -1.25
        depth = pc.f32(depth)
        depth[POISONED_VIEW, :9] = su.SPECIAL
        return {"depth": depth, "camera": _pinhole(*pc.draw_camera(rng, B), W, H), "frame": "world", "shape": (B, H, W),
                "upstream": {"pos": pc.f32(rng.uniform(-1, 1, (B, H * W, 3)))}}
    if layer == "dense":                     # 9 x 8: 72 surfels are two one-wave workgroups, the second with 8 live lanes
        H, W, D, sigma = 9, 8, 2, 0.9
        for _ in range(50):
            eye, at, up = pc.draw_camera(rng, B)
            px, py = pc.jittered_grid(rng, B, H, W, 1.2)
            surfels = pc.f32(pc.lift(px, py, rng.uniform(1.5, 3.0, (B, H * W)), eye, at, up, W, H))
            camera = _pinhole(eye, at, up, W, H)
            if do.z_margin(surfels, camera) >= de.Z_MARGIN:
                break
        else:
            raise RuntimeError("poisoned_dense: no draw is clear of Z = 0")
        surfels[POISONED_VIEW, 37, 1] = np.nan
        return {"surfels": surfels, "rgb": pc.f32(rng.uniform(0, 1, (B, H, W, D))),
                "rotated_image": pc.f32(rng.uniform(0, 1, (B, H, W, D))), "camera": camera,
                "blur_size": float(np.float32(6 * sigma / W)), "shape": (B, H, W, D), "layout": "grid",
                "upstream": {"out": pc.f32(rng.uniform(-1, 1, (B, H, W, D))), "mask": pc.f32(rng.uniform(-1, 1, (B, H, W, 1)))}}
    if layer == "normals":                   # nan_7x7's construction on 2 x 300: three workgroups of 256, the last partly empty
        H, W = 2, 300
        camera = _pinhole(*pc.draw_camera(rng, B), W, H)
        pos = nc.lifted(nc.draw_depth(rng, B, H, W), camera)
        upstream = np.round(rng.uniform(-1, 1, (B, H, W, 3)) * 64) / 64
        pos[POISONED_VIEW, 1, 150, 2] = np.nan
        upstream[POISONED_VIEW, 0, W - 1, 2] = np.nan
        return {"pos": pos, "camera": camera, "frame": "world", "shape": (B, H, W), "upstream": {"normal": pc.f32(upstream)},
                "nonzero": True}
    assert layer == "transform", name        # 257 points and normals: a second workgroup with one live lane
    n = 257
    pos = rng.uniform(-2.0, 2.0, (B, n, 4))
    pos[..., 3] = rng.uniform(0.5, 2.0, (B, n))
    normal = rng.uniform(-1.0, 1.0, (B, n, 3))
    pos[POISONED_VIEW, 100, 0] = np.nan
    normal[POISONED_VIEW, 256, 1] = np.nan
    return {"camera": fc.camera_vectors(rng, B, False), "pos": pc.f32(pos), "normal": pc.f32(normal),
            "upstream": {"pos": pc.f32(rng.uniform(-1, 1, (B, n, 4))), "normal": pc.f32(rng.uniform(-1, 1, (B, n, 3)))}}


@functools.lru_cache(maxsize=None)
def case(layer, name, variant=None):
    if layer == "lift":
        return _special_finite() if name == "special_finite_3x3" else su.case(name)
    if layer == "dense":
        return _dense_zdepth() if name == "zdepth_9x7" else de.case(name, *variant)
    if layer == "normals":
        return dict(ne.case(name), frame="world")
    if layer == "along_ray":
        scene, kwargs, _ = se.build(name)
        return {"scene": scene, "kwargs": kwargs, "upstream": se.upstream(scene, kwargs)}
    if layer == "ndc":
        return sne.case(name)
    if layer == "transform":
        return _transform_case(name)
    if layer == "project":
        assert name == "zdepth_16x12", name
        return _zdepth_case()
    assert layer == "poisoned", layer
    return _poisoned(name)


# ---- the restatements ------------------------------------------------------------------------------------------------
def _gradients(layer, c, variant=None):
    """(values, gradients, camera gradients) of a case dict of `layer` (not 'poisoned')."""
    if layer == "lift":
        v, g, cam = co.lift_gradients({"depth": c["depth"]}, c["camera"], c["upstream"], "world")
    elif layer == "dense":
        v, g, cam = dco.project_gradients(de.inputs(c), c["camera"], c["upstream"], c["blur_size"])
    elif layer == "normals":
        v, g, cam = dco.normals_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], "world")
    elif layer in ("along_ray", "ndc"):
        got = sco.batch_gradients(layer, c["scene"], c["upstream"]["image"], **c["kwargs"])
        return None, None, {k: got["camera." + k] for k in KEYS}
    elif layer == "transform":
        return fo.transform_gradients(variant, fc.transform_inputs(c), c["camera"], c["upstream"])
    else:
        assert layer == "project", layer
        key = "px_coord" if variant else "plane"
        return fo.project_gradients(variant, c["surfels"], c["camera"], {key: c["upstream"][key]})
    return v, g, cam["camera"]


def _layer_of(layer, name):
    return poisoned_layer(name) if layer == "poisoned" else layer


@functools.lru_cache(maxsize=None)
def expected(layer, name, variant=None):
    return _gradients(_layer_of(layer, name), case(layer, name, variant), variant)


@functools.lru_cache(maxsize=None)
def magnitudes(layer, name, variant=None):
    """(values, gradients, camera gradients): the restatements' sums of |terms| per entry of expected()
    (tests/entry_checks.py), for the layers that are held per entry -- lift, normals, transform, project and their
    poisoned batches.  The plane fit's values and pos gradient have no such sum (None: entry_checks.check_plane_fit)."""
    import entry_checks
    c, layer = case(layer, name, variant), _layer_of(layer, name)
    if layer == "lift":
        return so.magnitudes({"depth": c["depth"]}, c["camera"], c["upstream"], "world")
    if layer == "normals":
        return None, None, no.camera_magnitudes({"pos": c["pos"]}, c["camera"], c["upstream"], c["shape"],
                                                entry_checks.NORMALS_C64 / entry_checks.C)
    if layer == "transform":
        return fo.transform_magnitudes(variant, fc.transform_inputs(c), c["camera"], c["upstream"])
    assert layer == "project", layer
    key = "px_coord" if variant else "plane"
    return fo.project_magnitudes(variant, c["surfels"], c["camera"], {key: c["upstream"][key]})


def one_view(layer, c, b):
    """View b of a batched case dict of the lift, the dense layer, the normals or the transform, as a case of its own."""
    keys = {"lift": ("depth",), "dense": do.INPUTS, "normals": ("pos",), "transform": ("pos", "normal")}[layer]
    one = dict(c, **{k: (None if c[k] is None else c[k][b:b + 1]) for k in keys},
               upstream={k: u[b:b + 1] for k, u in c["upstream"].items()},
               camera=dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in KEYS}))
    if "shape" in c:
        one["shape"] = (1, *c["shape"][1:])
    return one


def _reversed(layer, c):
    """The case with its points in reversed order: the same function, the sums over the points run backwards."""
    if layer == "lift":
        return dict(c, depth=c["depth"][:, ::-1].copy(), upstream={"pos": c["upstream"]["pos"][:, ::-1].copy()})
    if layer == "dense":
        B, H, W, D = c["shape"]
        return dict(c, surfels=c["surfels"][:, ::-1].copy(), rgb=c["rgb"].reshape(B, H * W, D)[:, ::-1].reshape(c["rgb"].shape))
    if layer == "normals":
        return dict(c, pos=c["pos"][:, ::-1, ::-1].copy(), upstream={"normal": c["upstream"]["normal"][:, ::-1, ::-1].copy()})
    if layer == "transform":
        return dict(c, pos=c["pos"][:, ::-1].copy(), normal=c["normal"][:, ::-1].copy(),
                    upstream={k: u[:, ::-1].copy() for k, u in c["upstream"].items()})
    assert layer == "project", layer
    return dict(c, surfels=c["surfels"][:, ::-1].copy(), upstream={k: u[:, ::-1].copy() for k, u in c["upstream"].items()})


@functools.lru_cache(maxsize=None)
def second(layer, name, variant=None):
    """The camera gradients of expected() from another order of the same sums (module docstring)."""
    c = case(layer, name, variant)
    layer = _layer_of(layer, name)
    if layer in ("along_ray", "ndc"):
        g = c["upstream"]["image"]
        flat = np.arange(g.size).reshape(g.shape) < g.size // 2
        halves = [_gradients(layer, dict(c, upstream={"image": np.where(m, g, np.float32(0))}))[2] for m in (flat, ~flat)]
        return {k: halves[0][k] + halves[1][k] for k in KEYS}
    if layer == "lift":                      # the pixel grid runs backwards with the depths
        grid = so.pixel_grid
        with mock.patch.object(so, "pixel_grid", lambda *a, **k: tuple(np.ascontiguousarray(v[::-1]) for v in grid(*a, **k))):
            return _gradients(layer, _reversed(layer, c), variant)[2]
    return _gradients(layer, _reversed(layer, c), variant)[2]


def top(want):
    """The camera's largest finite gradient."""
    vals = [np.abs(w[np.isfinite(w)]).max() for w in want.values() if np.isfinite(w).any()]
    return max(vals) if vals else 0.0


@functools.lru_cache(maxsize=None)
def noise(layer, name, variant=None):
    """{entry: bool mask like the entry}: where the two orders differ by more than 1e-7 relative -- rounding noise of the
    restatement, which no relative comparison can hold; all False for a non-finite entry."""
    a, b = expected(layer, name, variant)[2], second(layer, name, variant)
    out = {}
    for k in KEYS:
        with np.errstate(invalid="ignore"):
            out[k] = np.isfinite(a[k]) & np.isfinite(b[k]) & (np.abs(a[k] - b[k]) > 1e-7 * np.maximum(np.abs(a[k]), np.abs(b[k])))
    return out
