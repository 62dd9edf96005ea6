"""What the binned finish rounds take from their TILE instead of computing per pixel (srh_binned.h: RayTable, the ray
numerator's addends per column and row; srh_device.h: ToneHint), and the round's output stores: `binned` against
`exact`, bit for bit.

Every scene but those of test_no_hit_and_one_hit_tiles has a camera-facing wall behind its other primitives, so every
pixel is hit and goes through a finish round; depth must then be finite everywhere.  Shapes are the smallest that reach
each path: frames of one tile, of edge tiles in both directions and of one sample per axis (the linspace end-point
rule), slabs whose first row is no multiple of 16, row pitches of 2^26 elements and more."""
import numpy as np
import pytest
import torch

from surf_renderer_amd import pipeline, renderer, synthetic

DEV = "cuda:0"


def wall(scene, z=-3.0, radius=60.0):
    """`scene` with one more disc: a wall facing the camera (eye on +z), behind everything else"""
    d = scene["objects"].setdefault("disk", {"pos": np.zeros((0, 4)), "normal": np.zeros((0, 4)), "radius": np.zeros(0),
                                             "material_idx": np.zeros(0, dtype=np.int64)})
    d["pos"] = np.concatenate([np.asarray(d["pos"], dtype=np.float64), [[0.0, 0.0, z, 1.0]]])
    d["normal"] = np.concatenate([np.asarray(d["normal"], dtype=np.float64), [[0.0, 0.0, 1.0, 0.0]]])
    d["radius"] = np.concatenate([np.asarray(d["radius"], dtype=np.float64), [radius]])
    d["material_idx"] = np.concatenate([np.asarray(d["material_idx"], dtype=np.int64), [0]])
    return scene


def cloud(width, height, n=300, radius=0.3, seed=11):
    return wall(synthetic.disk_cloud_scene(n, width, height, radius=radius, seed=seed))


def one_type(kind, width, height, n=40, seed=5):
    """a one-batch scene of `kind`: n primitives in front of the camera and what plays the wall for that type"""
    rng = np.random.RandomState(seed)
    sc = synthetic.disk_cloud_scene(1, width, height)
    pos = np.concatenate([rng.uniform(-1.0, 1.0, size=(n, 3)), np.ones((n, 1))], axis=1)
    mat = np.zeros(n + 1, dtype=np.int64)
    if kind == "disk":
        return cloud(width, height, n=n, seed=seed)
    if kind == "sphere":
        objects = {"sphere": {"pos": np.concatenate([pos, [[0.0, 0.0, -200.0, 1.0]]]).astype(np.float32).astype(np.float64),
                              "radius": np.concatenate([np.full(n, 0.2), [190.0]]).astype(np.float32).astype(np.float64),
                              "material_idx": mat}}
    elif kind == "plane":
        nrm = np.concatenate([rng.normal(size=(3, 3)) * 0.2 + [0.0, 0.0, 1.0], np.zeros((3, 1))], axis=1)
        objects = {"plane": {"pos": np.array([[0.0, 0.0, -3.0, 1.0], [0.0, 0.0, -1.0, 1.0], [0.5, 0.0, 0.0, 1.0], [0.0, 0.5, 0.5, 1.0]]),
                             "normal": np.concatenate([[[0.0, 0.0, 1.0, 0.0]], nrm]).astype(np.float32).astype(np.float64),
                             "material_idx": np.zeros(4, dtype=np.int64)}}
    else:
        off = rng.uniform(-0.4, 0.4, size=(n, 3, 3))
        face = pos[:, None, :3] + off
        big = np.array([[[-90.0, -90.0, -3.0], [90.0, -90.0, -3.0], [0.0, 120.0, -3.0]]])
        face = np.concatenate([face, big])
        face = np.concatenate([face, np.ones((n + 1, 3, 1))], axis=2)
        e1, e2 = face[:, 1, :3] - face[:, 0, :3], face[:, 2, :3] - face[:, 0, :3]
        nrm = np.cross(e1, e2)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm[nrm[:, 2] < 0] *= -1.0
        objects = {"triangle": {"face": face.astype(np.float32).astype(np.float64),
                                "normal": np.concatenate([nrm, np.zeros((n + 1, 1))], axis=1).astype(np.float32).astype(np.float64),
                                "material_idx": mat}}
    sc["objects"] = objects
    return sc


def mixed(width, height):
    return synthetic.demo_scene(width, height, with_planes=True)      # its back wall plane covers every pixel


def frames(scene, shading="numpy", rows=None, wpt=0, aux=False):
    """(binned outputs, exact outputs) as lists of numpy arrays: image, depth, nearest [, normal, pos]"""
    buf = renderer.flatten_scene(scene, device=DEV)
    cam = renderer.camera_struct(scene["camera"], shading)
    width, height = renderer.frame_size(cam)
    h = height if rows is None else rows[1] - rows[0]
    outs = []
    for mode in ("binned", "exact"):
        extra = None
        if aux:      # NaN-filled: every element has to be written
            extra = tuple(torch.full((h, width, 3), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
        got = renderer.render_buffers(buf, cam, rows=rows, mode=mode, shading=shading, aux=extra,
                                      waves_per_tile=wpt if mode == "binned" else 0,
                                      workspace=buf.new_workspace(width, height))
        outs.append([t.cpu().numpy() for t in list(got) + list(extra or ())])
    return outs


def check(got, want, all_hit=True):
    names = ("image", "depth", "nearest", "normal", "pos")
    for name, g, w in zip(names, got, want):
        np.testing.assert_array_equal(g, w, err_msg=name)
    if all_hit:
        assert np.isfinite(got[1]).all()
        assert np.isfinite(got[0]).all()


EDGE_FRAMES = [(16, 16), (17, 16), (37, 29), (1, 1), (7, 1), (1, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("shading", ["numpy", "torch"])
@pytest.mark.parametrize("wpt", [1, 4])
@pytest.mark.parametrize("size", EDGE_FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_tiles_and_end_points(size, wpt, shading):
    got, want = frames(cloud(*size), shading=shading, wpt=wpt)
    check(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("wpt", [1, 4])
@pytest.mark.parametrize("rows", [(5, 41), (16, 17)])
def test_slab_rows_into_the_benchmarks_layout(rows, wpt):
    """H = 50, a slab whose first row is not a multiple of 16 (and one of a single row), written into the strided views of
    a (rows, 4W) slab; compared with the same rows of a full-frame exact render."""
    width, height = 37, 50
    scene = cloud(width, height)
    buf = renderer.flatten_scene(scene, device=DEV)
    cam = renderer.camera_struct(scene["camera"])
    full = renderer.render_buffers(buf, cam, mode="exact")
    h = rows[1] - rows[0]
    slab = torch.full((h, 4 * width), float("nan"), dtype=torch.float32, device=DEV)
    image, depth = pipeline.slab_views(slab, width)
    nearest = torch.full((h, width), -7, dtype=torch.int32, device=DEV)
    renderer.render_buffers(buf, cam, rows=rows, mode="binned", out=(image, depth, nearest), waves_per_tile=wpt,
                            workspace=buf.new_workspace(width, height))
    got = [image.cpu().numpy(), depth.cpu().numpy(), nearest.cpu().numpy()]
    check(got, [t[rows[0]:rows[1]].cpu().numpy() for t in full])


@pytest.mark.gpu
@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
@pytest.mark.parametrize("wpt", [1, 4])
@pytest.mark.parametrize("kind", ["disk", "plane", "sphere", "triangle", "mixed"])
def test_every_instantiation(kind, wpt, aux):
    """One-batch scenes of each type and the four-type scene, Lambert and (with the normal / pos outputs, which only the
    torch shading has) Phong: together every k_render_binned_mem instantiation."""
    scene = mixed(37, 29) if kind == "mixed" else one_type(kind, 37, 29)
    got, want = frames(scene, shading="torch" if aux else "numpy", wpt=wpt, aux=aux)
    check(got, want)
    if not aux:
        got, want = frames(scene, shading="torch", wpt=wpt)
        check(got, want)


# 2 rows x 20 columns in a 512 MB buffer: row pitches whose byte offsets need more than 28 and more than 29 bits, and
# (15 rows of a tile at 2^27 - 64 elements) would not fit 32.  The stores form their addresses in 64 bits.
BIG = 1 << 27
PITCHES = [1 << 26, BIG - 64]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["image", "depth"])
@pytest.mark.parametrize("pitch", PITCHES, ids=["2^26", "2^27-64"])
def test_wide_row_pitch(pitch, which):
    width, height = 20, 2
    scene = cloud(width, height, n=60)
    buf = renderer.flatten_scene(scene, device=DEV)
    cam = renderer.camera_struct(scene["camera"])
    want = [t.cpu().numpy() for t in renderer.render_buffers(buf, cam, mode="exact")]
    big = torch.zeros(BIG, dtype=torch.float32, device=DEV)
    if which == "image":
        image = big.as_strided((height, width, 3), (pitch, 3, 1), 0)
        depth = torch.full((height, width), float("nan"), dtype=torch.float32, device=DEV)
    else:
        image = torch.full((height, width, 3), float("nan"), dtype=torch.float32, device=DEV)
        depth = big.as_strided((height, width), (pitch, 1), 0)
    nearest = torch.full((height, width), -7, dtype=torch.int32, device=DEV)
    for wpt in (1, 4):
        big.zero_()
        renderer.render_buffers(buf, cam, mode="binned", out=(image, depth, nearest), waves_per_tile=wpt,
                                workspace=buf.new_workspace(width, height))
        check([image.cpu().numpy(), depth.cpu().numpy(), nearest.cpu().numpy()], want)
        # nothing landed outside the two rows
        n_row = width * (3 if which == "image" else 1)
        assert int(torch.count_nonzero(big[n_row:pitch])) == 0 and int(torch.count_nonzero(big[pitch + n_row:])) == 0
    del big


@pytest.mark.gpu
def test_render_views_with_row_strides():
    width, height = 37, 29
    scene = cloud(width, height)
    buf = renderer.flatten_scene(scene, device=DEV)
    cams = []
    for k in range(3):
        cam = dict(scene["camera"])
        cam["eye"] = [0.3 * k, -0.2 * k, 4.0 - 0.3 * k, 1.0]
        cam["fovy"] = float(np.deg2rad(45.0 + 5.0 * k))
        cams.append(renderer.camera_struct(cam))
    send = torch.full((3, height, 4 * width), float("nan"), dtype=torch.float32, device=DEV)
    img = send.as_strided((3, height, width, 3), (height * 4 * width, 4 * width, 3, 1), 0)
    dep = send.as_strided((3, height, width), (height * 4 * width, 4 * width, 1), 3 * width)
    near = torch.full((3, height, width), -7, dtype=torch.int32, device=DEV)
    renderer.render_views_buffers(buf, cams, img, dep, near, image_row_stride=4 * width, depth_row_stride=4 * width,
                                  mode="binned")
    for k, cam in enumerate(cams):
        want = renderer.render_buffers(buf, cam, mode="exact")
        check([img[k].cpu().numpy(), dep[k].cpu().numpy(), near[k].cpu().numpy()], [t.cpu().numpy() for t in want])


@pytest.mark.gpu
@pytest.mark.parametrize("wpt", [1, 4])
def test_no_hit_and_one_hit_tiles(wpt):
    """Nothing hit anywhere (no tile builds a table), and a 48 x 48 frame where one tiny disc shows in a single pixel of
    one tile.  No wall here: depth is not finite."""
    empty = synthetic.disk_cloud_scene(5, 37, 29, radius=0.01)
    empty["objects"]["disk"]["pos"][:, 0] += 50.0
    got, want = frames(empty, wpt=wpt)
    check(got, want, all_hit=False)
    assert not np.isfinite(got[1]).any()

    one = synthetic.disk_cloud_scene(1, 48, 48, radius=0.01)
    # the disc sits on the ray of pixel (column 21, row 26), facing the camera
    ray = renderer.generate_rays(one["camera"], device=DEV).cpu().numpy().reshape(4, 48, 48)[:3, 26, 21].astype(np.float64)
    eye = np.array(one["camera"]["eye"][:3])
    centre = (eye + 4.0 * ray / np.linalg.norm(ray)).astype(np.float32).astype(np.float64)
    one["objects"]["disk"]["pos"] = np.array([[centre[0], centre[1], centre[2], 1.0]])
    one["objects"]["disk"]["normal"] = np.array([[0.0, 0.0, 1.0, 0.0]])
    one["objects"]["disk"]["radius"] = np.array([np.float32(0.005)], dtype=np.float64)
    got, want = frames(one, wpt=wpt)
    check(got, want, all_hit=False)
    assert int(np.isfinite(got[1]).sum()) == 1 and np.isfinite(got[1][26, 21])


@pytest.mark.gpu
@pytest.mark.parametrize("shading", ["numpy", "torch"])
@pytest.mark.parametrize("tone", [0.8, 0.0, -1.0, None], ids=["g0.8", "g0", "g-1", "off"])
def test_tonemap(tone, shading):
    scene = cloud(37, 29)
    if tone is None:
        scene.pop("tonemap")
    else:
        scene["tonemap"] = {"type": "gamma", "gamma": tone}
    for wpt in (1, 4):
        got, want = frames(scene, shading=shading, wpt=wpt)
        for name, g, w in zip(("image", "depth", "nearest"), got, want):
            np.testing.assert_array_equal(g, w, err_msg=name)
        assert np.isfinite(got[1]).all()
