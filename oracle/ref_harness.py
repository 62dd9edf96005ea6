"""What every golden generator shares: the reference import, the scene builder, the upstream gradients, the masked
loss, and packing / writing a fixture -- test infrastructure.

Runs only where the reference checkout is present (``SRH_REFERENCE``, default /root/reference); the GPU box never sees
it and no test imports this module.  The reference is imported UNMODIFIED, once, here, with its start-up prints
silenced; the generator modules (``oracle/golden_<fixture prefixes>.py``) reach it through this module's ``ref_*``
names.  Nothing of the reference's code is written anywhere: fixtures hold arrays and the ``meta`` / ``note`` /
``kwargs`` strings only.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SRH_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

from oracle.golden_io import diff_npz, pack_scene  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import diffrend.numpy.renderer as ref_np  # noqa: E402
    import diffrend.model as ref_model  # noqa: E402
    import diffrend.torch.render as ref_tch_render  # noqa: E402
    import diffrend.torch.renderer as ref_tch  # noqa: E402
    import diffrend.torch.utils as ref_utils  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")     # the entry point redirects this for --check
ONLY = []                                       # name prefixes: generate just those fixtures
WRITTEN = []                                    # names written in this run, in order


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def torch_scene(sc, dtype=torch.float32, camera_leaves=False, requires_grad=True):
    """The reference's torch scene dict for scene ``sc``; returns (scene, leaves).

    Every differentiable input -- lights.pos / attenuation / ambient, colors, materials.albedo / coeffs, every object
    field but material_idx, and with ``camera_leaves`` also camera.eye / at / up -- is a tensor of ``dtype`` that
    requires grad (or not: ``requires_grad=False`` is the forward-only scene), listed in ``leaves`` under its dotted
    name.  Values: float32 converts directly; float64 rounds through float32 first, so both precisions render the
    values the fixture stores.  A scene without attenuation / ambient / coeffs (the numpy backend's model, g9) gets the
    neutral (1, 0, 0) / 0 / (1, 0, 0) as plain tensors, not leaves.
    """
    def tensor(a):
        a = np.asarray(a, dtype=np.float32)
        return torch.tensor(a.astype(np.float64) if dtype == torch.float64 else a)

    def leaf(a):
        return tensor(a).requires_grad_(requires_grad)

    leaves = {}
    tsc = {"camera": dict(sc["camera"], proj_type=sc["camera"].get("proj_type", "perspective"))}
    for k in ("eye", "at", "up"):
        if camera_leaves:
            tsc["camera"][k] = leaves["camera." + k] = leaf(sc["camera"][k])
        else:
            tsc["camera"][k] = tensor(sc["camera"][k])
    n_lights, n_mat = len(sc["lights"]["pos"]), len(sc["materials"]["albedo"])
    neutral = {"lights.attenuation": [[1., 0., 0.]] * n_lights, "lights.ambient": [0., 0., 0.],
               "materials.coeffs": [[1., 0., 0.]] * n_mat}
    tsc["lights"] = {"color_idx": torch.tensor(np.asarray(sc["lights"]["color_idx"]))}
    tsc["materials"] = {}
    for name in ("lights.pos", "lights.attenuation", "lights.ambient", "colors", "materials.albedo", "materials.coeffs"):
        grp, _, k = name.rpartition(".")
        src, dst = (sc[grp], tsc[grp]) if grp else (sc, tsc)
        if k in src:
            dst[k] = leaves[name] = leaf(src[k])
        else:
            dst[k] = tensor(neutral[name])
    tsc["objects"] = {}
    for kind, grp in sc["objects"].items():
        tg = {"material_idx": torch.tensor(np.asarray(grp["material_idx"]))}
        for k, v in grp.items():
            if k != "material_idx":
                tg[k] = leaves[f"{kind}.{k}"] = leaf(v)
        tsc["objects"][kind] = tg
    if "tonemap" in sc:
        tsc["tonemap"] = {"type": "gamma", "gamma": torch.tensor([float(np.ravel(sc["tonemap"]["gamma"])[0])], dtype=dtype)}
    return tsc, leaves


@contextlib.contextmanager
def itruediv_shim():
    """``x /= y`` on tensors rebinds x to x / y instead of dividing in place.

    The reference's perspective generate_rays normalises its ray directions in place (``ray_dir /= ...``,
    torch/utils.py:476), and current torch refuses to differentiate that with respect to the camera ("modified by an
    inplace operation").  The reference's code runs WITHOUT EDITS while ``torch.Tensor.__itruediv__`` is replaced by
    ``lambda self, other: self / other`` for the duration of the call: Python then rebinds the name to the quotient
    instead of writing in place, i.e. the statement is read as d = v / |v|.  The orthographic branch has no in-place
    step and gives the same result with and without the shim.
    """
    saved = torch.Tensor.__itruediv__
    torch.Tensor.__itruediv__ = lambda self, other: self / other
    try:
        yield
    finally:
        torch.Tensor.__itruediv__ = saved


@contextlib.contextmanager
def precision(dtype):
    """The reference creates its own tensors as ``diffrend.torch.utils.FloatTensor``; pointing that name at
    ``torch.DoubleTensor`` for the duration of a call runs the same unedited code in float64 on float64 leaves."""
    saved = ref_utils.FloatTensor
    ref_utils.FloatTensor = torch.DoubleTensor if dtype == torch.float64 else torch.FloatTensor
    try:
        yield
    finally:
        ref_utils.FloatTensor = saved


def render(tsc, **kw):
    """The reference torch backend's render(), untiled and unshadowed unless ``kw`` says otherwise, prints silenced."""
    with quiet():
        return ref_tch.render(tsc, **{"tiled": False, "shadow": False, **kw})


def upstream(shape, aux=False, rng=None):
    """Upstream gradients in (-1, 1), fp32-representable, for outputs of ``shape`` = (H, W) or (views, H, W): image and
    depth from RandomState(7) -- or from ``rng`` where a family draws them from a stream of its own (g9: RandomState(99);
    v1: RandomState(23), after its per-view offsets) -- and with ``aux`` normal and pos from RandomState(11)."""
    rng = rng or np.random.RandomState(7)
    ups = {"image": f32(rng.uniform(-1, 1, size=shape + (3,))), "depth": f32(rng.uniform(-1, 1, size=shape))}
    if aux:
        rng = np.random.RandomState(11)
        ups["normal"] = f32(rng.uniform(-1, 1, size=shape + (3,)))
        ups["pos"] = f32(rng.uniform(-1, 1, size=shape + (3,)))
    return ups


def masked_loss(res, ups, hit):
    """sum image * g_i + sum_hit depth * g_d (+ sum_hit normal . g_n + sum_hit pos . g_p): every per-pixel term but the
    image's is masked by torch.where(hit, ., 0) -- the hip backend ignores the upstream gradients of misses (the
    reference differentiates object 0's intersection there)."""
    dtype = res["image"].dtype
    loss = torch.sum(res["image"] * torch.tensor(ups["image"], dtype=dtype))
    for k in ("depth", "normal", "pos"):
        if k in ups:
            x = res[k]
            m = hit if x.dim() == hit.dim() else hit[:, :, None].expand(*x.shape)
            loss = loss + torch.sum(torch.where(m, x * torch.tensor(ups[k], dtype=dtype), torch.zeros_like(x)))
    return loss


def pack_grads(out, leaves, prefix="grad/"):
    """``grad/<leaf>`` for every leaf: what autograd left in .grad, zeros where it returned None."""
    for k, v in leaves.items():
        out[prefix + k] = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), dtype=np.float32)
        print(f"{k:22s} |grad| max {np.abs(out[prefix + k]).max():.4g}")


def pack_run(sc, ups, res, leaves, kw=None):
    """A gradient fixture's common keys: the scene, grad_in/<output>, ref/<output> and ref/nearest, kwargs, grad/<leaf>."""
    out = pack_scene(sc)
    for k, g in ups.items():
        out["grad_in/" + k] = g
        out["ref/" + k] = res[k].detach().numpy()
    out["ref/nearest"] = res["nearest"].detach().numpy().astype(np.int64)
    if kw is not None:
        out["kwargs"] = np.asarray(json.dumps(kw))
    pack_grads(out, leaves)
    return out


def layer_camera(camera, dtype=torch.float32):
    """A seeded case's camera (tests/*projection_cases.py) for the reference's projection layers: eye / at / up as tensors
    of the case's float32 values in ``dtype``."""
    return {k: (torch.tensor(np.asarray(v, dtype=np.float32), dtype=dtype) if k in ("eye", "at", "up") else v)
            for k, v in camera.items()}


def camera_views(camera, views):
    return {k: (v[views] if k in ("eye", "at", "up") else v) for k, v in camera.items()}


def run_views(run, n_views):
    """{output: tensor} of ``run(views)`` (``views`` a slice of the batch) over the whole batch."""
    if n_views != 3:
        return run(slice(None))
    # lookat_rot_inv calls torch.cross(up, z) without `dim`, which for [3, 3] operands -- three views, and only three --
    # still means dim 0: the cross product is taken ACROSS the views.  That is an accident of B == 3, not a meaning of
    # the layer, so such a case is recorded view by view
    per_view = [run(slice(b, b + 1)) for b in range(n_views)]
    return {k: torch.cat([r[k] for r in per_view]) for k in per_view[0]}


def pack_layer(c, leaves, res, cameras=("camera",), dtype=torch.float32):
    """A projection layer's fixture from case ``c``, its leaf tensors and the reference's outputs: backward of
    sum_outputs sum(output * upstream), then in/<input>, in/<camera>/<entry>, grad_in/<output>, ref/<output> and
    grad/<input> (zeros where autograd left None).  The caller adds its layer's own in/ keys."""
    assert set(res) == set(c["upstream"]), (sorted(res), sorted(c["upstream"]))
    sum(torch.sum(res[k] * torch.tensor(g, dtype=dtype)) for k, g in c["upstream"].items()).backward()
    flat = {"in/" + k: c[k] for k in leaves}
    for cam in cameras:
        for k, v in c[cam].items():
            flat[f"in/{cam}/{k}"] = np.asarray(v, dtype=np.float64 if k in ("fovy", "focal_length") else None)
    for k, g in c["upstream"].items():
        assert res[k].dtype == dtype and tuple(res[k].shape) == g.shape, k
        flat["grad_in/" + k] = g
        flat["ref/" + k] = res[k].detach().numpy()
    for k, t in leaves.items():
        flat["grad/" + k] = t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape), np.float32)
    return flat


def fixture_dir(subfolder, argv=None):
    """Where a layer's generator writes: tests/golden/<subfolder>, or the directory given with --out (a fresh run to
    compare with the committed fixtures)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the fixtures here instead of tests/golden/" + subfolder)
    return ap.parse_args(argv).out or os.path.join(REPO, "tests", "golden", subfolder)


def wanted(name):
    return not ONLY or any(name.startswith(p) for p in ONLY)


def write(name, flat):
    """Store fixture ``name``.  A file that already holds exactly this data is left alone (a zip's bytes carry the time
    of writing), so regenerating an unchanged fixture does not touch the working tree."""
    buf = io.BytesIO()
    np.savez_compressed(buf, **flat)
    path = os.path.join(OUT, name + ".npz")
    WRITTEN.append(name)
    if os.path.exists(path) and not diff_npz(np.load(path, allow_pickle=False), np.load(io.BytesIO(buf.getvalue()), allow_pickle=False)):
        print(f"{name}: unchanged")
        return
    os.makedirs(OUT, exist_ok=True)
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print(f"{name}: written, {len(buf.getvalue())} bytes")
