"""The hip backend's mirror of the reference backend interface: ``render(scene, **params) -> dict``.

Same call and same scene dict as ``diffrend.numpy.renderer.render`` (numpy/renderer.py:204-272) and
``diffrend.torch.renderer.render`` (torch/renderer.py:136-355); the work is done by hand-written
gfx950 kernels behind the C ABI of include/srh.h.  PyTorch is used for device memory and streams only.

Layers
  flatten_scene()   expanded scene dict (lists / ndarrays / tensors) -> SceneBuffers: contiguous fp32 /
                    int32 device arrays in the reference's layouts and concatenation order, plus the
                    ctypes descriptors libsrh consumes.  Done once per scene; stays resident in HBM.
  render_buffers()  one frame from resident buffers and a camera (what bench.py times).
  render()          the drop-in: flatten + render_buffers + reference-shaped result dict.

There is no CPU fallback: without a GPU or without libsrh.so these functions raise.
"""
from __future__ import annotations

import ctypes as C
import threading
from dataclasses import dataclass, field
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .scene import PRIM_CODE, _OBJ_FIELDS, unit_up

# keyword arguments of the torch backend's render() that callers pass routinely (torch/renderer.py:152-168, 233-245,
# 291, 326-327); the hip backend accepts them so call sites need no edits.  What each does here:
#   tiled, tile_size        memory knobs of the reference's (pixels x primitives) arrays: no effect on any output
#   backface_culling        the reference only LABELS primitives (torch/utils.py:515-536) and never reads the labels:
#                           every output is unchanged (oracle/check_ref_kwargs.py ran the reference both ways)
#   vis_stat                True raises in the reference ('Removed Support for vis_stat', :235) and here
#   norm_depth_image_only   `image` becomes the normalised depth of :245-249 (see render())
#   shadow                  shadow rays (:291-314)
_TORCH_ONLY_KWARGS = {"tiled", "tile_size", "backface_culling", "norm_depth_image_only", "vis_stat", "shadow"}


def _require_gpu(device: torch.device) -> None:
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("the hip backend needs an AMD GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback -- use the reference's numpy backend instead")


def _as_tensor(x, dtype: torch.dtype, device: torch.device, keep_graph: bool = False) -> torch.Tensor:
    """Contiguous tensor of ``x`` in ``dtype``: on ``device`` if ``x`` already lives there or takes part in autograd
    (with ``keep_graph`` a tensor that requires grad stays attached to the graph -- casts and copies are
    differentiable -- so gradients reach the caller's leaf); otherwise still in host memory, for ``_upload`` to send
    with everything else in one transfer."""
    if isinstance(x, torch.Tensor):
        t = x if (keep_graph and x.requires_grad) else x.detach()
        if t.is_cuda or t.requires_grad:
            return t.to(device=device, dtype=dtype).contiguous()
        x = t.numpy()
    # host leaves are converted and packed with numpy (plain single-threaded copies): torch's CPU operators go through
    # its OpenMP pool, which on a box with fewer cores than threads costs milliseconds per frame while the GPU runs
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=_NP_DTYPE[dtype]))


_NP_DTYPE = {torch.float32: np.float32, torch.int32: np.int32}
_STAGING: Dict[torch.device, Tuple[torch.Tensor, torch.cuda.Event]] = {}
_STAGING_LOCK = threading.Lock()
_UPLOAD_ALIGN = 256


def _upload(tensors: Dict[str, torch.Tensor], device: torch.device) -> None:
    """Move every host tensor of ``tensors`` to the device in ONE host-to-device copy: the leaves are packed into a
    pinned staging buffer (kept per device, guarded by an event so that a new frame's packing waits for the previous
    frame's copy) and the device side is carved into typed views.  A scene is ~10 small arrays; sent one by one from
    pageable memory each costs a synchronous copy of ~0.6 ms, which was all of render(scene)'s time."""
    host = [(k, t) for k, t in tensors.items() if not t.is_cuda]
    if not host:
        return
    offsets, total = [], 0
    for _, t in host:
        offsets.append(total)
        total += -(-t.numel() * t.element_size() // _UPLOAD_ALIGN) * _UPLOAD_ALIGN
    total = max(total, _UPLOAD_ALIGN)
    with _STAGING_LOCK:
        _upload_locked(tensors, device, host, offsets, total)


def _upload_locked(tensors, device, host, offsets, total) -> None:
    entry = _STAGING.get(device)
    if entry is not None:
        entry[1].synchronize()
    if entry is None or entry[0].numel() < total:
        entry = (torch.empty(max(total, 1 << 20), dtype=torch.uint8).pin_memory(), torch.cuda.Event())
        _STAGING[device] = entry
    staging, done = entry
    staging_np = staging.numpy()
    for (_, t), off in zip(host, offsets):
        n = t.numel() * t.element_size()
        if n:
            staging_np[off:off + n] = t.numpy().reshape(-1).view(np.uint8)
    packed = torch.empty(total, dtype=torch.uint8, device=device)
    packed.copy_(staging[:total], non_blocking=True)
    done.record(torch.cuda.current_stream(device))
    for (k, t), off in zip(host, offsets):
        n = t.numel() * t.element_size()
        tensors[k] = packed[off:off + n].view(t.dtype).reshape(t.shape)


def _host_view(x) -> Optional[np.ndarray]:
    """numpy view for host-side validation; None for device tensors (not worth a sync)."""
    if isinstance(x, torch.Tensor):
        return None if x.is_cuda else x.detach().numpy()
    return np.asarray(x)


@dataclass
class SceneBuffers:
    """A scene resident in HBM in the layouts of include/srh.h."""
    device: torch.device
    kinds: List[str]
    counts: List[int]
    tensors: Dict[str, torch.Tensor]          # "<kind>.<field>", "lights.pos", ... (keeps memory alive)
    objects: _lib.SrhObjects
    lights: _lib.SrhLights
    materials: _lib.SrhMaterials
    gamma: Optional[float]
    workspace: Optional[torch.Tensor] = None   # per-frame scratch, sized for the largest frame seen so far
    workspace_frame: Tuple[int, int] = (0, 0)
    total: int = 0
    shadow_workspace: Optional[torch.Tensor] = None   # scratch of the accelerated shadow pass (light views)
    camera_scratch: Optional[torch.Tensor] = None     # workgroup partial sums of the camera gradients (srh_render_bwd_camera)
    camera_scratch_views: Optional[torch.Tensor] = None   # the same for a batch of views (srh_render_views_bwd_camera)

    def ensure_workspace(self, width: int, height: int) -> torch.Tensor:
        """Device scratch for libsrh (primitive records + tile bins) at ``width x height``."""
        if self.workspace is None or width > self.workspace_frame[0] or height > self.workspace_frame[1]:
            lib = _lib.load()
            w, h = max(width, self.workspace_frame[0]), max(height, self.workspace_frame[1])
            need = lib.srh_workspace_bytes(C.byref(self.objects), w, h)
            if need == 0:
                raise _lib.SrhError(-1, lib.srh_last_error().decode())
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.workspace_frame = (w, h)
        return self.workspace

    def ensure_shadow_workspace(self, width: int, height: int) -> torch.Tensor:
        """Scratch of the accelerated shadow pass: room for the light views (tile bins in every light's screen space)
        behind the primary frame's scratch."""
        lib = _lib.load()
        need = lib.srh_shadow_workspace_bytes(C.byref(self.objects), width, height, self.lights.n_lights)
        if need == 0:
            raise _lib.SrhError(-2, lib.srh_last_error().decode())
        if self.shadow_workspace is None or self.shadow_workspace.numel() < need:
            self.shadow_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.shadow_workspace

    def ensure_camera_scratch(self, width: int, rows: int) -> torch.Tensor:
        """Scratch of srh_render_bwd_camera for a backward over ``width x rows`` pixels.  Its contents never matter: every
        workgroup of a backward launch overwrites its own slot."""
        lib = _lib.load()
        need = lib.srh_camera_grad_scratch_bytes(width, rows)
        if need == 0:
            raise _lib.SrhError(-2, lib.srh_last_error().decode())
        if self.camera_scratch is None or self.camera_scratch.numel() * 8 < need:
            self.camera_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        return self.camera_scratch

    def ensure_camera_scratch_views(self, width: int, rows: int, n_views: int) -> torch.Tensor:
        """Scratch of srh_render_views_bwd_camera for a backward over ``n_views`` views of ``width x rows`` pixels: the
        views' finish descriptors and a slice of partial sums per view.  Its contents never matter either."""
        lib = _lib.load()
        need = lib.srh_camera_grad_scratch_bytes_views(width, rows, n_views)
        if need == 0:
            raise _lib.SrhError(-2, lib.srh_last_error().decode())
        if self.camera_scratch_views is None or self.camera_scratch_views.numel() * 8 < need:
            self.camera_scratch_views = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        return self.camera_scratch_views

    def new_workspace(self, width: int, height: int) -> torch.Tensor:
        """An additional scratch buffer (one per frame in flight when frames are pipelined over several streams)."""
        lib = _lib.load()
        need = lib.srh_workspace_bytes(C.byref(self.objects), width, height)
        if need == 0:
            raise _lib.SrhError(-1, lib.srh_last_error().decode())
        return torch.empty(need, dtype=torch.uint8, device=self.device)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors.values())


class _Leaf(NamedTuple):
    """A scene leaf outside scene['objects'].  Its field in the descriptor is named like the last step of its path."""
    path: Tuple[str, ...]               # where it sits in the scene dict
    struct: str                         # the descriptor that points at it: "lights" (SrhLights), "materials" (SrhMaterials)
    grad: Optional[str]                 # its SrhGrads field; None: an index array, not differentiable
    shape: Tuple[int, ...]              # its shape in SceneBuffers.tensors
    torch_only: bool = False            # an optional input of the torch backend's shading model (the numpy one ignores
                                        # it, numpy/renderer.py:234-255)


# the scene's leaves outside scene['objects'] under their SceneBuffers.tensors keys, in the order of _float_keys
_SCENE_LEAVES = {
    "lights.pos": _Leaf(("lights", "pos"), "lights", "lights_pos", (-1, 4)),
    "lights.color_idx": _Leaf(("lights", "color_idx"), "lights", None, (-1,)),
    "colors": _Leaf(("colors",), "lights", "colors", (-1, 3)),
    "materials.albedo": _Leaf(("materials", "albedo"), "materials", "albedo", (-1, 3)),
    "materials.coeffs": _Leaf(("materials", "coeffs"), "materials", "coeffs", (-1, 3), True),
    "lights.attenuation": _Leaf(("lights", "attenuation"), "lights", "attenuation", (-1, 3), True),
    "lights.ambient": _Leaf(("lights", "ambient"), "lights", "ambient", (3,), True),
}


def _check_w(name: str, arr: Optional[np.ndarray], want: float) -> None:
    if arr is None or arr.size == 0:
        return
    w = arr[..., 3]
    if not np.all(w == want):
        raise ValueError(f"{name}: homogeneous w must be {want:g} for every row (the reference's convention, "
                         f"docs/scene_description.md:3-5); found {np.unique(w)[:4]}")


def flatten_scene(scene: Dict[str, Any], device="cuda", validate: bool = True, keep_graph: bool = False) -> SceneBuffers:
    """Upload an expanded scene.  Object batches keep scene['objects'] dict order, which defines the
    global primitive numbering (numpy/renderer.py:172-201).  The caller's scene is not modified.
    ``keep_graph`` keeps tensors that require grad attached to autograd (see ``render``)."""
    device = torch.device(device)
    _require_gpu(device)
    if device.type == "cuda" and device.index is None:
        # "cuda" means the current device; tensors report "cuda:N", and the out-buffer checks compare devices
        device = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    objs = scene["objects"]
    if not objs:
        raise ValueError("scene['objects'] is empty")
    if len(objs) > _lib.MAX_SEGMENTS:
        raise ValueError(f"at most {_lib.MAX_SEGMENTS} object batches")
    f32, i32 = torch.float32, torch.int32
    tensors: Dict[str, torch.Tensor] = {}
    kinds: List[str] = []
    counts: List[int] = []
    ob = _lib.SrhObjects()
    n_mat = int(np.asarray(_shape_of(scene["materials"]["albedo"]))[0])
    for s, (kind, grp) in enumerate(objs.items()):
        if kind not in PRIM_CODE:
            raise ValueError(f"unknown object type {kind!r}; expanded scenes hold disk / plane / sphere / "
                             f"triangle (use surf_renderer_amd.scene.load_scene for JSON 'obj' lists)")
        seg = ob.seg[s]
        seg.type = PRIM_CODE[kind]
        count = None
        for name in _OBJ_FIELDS[kind]:
            t = _as_tensor(grp[name], f32, device, keep_graph)
            if name == "radius":
                t = t.reshape(-1)
            elif name == "face":
                t = t.reshape(-1, 3, 4)
            else:
                t = t.reshape(-1, 4)
            if count is None:
                count = t.shape[0]
            elif t.shape[0] != count:
                raise ValueError(f"{kind}.{name}: {t.shape[0]} rows, expected {count}")
            if validate:
                host = _host_view(grp[name])
                if name in ("pos", "face"):
                    _check_w(f"{kind}.{name}", None if host is None else host.reshape(-1, 4), 1.0)
                elif name == "normal":
                    _check_w(f"{kind}.{name}", None if host is None else host.reshape(-1, 4), 0.0)
            tensors[f"{kind}.{name}"] = t
        mi_host = _host_view(grp["material_idx"])
        if validate and mi_host is not None and mi_host.size:
            if mi_host.min() < 0 or mi_host.max() >= n_mat:
                raise IndexError(f"{kind}.material_idx out of range for {n_mat} materials")
        mi = _as_tensor(grp["material_idx"], i32, device).reshape(-1)
        if mi.shape[0] != count:
            raise ValueError(f"{kind}.material_idx: {mi.shape[0]} entries, expected {count}")
        if count == 0:
            raise ValueError(f"{kind}: empty batch")
        tensors[f"{kind}.material_idx"] = mi
        seg.count = count
        kinds.append(kind)
        counts.append(count)
    ob.n_segments = len(kinds)

    src = _scene_leaves(scene)
    for key, x in src.items():
        leaf = _SCENE_LEAVES[key]
        tensors[key] = _as_tensor(x, i32 if leaf.grad is None else f32, device, keep_graph).reshape(leaf.shape)
    lpos, colors, albedo = tensors["lights.pos"], tensors["colors"], tensors["materials.albedo"]
    if lpos.shape[0] != tensors["lights.color_idx"].shape[0]:
        raise ValueError("lights.pos and lights.color_idx disagree on the number of lights")
    if lpos.shape[0] > _lib.MAX_LIGHTS:
        raise ValueError(f"at most {_lib.MAX_LIGHTS} lights")
    if validate:
        _check_w("lights.pos", _host_view(src["lights.pos"]), 1.0)
        ci = _host_view(src["lights.color_idx"])
        if ci is not None and ci.size and (ci.min() < 0 or ci.max() >= colors.shape[0]):
            raise IndexError("lights.color_idx out of range for the colour table")
    if "lights.attenuation" in tensors and tensors["lights.attenuation"].shape[0] != lpos.shape[0]:
        raise ValueError("lights.attenuation must have one (kc, kl, kq) row per light")
    if "materials.coeffs" in tensors and tensors["materials.coeffs"].shape[0] != albedo.shape[0]:
        raise ValueError("materials.coeffs must have one row per material")

    _upload(tensors, device)
    for s, kind in enumerate(kinds):
        for name in _OBJ_FIELDS[kind] + ("material_idx",):
            setattr(ob.seg[s], name, tensors[f"{kind}.{name}"].data_ptr())
    ls = _lib.SrhLights(n_lights=lpos.shape[0], n_colors=colors.shape[0])
    ms = _lib.SrhMaterials(n_materials=albedo.shape[0])
    for key in src:
        leaf = _SCENE_LEAVES[key]
        setattr(ls if leaf.struct == "lights" else ms, leaf.path[-1], tensors[key].data_ptr())

    gamma = None
    if "tonemap" in scene:
        tm = scene["tonemap"]
        if tm.get("type", "gamma") != "gamma":
            raise ValueError(f"tonemap type {tm.get('type')!r}: only 'gamma' exists (numpy/renderer.py:140-142)")
        g = tm["gamma"]
        gamma = float(g.detach().cpu().reshape(-1)[0]) if isinstance(g, torch.Tensor) else float(np.ravel(g)[0])

    return SceneBuffers(device=device, kinds=kinds, counts=counts, tensors=tensors, objects=ob, lights=ls,
                        materials=ms, gamma=gamma, total=sum(counts))


def _shape_of(x):
    if isinstance(x, torch.Tensor):
        return tuple(x.shape)
    return np.asarray(x).shape


def _scene_leaves(scene: Dict[str, Any]) -> Dict[str, Any]:
    """The caller's own leaf objects outside scene['objects'] (``_SCENE_LEAVES``) that the scene has, by flat key."""
    out: Dict[str, Any] = {}
    for key, leaf in _SCENE_LEAVES.items():
        grp = scene if len(leaf.path) == 1 else scene[leaf.path[0]]
        if not leaf.torch_only or leaf.path[-1] in grp:
            out[key] = grp[leaf.path[-1]]
    return out


def camera_struct(camera: Dict[str, Any], shading: str = "numpy") -> _lib.SrhCamera:
    """scene['camera'] -> SrhCamera.  List-typed ``at`` / ``up`` take the reference's float32 detour
    (numpy/ops.py:95-100, quirk Q11), which for the numpy backend's semantics includes normalising ``up`` in
    float32; arrays and tensors are taken at full precision."""
    def vec(val, f32_if_list: bool):
        if isinstance(val, torch.Tensor):
            return val.detach().cpu().double().numpy().reshape(-1)
        if f32_if_list and isinstance(val, (list, tuple)):
            return np.asarray(val, dtype=np.float32).astype(np.float64).reshape(-1)
        return np.asarray(val, dtype=np.float64).reshape(-1)

    def scalar(val) -> float:
        if isinstance(val, torch.Tensor):
            return float(val.detach().cpu().reshape(-1)[0])
        return float(np.ravel(val)[0])

    cam = _lib.SrhCamera()
    eye, at, up = vec(camera["eye"], False), vec(camera["at"], True), vec(camera["up"], True)
    if shading == "torch":
        # the torch backend holds all three as float32 tensors (make_torch_var, torch/render.py:81-100)
        eye, at, up = (v.astype(np.float32).astype(np.float64) for v in (eye, at, up))
    if up.size == 3:
        up = np.append(up, 0.0)
    if eye.size != 4 or at.size != 4 or up.size != 4:
        raise ValueError("camera.eye / camera.at must be homogeneous 4-vectors, camera.up a 3- or 4-vector")
    if shading == "numpy" and isinstance(camera["up"], (list, tuple)):
        # the reference normalises a list-typed up in float32 (numpy/ops.py:99,109): hand over the finished y axis
        with np.errstate(all="ignore"):
            unit = unit_up(camera["up"], up)
        if np.all(np.isfinite(unit)):
            up = np.append(unit, 0.0)
            cam.up_is_unit = 1
    cam.eye[:] = eye.tolist()
    cam.at[:] = at.tolist()
    cam.up[:] = up.tolist()
    cam.fovy = scalar(camera["fovy"])
    cam.focal_length = scalar(camera["focal_length"])
    cam.near_clip = scalar(camera["near"])
    cam.far_clip = scalar(camera["far"])
    vp = [int(v) for v in np.ravel(_host_view(camera["viewport"]) if not isinstance(camera["viewport"], torch.Tensor)
                                   else camera["viewport"].cpu().numpy())]
    cam.viewport[:] = vp
    proj = str(camera.get("proj_type", "perspective"))
    if proj in ("ortho", "orthographic"):
        cam.ortho = 1                    # torch/utils.py:461: only the torch backend's semantics have it
    elif proj not in ("persp", "perspective"):
        raise ValueError(f"camera.proj_type {proj!r}: expected 'perspective' or 'ortho'")
    return cam


_CAMERA_LEAVES = ("eye", "at", "up")


def camera_leaves(camera: Dict[str, Any], shading: str) -> Dict[str, torch.Tensor]:
    """The camera's differentiable leaves: those of ``eye``, ``at`` and ``up`` that are tensors with ``requires_grad``,
    under ``shading='torch'``.  The numpy backend's semantics keep detaching the camera (a different, non-orthonormal
    basis, and no autograd in the reference); ``fovy`` and ``focal_length`` never get a gradient (the reference passes
    them through numpy)."""
    if shading != "torch":
        return {}
    return {k: camera[k] for k in _CAMERA_LEAVES
            if isinstance(camera.get(k), torch.Tensor) and camera[k].requires_grad}


def frame_size(cam: _lib.SrhCamera) -> Tuple[int, int]:
    return cam.viewport[2] - cam.viewport[0], cam.viewport[3] - cam.viewport[1]


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# What a workspace's bin counters hold is known only to whoever used it last, so it is noted ON the tensor object (the
# note dies with it; a new tensor over recycled memory starts unknown): ("clean", layout) after a binned frame whose
# render kernel left every counter at zero, ("binned", layout) between a frame's two stages.  A clean workspace needs
# no clearing launch (SrhParams.counters_clean): a frame is then two kernels.
def _ws_state(ws: torch.Tensor):
    return getattr(ws, "_srh_state", None)


def _ws_note(ws: torch.Tensor, state) -> None:
    try:
        ws._srh_state = state
    except AttributeError:                                  # a tensor type that takes no attributes: always unknown
        pass


def _layout_key(buf: "SceneBuffers", width: int, height: int, what="frame"):
    ob = buf.objects
    return (what, tuple((ob.seg[s].type, ob.seg[s].count) for s in range(ob.n_segments)), int(width), int(height))


class _Shade(NamedTuple):
    """How a frame is shaded: the model (``'numpy'`` | ``'torch'``), the torch model's ``double_sided`` and
    ``use_quartic``, whether the shadow-ray pass runs and whether the ``normal`` / ``pos`` outputs are written."""
    shading: str = "numpy"
    double_sided: bool = False
    use_quartic: bool = False
    shadow: bool = False
    aux: bool = False


def _rows(rows: Optional[Tuple[int, int]], height: int) -> Tuple[int, int]:
    """The row slab ``rows`` as (r0, r1); None is the whole frame."""
    return (0, height) if rows is None else (int(rows[0]), int(rows[1]))


def _params(buf: SceneBuffers, rows: Tuple[int, int], mode: str, shade: _Shade, **fields) -> _lib.SrhParams:
    """SrhParams of a call over the resolved ``rows``: the scene's tonemap, ``mode``, ``shade``'s options and the call's
    own ``fields``."""
    return _lib.SrhParams(row0=rows[0], row1=rows[1], mode=_lib.MODES[mode], tonemap_gamma=0 if buf.gamma is None else 1,
                          gamma=1.0 if buf.gamma is None else buf.gamma, shading=_lib.SHADING[shade.shading],
                          double_sided=int(bool(shade.double_sided)), use_quartic=int(bool(shade.use_quartic)), **fields)


def render_buffers(buf: SceneBuffers, cam: _lib.SrhCamera, rows: Optional[Tuple[int, int]] = None,
                   mode: str = "auto", out: Optional[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = None,
                   want_nearest: bool = True, events: Optional[_lib.EventPair] = None,
                   workspace: Optional[torch.Tensor] = None, shading: str = "numpy", double_sided: bool = False,
                   use_quartic: bool = False, aux: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
                   waves_per_tile: int = 0, stages: int = 0):
    """One frame (or the row slab ``rows=(r0, r1)`` of it) from resident buffers.  Everything is
    enqueued on the current stream of ``buf.device``; nothing synchronises.  ``out`` may supply
    preallocated (image (h,W,3) f32, depth (h,W) f32, nearest (h,W) i32 or None).  ``workspace`` overrides the
    buffers' own scratch: frames in flight on different streams each need their own (``new_workspace``).
    ``stages`` (``_lib.STAGE_BIN`` / ``_lib.STAGE_RENDER``, 0 = both) splits a binned frame into its binning kernels and its
    render kernel, for a caller that runs them on two streams (``pipeline.FramePipeline``).
    ``shading='torch'`` selects the torch backend's semantics (Phong with attenuation / specular / ambient,
    ``double_sided``, ``use_quartic``, orthonormal camera, far+1 background); ``aux=(normal, pos)`` are optional
    dense (h,W,3) f32 outputs."""
    lib = _lib.load()
    width, height = frame_size(cam)
    r0, r1 = _rows(rows, height)
    h = r1 - r0
    if out is None:
        image = torch.empty((max(h, 0), width, 3), dtype=torch.float32, device=buf.device)
        depth = torch.empty((max(h, 0), width), dtype=torch.float32, device=buf.device)
        nearest = torch.empty((max(h, 0), width), dtype=torch.int32, device=buf.device) if want_nearest else None
    else:
        image, depth, nearest = out
        for t, shape, dt in ((image, (h, width, 3), torch.float32), (depth, (h, width), torch.float32),
                             (nearest, (h, width), torch.int32)):
            if t is None:
                continue
            inner = tuple(t.stride()[1:]) == ((3, 1) if len(shape) == 3 else (1,))
            if tuple(t.shape) != shape or t.dtype != dt or not inner or t.device != buf.device:
                raise ValueError(f"out buffer mismatch: want {dt} {shape} with dense rows on {buf.device}, "
                                 f"got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    params = _params(buf, (r0, r1), mode, _Shade(shading, double_sided, use_quartic))
    # this call's own fields are assigned here, not forwarded through _params as keywords: that costs a microsecond of
    # host time per frame
    params.waves_per_tile = int(waves_per_tile)
    params.stages = int(stages)
    if aux:
        params.normal_out = aux[0].data_ptr() if aux[0] is not None else None
        params.pos_out = aux[1].data_ptr() if aux[1] is not None else None
    if h > 1:
        params.image_row_stride = image.stride(0)
        params.depth_row_stride = depth.stride(0)
        params.nearest_row_stride = nearest.stride(0) if nearest is not None else 0
    if events:
        params.ev_start, params.ev_stop = events.start, events.stop
    if workspace is None:
        workspace = buf.ensure_workspace(width, height)
    binned = mode in ("auto", "binned") and not cam.ortho
    after = None
    if binned:
        key = _layout_key(buf, width, height)
        halves = int(stages) & (_lib.STAGE_BIN | _lib.STAGE_RENDER) or (_lib.STAGE_BIN | _lib.STAGE_RENDER)
        state = _ws_state(workspace)
        if halves & _lib.STAGE_BIN:
            params.counters_clean = int(state == ("clean", key))
        elif state != ("binned", key):
            raise ValueError("stages=STAGE_RENDER needs the bins of a stages=STAGE_BIN call with the same scene and "
                             "frame size in this workspace (its last use left it " +
                             ("without any" if state is None else f"{state[0]}") + ")")
        after = ("binned", key) if (not halves & _lib.STAGE_RENDER or int(stages) & _lib.STAGE_KEEP_BINS) else ("clean", key)
        _ws_note(workspace, None)                           # unknown until the call has been accepted
    with torch.cuda.device(buf.device):
        rc = lib.srh_render_fwd(C.byref(cam), C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials),
                                C.byref(params), workspace.data_ptr(), workspace.numel(),
                                image.data_ptr(), depth.data_ptr(),
                                nearest.data_ptr() if nearest is not None else None, _stream_ptr(buf.device))
    _lib.check(rc)
    if binned:
        _ws_note(workspace, after)
    return image, depth, nearest


def bin_statistics(buf: SceneBuffers, cam: _lib.SrhCamera, rows: Optional[Tuple[int, int]] = None) -> Dict[str, Any]:
    """What one binned frame really tests (measurement; synchronises).  Runs the frame's binning stage alone on a scratch
    workspace of its own and reads the list lengths back: ``entries`` (batches, tile rows, tile columns) = candidates of
    every 16 x 16-pixel tile's bins, ``wide`` (batches,) = primitives on the frame-wide lists that every tile tests,
    ``executed_pair_tests`` = sum over tiles of (bin entries + frame-wide entries) x 256 pixels -- the (pixel, primitive)
    pairs that go through the fp32 reject test, against ``algorithmic_pair_tests`` = primitives x pixels that the
    reference evaluates -- and ``tile_row_cost``, the per-tile-row sums ``dist.cost_weighted_slabs`` partitions."""
    lib = _lib.load()
    width, height = frame_size(cam)
    r0, r1 = _rows(rows, height)
    ws = buf.new_workspace(width, height)
    image = torch.empty((r1 - r0, width, 3), dtype=torch.float32, device=buf.device)
    depth = torch.empty((r1 - r0, width), dtype=torch.float32, device=buf.device)
    render_buffers(buf, cam, rows=(r0, r1), mode="binned", out=(image, depth, None), workspace=ws, stages=_lib.STAGE_BIN)
    off, tx, ty, pad, cap = C.c_size_t(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(lib.srh_bin_counters(C.byref(buf.objects), width, height, r0, r1, C.byref(off), C.byref(tx), C.byref(ty),
                                    C.byref(pad), C.byref(cap)))
    nseg = buf.objects.n_segments
    words = ws[off.value:off.value + 4 * (64 + nseg * pad.value)].view(torch.int32).cpu().numpy().astype(np.int64)
    which = int(words[9]) & 1
    wide = np.minimum(words[4 * which:4 * which + nseg], np.asarray(buf.counts, dtype=np.int64))
    bins = words[64:64 + nseg * pad.value].reshape(nseg, pad.value)[:, :tx.value * ty.value]
    entries = np.minimum(bins, cap.value).reshape(nseg, ty.value, tx.value)
    per_tile = entries.sum(axis=0) + int(wide.sum())
    return {"entries": entries, "wide": wide, "bin_capacity": cap.value,
            "executed_pair_tests": int(per_tile.sum()) * 256,
            "algorithmic_pair_tests": int(buf.total) * (r1 - r0) * width,
            "tile_row_cost": per_tile.sum(axis=1)}


def generate_rays(camera: Dict[str, Any], device="cuda", rows: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """``ray_dir`` as the reference returns it: (4, N) unit directions, row-major over the image
    (numpy/renderer.py:145-169)."""
    device = torch.device(device)
    _require_gpu(device)
    lib = _lib.load()
    cam = camera_struct(camera)
    width, height = frame_size(cam)
    r0, r1 = _rows(rows, height)
    out = torch.empty((4, max(r1 - r0, 0) * width), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.srh_generate_rays(C.byref(cam), r0, r1, out.data_ptr(), _stream_ptr(device)))
    return out


def _float_keys(buf: SceneBuffers, shading: str = "numpy") -> List[str]:
    """Keys of buf.tensors that are differentiable inputs, in a fixed order (the torch shading model adds its own
    inputs where the scene has them)."""
    keys = [f"{kind}.{name}" for kind in buf.kinds for name in _OBJ_FIELDS[kind]]
    return keys + [k for k, leaf in _SCENE_LEAVES.items()
                   if leaf.grad and k in buf.tensors and (shading == "torch" or not leaf.torch_only)]


def shadow_pass(buf: SceneBuffers, cam: _lib.SrhCamera, rows, image: torch.Tensor, depth: torch.Tensor,
                nearest: torch.Tensor, double_sided: bool = False, use_quartic: bool = False,
                all_pairs: bool = False) -> torch.Tensor:
    """The torch backend's ``shadow=True`` (torch/renderer.py:291-314) over a frame rendered with
    ``shading='torch'``: re-shades ``image`` in place with per-light visibility from shadow rays and returns the
    (rows, W) int64 visibility bit field (bit l = light l visible).  Candidates come from tile bins in each light's
    screen space; ``all_pairs=True`` runs the reference's O(pixels x lights x primitives) loop instead (same result)."""
    lib = _lib.load()
    width, height = frame_size(cam)
    r0, r1 = _rows(rows, height)
    vis = torch.empty((r1 - r0, width), dtype=torch.int64, device=buf.device)
    params = _params(buf, (r0, r1), "exact" if all_pairs else "auto", _Shade("torch", double_sided, use_quartic))
    if all_pairs:
        workspace = buf.ensure_workspace(width, height)
    else:
        workspace = buf.ensure_shadow_workspace(width, height)
    with torch.cuda.device(buf.device):
        _lib.check(lib.srh_shadow_shade(C.byref(cam), C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials),
                                        C.byref(params), workspace.data_ptr(), workspace.numel(), nearest.data_ptr(),
                                        depth.data_ptr(), image.data_ptr(), vis.data_ptr(), _stream_ptr(buf.device)))
    return vis


def _frame(buf: SceneBuffers, cam: _lib.SrhCamera, rows, mode: str, shade: _Shade, waves_per_tile: int = 0,
           workspace: Optional[torch.Tensor] = None):
    """render_buffers with what ``shade`` asks for around it: image, depth, nearest, the (normal, pos) buffers with
    ``shade.aux`` (else None) and the shadow pass's visibility with ``shade.shadow`` (else None)."""
    aux = _aux_buffers(cam, rows, buf.device) if shade.aux else None
    image, depth, nearest = render_buffers(buf, cam, rows=rows, mode=mode, shading=shade.shading,
                                           double_sided=shade.double_sided, use_quartic=shade.use_quartic, aux=aux,
                                           waves_per_tile=waves_per_tile, workspace=workspace)
    vis = shadow_pass(buf, cam, rows, image, depth, nearest, shade.double_sided, shade.use_quartic) if shade.shadow else None
    return image, depth, nearest, aux, vis


class _RenderFunction(torch.autograd.Function):
    """render_buffers with the analytic backward of libsrh (srh_render_bwd).  Gradient semantics are those of
    autograd through the reference's torch backend (SURVEY.md section 8, row a-B): selection and masks are piecewise
    constant; a disc's radius and a triangle's vertices 1, 2 receive zero gradient.  With ``shade.aux`` (torch shading
    only) the outputs are image, depth, nearest, normal, pos, and upstream gradients of normal / pos go to
    srh_render_bwd_aux.  ``cam_names`` names the camera leaves (``camera_leaves``) that follow the scene's inputs at the
    end of ``inputs``: the forward reads their values through ``cam`` as always, the backward is srh_render_bwd_camera
    and returns their gradients in each leaf's own shape, dtype and device (w = 0; a 3-vector ``up`` gets 3 values)."""

    @staticmethod
    def forward(ctx, buf, cam, rows, mode, shade: _Shade, cam_names, *inputs):
        if shade.aux:
            ctx.set_materialize_grads(False)            # an unused normal / pos must arrive as None, not as zeros
        image, depth, nearest, aux, vis = _frame(buf, cam, rows, mode, shade)
        ctx.buf, ctx.cam, ctx.rows, ctx.mode, ctx.shade = buf, cam, rows, mode, shade
        ctx.cam_names = tuple(cam_names)
        ctx.cam_like = [(t.shape, t.dtype, t.device) for t in inputs[len(inputs) - len(ctx.cam_names):]]
        ctx.save_for_backward(depth, nearest, vis)
        ctx.mark_non_differentiable(nearest)
        return (image, depth, nearest) + (aux or ())

    @staticmethod
    def backward(ctx, g_image, g_depth, _g_nearest, g_normal=None, g_pos=None):
        depth, nearest, vis = ctx.saved_tensors
        keys = _float_keys(ctx.buf, ctx.shade.shading)
        need = ctx.needs_input_grad[6:]
        cam_need = tuple(k for k, want in zip(ctx.cam_names, need[len(keys):]) if want)
        grads = _render_backward(ctx.buf, ctx.cam, ctx.rows, ctx.mode, ctx.shade, depth, nearest, vis, g_image, g_depth,
                                 need[:len(keys)], g_normal, g_pos, camera=cam_need)
        cam_grads = []
        for k, (shape, dtype, device) in zip(ctx.cam_names, ctx.cam_like):
            g = grads.get("camera." + k)
            cam_grads.append(None if g is None else g[:int(np.prod(shape))].to(device=device, dtype=dtype).reshape(shape))
        return (None, None, None, None, None, None) + tuple(grads.get(k) for k in keys) + tuple(cam_grads)


def _forward(buf: SceneBuffers, cam: _lib.SrhCamera, rows, mode: str, shade: _Shade, inputs: Sequence[torch.Tensor],
             differentiable: bool, waves_per_tile: int = 0, cam_leaves: Optional[Dict[str, torch.Tensor]] = None):
    """One frame for ``render`` and ``ResidentScene.render``: through ``_RenderFunction`` when ``differentiable`` (the
    shadow pass, if any, then runs inside it), else straight from ``_frame``.  Returns image, depth, nearest and a dict
    of the extra outputs: ``normal`` and ``pos`` with ``shade.aux``, and outside autograd ``light_visibility`` with
    ``shade.shadow``.  ``cam_leaves`` (``camera_leaves``) become inputs of the function beside the scene's."""
    if differentiable:
        cam_leaves = cam_leaves or {}
        out = _RenderFunction.apply(buf, cam, rows, mode, shade, tuple(cam_leaves), *inputs, *cam_leaves.values())
        return out[0], out[1], out[2], ({"normal": out[3], "pos": out[4]} if shade.aux else {})
    image, depth, nearest, aux, vis = _frame(buf, cam, rows, mode, shade, waves_per_tile)
    extra = {"normal": aux[0], "pos": aux[1]} if aux else {}
    if vis is not None:
        extra["light_visibility"] = vis
    return image, depth, nearest, extra


def _render_backward(buf: SceneBuffers, cam: _lib.SrhCamera, rows, mode: str, shade: _Shade, depth: torch.Tensor,
                     nearest: torch.Tensor, vis: Optional[torch.Tensor], g_image: Optional[torch.Tensor],
                     g_depth: Optional[torch.Tensor], need: Sequence[bool], g_normal: Optional[torch.Tensor] = None,
                     g_pos: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                     camera: Sequence[str] = ()) -> Dict[str, torch.Tensor]:
    """srh_render_bwd: gradients of the inputs named by ``_float_keys`` (those with ``need``) for the upstream gradients
    of image and depth, from the winners the forward pass saved.  Everything is enqueued on the current stream.
    With an upstream gradient of the torch shading's ``normal`` or ``pos`` output the call is srh_render_bwd_aux
    instead; there a missing ``g_image`` is passed as NULL (the geometry-only kernel) rather than as zeros.
    ``workspace`` defaults to the buffers' own scratch (``ensure_workspace``).  ``camera`` names the camera leaves
    (of 'eye', 'at', 'up') whose gradients are wanted too: the call is then srh_render_bwd_camera, and they come back as
    (4,) float32 device tensors under 'camera.eye' / 'camera.at' / 'camera.up'."""
    lib = _lib.load()
    width, height = frame_size(cam)
    r0, r1 = _rows(rows, height)
    keys = _float_keys(buf, shade.shading)
    grads: Dict[str, torch.Tensor] = {}
    sg = _lib.SrhGrads()
    for key, want in zip(keys, need):
        if not want:
            continue
        g = torch.zeros_like(buf.tensors[key])
        grads[key] = g
        if key in _SCENE_LEAVES:
            setattr(sg, _SCENE_LEAVES[key].grad, g.data_ptr())
        elif key != "disk.radius":            # identically zero (numpy/renderer.py:88: the radius only feeds a mask)
            kind, name = key.split(".")
            getattr(sg, name)[buf.kinds.index(kind)] = g.data_ptr()
    aux = g_normal is not None or g_pos is not None
    if camera and shade.shading != "torch":
        raise ValueError("camera gradients exist only in the torch backend's semantics: shading='torch'")
    g_image = g_image.to(torch.float32).contiguous() if g_image is not None else \
        (None if aux or (camera and g_depth is not None) else torch.zeros((r1 - r0, width, 3), dtype=torch.float32, device=buf.device))
    g_depth = g_depth.to(torch.float32).contiguous() if g_depth is not None else None
    g_normal = g_normal.to(torch.float32).contiguous() if g_normal is not None else None
    g_pos = g_pos.to(torch.float32).contiguous() if g_pos is not None else None
    params = _params(buf, (r0, r1), mode, shade, visibility=vis.data_ptr() if vis is not None else None)
    if workspace is None:
        workspace = buf.ensure_workspace(width, height)
    def ptr(t):
        return t.data_ptr() if t is not None else None

    with torch.cuda.device(buf.device):
        if camera:
            cg = _lib.SrhCameraGrads()
            for k in camera:
                grads["camera." + k] = torch.empty(4, dtype=torch.float32, device=buf.device)
                setattr(cg, k, grads["camera." + k].data_ptr())
            scratch = buf.ensure_camera_scratch(width, r1 - r0)
            rc = lib.srh_render_bwd_camera(C.byref(cam), C.byref(buf.objects), C.byref(buf.lights),
                                           C.byref(buf.materials), C.byref(params), workspace.data_ptr(),
                                           workspace.numel(), ptr(g_image), ptr(g_depth), ptr(g_normal), ptr(g_pos),
                                           nearest.data_ptr(), depth.data_ptr(), C.byref(sg), C.byref(cg),
                                           scratch.data_ptr(), scratch.numel() * 8, _stream_ptr(buf.device))
        elif aux:
            rc = lib.srh_render_bwd_aux(C.byref(cam), C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials),
                                        C.byref(params), workspace.data_ptr(), workspace.numel(), ptr(g_image),
                                        ptr(g_depth), ptr(g_normal), ptr(g_pos), nearest.data_ptr(), depth.data_ptr(),
                                        C.byref(sg), _stream_ptr(buf.device))
        else:
            rc = lib.srh_render_bwd(C.byref(cam), C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials),
                                    C.byref(params), workspace.data_ptr(), workspace.numel(),
                                    g_image.data_ptr(), g_depth.data_ptr() if g_depth is not None else None,
                                    nearest.data_ptr(), depth.data_ptr(), C.byref(sg), _stream_ptr(buf.device))
    _lib.check(rc)
    return grads


class ViewScenes:
    """One scene per view, as srh_render_views takes it (SrhParams.per_view): arrays of SrhObjects / SrhLights /
    SrhMaterials that equal the base scene's except for the pointers a view overrides.  ``overrides[v]`` maps flat leaf
    names (``"disk.pos"``, ``"disk.normal"``, ``"lights.pos"``, ``"colors"``, ``"materials.albedo"``, ...: the keys of
    ``SceneBuffers.tensors``) to arrays or tensors of the base leaf's shape -- what the reference's batch loop assigns
    per element before each ``render()`` (diffrend/torch/GAN/gan.py:325-378: ``disk.pos``, ``disk.normal``,
    ``lights.pos``).  float32 contiguous tensors on the device are used in place; everything else is converted."""

    def __init__(self, buf: SceneBuffers, overrides: Sequence[Dict[str, Any]]):
        n = len(overrides)
        self.n, self.mask, self.keep = n, 0, []
        self.keys: List[Dict[str, torch.Tensor]] = [{} for _ in range(n)]      # per view: leaf key -> the tensor it reads
        self.objects = (_lib.SrhObjects * n)(*[_lib.SrhObjects.from_buffer_copy(buf.objects) for _ in range(n)])
        self.lights = (_lib.SrhLights * n)(*[_lib.SrhLights.from_buffer_copy(buf.lights) for _ in range(n)])
        self.materials = (_lib.SrhMaterials * n)(*[_lib.SrhMaterials.from_buffer_copy(buf.materials) for _ in range(n)])
        for v, ov in enumerate(overrides):
            for key, val in (ov or {}).items():
                base = buf.tensors.get(key)
                if base is None:
                    raise KeyError(f"view {v}: {key!r} is not a leaf of this scene (leaves: {sorted(buf.tensors)})")
                t = _as_tensor(val, base.dtype, buf.device)
                if not t.is_cuda:
                    t = t.to(buf.device)
                t = t.reshape(base.shape) if t.numel() == base.numel() else t
                if tuple(t.shape) != tuple(base.shape):
                    raise ValueError(f"view {v}: {key} has shape {tuple(t.shape)}, the scene's leaf {tuple(base.shape)}")
                self.keep.append(t)
                self.keys[v][key] = t
                leaf = _SCENE_LEAVES.get(key)
                if leaf is not None:
                    setattr(getattr(self, leaf.struct)[v], leaf.path[-1], t.data_ptr())
                    self.mask |= _lib.VIEWS_LIGHTS if leaf.struct == "lights" else _lib.VIEWS_MATERIALS
                else:
                    kind, field = key.split(".")
                    setattr(self.objects[v].seg[buf.kinds.index(kind)], field, t.data_ptr())
                    self.mask |= _lib.VIEWS_OBJECTS

    def view(self, buf: SceneBuffers, v: int) -> SceneBuffers:
        """The scene of view v as resident buffers of its own (for the per-view passes: shadows)."""
        import copy
        one = copy.copy(buf)
        one.objects, one.lights, one.materials = self.objects[v], self.lights[v], self.materials[v]
        return one


def render_views_buffers(buf: SceneBuffers, cams: Sequence[_lib.SrhCamera], images: torch.Tensor, depths: torch.Tensor,
                         nearests: Optional[torch.Tensor] = None, rows: Optional[Tuple[int, int]] = None,
                         workspace: Optional[torch.Tensor] = None, image_row_stride: int = 0,
                         depth_row_stride: int = 0, view_row0: Optional[Sequence[int]] = None,
                         scenes: Optional[ViewScenes] = None, mode: str = "auto", first_view: int = 0,
                         aux: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
                         **shading_kw) -> torch.Tensor:
    """Low-level form of ``render_views``: resident scene buffers, camera structs, caller-provided stacked outputs
    (view v starts v * rows * row_stride elements after view 0) and an optional row slab; with ``view_row0`` view v
    renders rows [view_row0[v], view_row0[v] + rows[1] - rows[0]) instead; ``scenes`` gives every view its own
    geometry / lights / materials (``ViewScenes``), camera i drawing view ``first_view + i`` of it.  ``mode`` is
    'auto' or 'binned'.  ``aux=(normals, poses)`` are optional stacked dense (n,rows,W,3) float32 outputs of the torch
    shading (srh_render_views_aux).  One library call, every pipeline kernel launched once for the whole batch.  Returns
    the workspace (pass it back in to reuse it)."""
    lib = _lib.load()
    width, height = frame_size(cams[0])
    n = len(cams)
    shade = _Shade(shading_kw.get("shading", "numpy"), shading_kw.get("double_sided", False),
                   shading_kw.get("use_quartic", False))
    params = _params(buf, _rows(rows, height), mode, shade, waves_per_tile=int(shading_kw.get("waves_per_tile", 0)),
                     image_row_stride=int(image_row_stride), depth_row_stride=int(depth_row_stride))
    row0_arr = None
    if view_row0 is not None:
        if len(view_row0) != n:
            raise ValueError("view_row0 needs one entry per view")
        row0_arr = (C.c_int32 * n)(*[int(r) for r in view_row0])
        params.view_row0 = C.cast(row0_arr, C.c_void_p)
    nbytes = lib.srh_workspace_bytes_views(C.byref(buf.objects), width, height, n)
    if nbytes == 0:
        raise _lib.SrhError(-2, lib.srh_last_error().decode())
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=buf.device)
    arr = (_lib.SrhCamera * n)(*cams)
    binned = not cams[0].ortho
    key = _layout_key(buf, width, height, ("views", n))
    if binned:
        params.counters_clean = int(_ws_state(workspace) == ("clean", key))
        _ws_note(workspace, None)
    ob, ls, ms = C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials)
    if scenes is not None:
        if first_view < 0 or first_view + n > scenes.n:
            raise ValueError(f"{scenes.n} per-view scenes for {n} cameras from view {first_view}")
        params.per_view = scenes.mask
        if scenes.mask & _lib.VIEWS_OBJECTS:
            ob = C.byref(scenes.objects[first_view])
        if scenes.mask & _lib.VIEWS_LIGHTS:
            ls = C.byref(scenes.lights[first_view])
        if scenes.mask & _lib.VIEWS_MATERIALS:
            ms = C.byref(scenes.materials[first_view])
    if aux is not None:
        for t in aux:
            if t is not None and (tuple(t.shape) != (n, params.row1 - params.row0, width, 3) or t.dtype != torch.float32
                                  or not t.is_contiguous() or t.device != buf.device):
                raise ValueError(f"aux buffer mismatch: want contiguous float32 {(n, params.row1 - params.row0, width, 3)} "
                                 f"on {buf.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    with torch.cuda.device(buf.device):
        args = (n, arr, ob, ls, ms, C.byref(params), workspace.data_ptr(), workspace.numel(), images.data_ptr(),
                depths.data_ptr(), nearests.data_ptr() if nearests is not None else None)
        if aux is None:
            _lib.check(lib.srh_render_views(*args, _stream_ptr(buf.device)))
        else:
            _lib.check(lib.srh_render_views_aux(*args, aux[0].data_ptr() if aux[0] is not None else None,
                                                aux[1].data_ptr() if aux[1] is not None else None,
                                                _stream_ptr(buf.device)))
    if binned:
        _ws_note(workspace, ("clean", key))
    return workspace


def render_views_bwd_buffers(buf: SceneBuffers, cams: Sequence[_lib.SrhCamera], g_images: Optional[torch.Tensor],
                             g_depths: Optional[torch.Tensor], nearests: torch.Tensor, depths: torch.Tensor, grads,
                             workspace: Optional[torch.Tensor] = None, scenes: Optional[ViewScenes] = None,
                             first_view: int = 0, visibility: Optional[torch.Tensor] = None,
                             g_normals: Optional[torch.Tensor] = None, g_poses: Optional[torch.Tensor] = None,
                             camera_grads=None, camera_scratch: Optional[torch.Tensor] = None,
                             **shading_kw) -> torch.Tensor:
    """Low-level form of the backward of ``render_views`` (srh_render_views_bwd): the views of ``cams`` in one call, from
    stacked contiguous upstream gradients ``g_images`` (n,H,W,3) and ``g_depths`` (n,H,W) or None, the forward's stacked
    ``nearests`` / ``depths`` and, for a ``shadow=True`` forward, its stacked ``visibility``.  ``grads`` is a ctypes
    array of n ``_lib.SrhGrads``: where each view's gradients are ADDED (the same pointer in every struct for a leaf the
    views share; zero-filled by the caller).  ``scenes`` / ``first_view`` as in ``render_views_buffers``.  The bin
    counters of ``workspace`` are not touched: what is noted about them stays true.  Returns the workspace.

    With ``g_normals`` / ``g_poses`` (stacked contiguous (n,H,W,3) upstream gradients of the torch shading's ``normal`` /
    ``pos`` outputs), ``camera_grads`` (a ctypes array of n ``_lib.SrhCameraGrads``: where each view's eye / at / up
    gradients are WRITTEN, 4 floats each) or ``camera_scratch`` the call is srh_render_views_bwd_camera instead; there
    ``g_images`` may be None (the geometry-only kernel) as long as one upstream gradient is given, and ``camera_scratch``
    defaults to the buffers' own (``ensure_camera_scratch_views``) when ``camera_grads`` is given."""
    lib = _lib.load()
    width, height = frame_size(cams[0])
    n = len(cams)
    shade = _Shade(shading_kw.get("shading", "numpy"), shading_kw.get("double_sided", False),
                   shading_kw.get("use_quartic", False))
    params = _params(buf, (0, height), "auto", shade, visibility=visibility.data_ptr() if visibility is not None else None)
    nbytes = lib.srh_workspace_bytes_views(C.byref(buf.objects), width, height, n)
    if nbytes == 0:
        raise _lib.SrhError(-2, lib.srh_last_error().decode())
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=buf.device)
    state = _ws_state(workspace)
    if state is not None and state[1] != _layout_key(buf, width, height, ("views", n)):
        _ws_note(workspace, None)                           # another batch size's layout: its counters may lie under records
    arr = (_lib.SrhCamera * n)(*cams)
    ob, ls, ms = C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials)
    if scenes is not None:
        if first_view < 0 or first_view + n > scenes.n:
            raise ValueError(f"{scenes.n} per-view scenes for {n} cameras from view {first_view}")
        params.per_view = scenes.mask
        if scenes.mask & _lib.VIEWS_OBJECTS:
            ob = C.byref(scenes.objects[first_view])
        if scenes.mask & _lib.VIEWS_LIGHTS:
            ls = C.byref(scenes.lights[first_view])
        if scenes.mask & _lib.VIEWS_MATERIALS:
            ms = C.byref(scenes.materials[first_view])
    def ptr(t):
        return t.data_ptr() if t is not None else None

    with torch.cuda.device(buf.device):
        if g_normals is None and g_poses is None and camera_grads is None and camera_scratch is None:
            _lib.check(lib.srh_render_views_bwd(n, arr, ob, ls, ms, C.byref(params), workspace.data_ptr(),
                                                workspace.numel(), g_images.data_ptr(), ptr(g_depths),
                                                nearests.data_ptr(), depths.data_ptr(), grads, _stream_ptr(buf.device)))
        else:
            if camera_grads is not None and camera_scratch is None:
                camera_scratch = buf.ensure_camera_scratch_views(width, height, n)
            _lib.check(lib.srh_render_views_bwd_camera(
                n, arr, ob, ls, ms, C.byref(params), workspace.data_ptr(), workspace.numel(), ptr(g_images), ptr(g_depths),
                ptr(g_normals), ptr(g_poses), nearests.data_ptr(), depths.data_ptr(), grads, camera_grads,
                ptr(camera_scratch), camera_scratch.numel() * camera_scratch.element_size() if camera_scratch is not None else 0,
                _stream_ptr(buf.device)))
    return workspace


class _ViewsCall(NamedTuple):
    """What one ``render_views`` call renders: the resident scene, the camera structs, the per-view scenes (or None) and
    the call's options."""
    buf: SceneBuffers
    cams: List[_lib.SrhCamera]
    every: Optional[ViewScenes]
    mode: str
    streams: int
    want_nearest: bool
    batch: int
    shadow: bool
    shading_kw: Dict[str, Any]
    aux: bool = False


def _views_forward(call: _ViewsCall) -> Tuple[Dict[str, torch.Tensor], Optional[torch.Tensor]]:
    """The forward of ``render_views``: the result dict and the workspace of the batched path (None round-robin)."""
    buf, cams, every, mode, shading_kw = call.buf, call.cams, call.every, call.mode, call.shading_kw
    device, want_nearest, shadow = buf.device, call.want_nearest, call.shadow
    width, height = frame_size(cams[0])
    n = len(cams)
    image = torch.empty((n, height, width, 3), dtype=torch.float32, device=device)
    depth = torch.empty((n, height, width), dtype=torch.float32, device=device)
    nearest = torch.empty((n, height, width), dtype=torch.int32, device=device) if want_nearest else None
    out = {"image": image, "depth": depth}
    if want_nearest:
        out["nearest"] = nearest
    normal = pos = None
    if call.aux:
        normal = out["normal"] = torch.empty((n, height, width, 3), dtype=torch.float32, device=device)
        pos = out["pos"] = torch.empty((n, height, width, 3), dtype=torch.float32, device=device)

    def scene_of(v: int) -> SceneBuffers:
        return every.view(buf, v) if every is not None else buf

    def shadows(first: int, count: int) -> None:
        if not shadow:
            return
        if "visibility" not in out:
            out["visibility"] = torch.empty((n, height, width), dtype=torch.int64, device=device)
        buf.ensure_shadow_workspace(width, height)          # the per-view copies below share it
        for v in range(first, first + count):
            out["visibility"][v] = shadow_pass(scene_of(v), cams[v], None, image[v], depth[v], nearest[v],
                                               double_sided=bool(shading_kw.get("double_sided", False)),
                                               use_quartic=bool(shading_kw.get("use_quartic", False)))

    if mode in ("auto", "binned") and int(call.batch) > 0:
        step = max(1, min(int(call.batch), n))
        workspace = None                                    # sized by the first (largest) batch, reused by the others
        for i in range(0, n, step):
            m = min(step, n - i)
            workspace = render_views_buffers(buf, cams[i:i + m], image[i:i + m], depth[i:i + m],
                                             nearest[i:i + m] if want_nearest else None, workspace=workspace,
                                             scenes=every, mode=mode, first_view=i,
                                             aux=(normal[i:i + m], pos[i:i + m]) if call.aux else None, **shading_kw)
            shadows(i, m)
        return out, workspace
    n_streams = max(1, min(int(call.streams), n))
    pool = [torch.cuda.Stream(device) for _ in range(n_streams)]
    scratch = [buf.new_workspace(width, height) for _ in range(n_streams)]
    current = torch.cuda.current_stream(device)
    for st in pool:
        st.wait_stream(current)                 # uploads and allocations above happen-before the views
    for v, cam in enumerate(cams):
        k = v % n_streams
        with torch.cuda.stream(pool[k]):
            render_buffers(scene_of(v), cam, mode=mode, out=(image[v], depth[v], nearest[v] if want_nearest else None),
                           workspace=scratch[k], aux=(normal[v], pos[v]) if call.aux else None, **shading_kw)
    for st in pool:
        current.wait_stream(st)
    for t in (image, depth, nearest, normal, pos, *scratch, *buf.tensors.values(), *(every.keep if every is not None else ())):
        if t is not None:
            t.record_stream(current)
    shadows(0, n)
    return out, None


class _RenderViewsFunction(torch.autograd.Function):
    """``render_views`` with the batched analytic backward of libsrh: one library call, and one backward launch, per
    chunk of views.  ``inputs`` are the scene's shared leaves (``_float_keys``), then the override tensors named by
    ``slots`` = ((view, key), ...), then the camera leaves named by ``cam_slots`` = ((view, 'eye' | 'at' | 'up'), ...).
    Gradient semantics are ``_RenderFunction``'s per view; a shared leaf gets the sum over the views that read it, an
    override tensor and a camera leaf the gradient of its own view (the camera's in the leaf's own shape, dtype and
    device, w = 0).  The outputs are image, depth, nearest, then ``visibility`` with ``call.shadow``, then ``normal`` and
    ``pos`` with ``call.aux``.  The backward is srh_render_views_bwd; with an upstream gradient of normal / pos, or a
    camera leaf that needs its gradient, it is srh_render_views_bwd_camera."""

    @staticmethod
    def forward(ctx, call: _ViewsCall, slots, cam_slots, *inputs):
        if call.aux:
            ctx.set_materialize_grads(False)            # an unused normal / pos must arrive as None, not as zeros
        out, workspace = _views_forward(call)
        ctx.call, ctx.slots, ctx.cam_slots, ctx.workspace = call, tuple(slots), tuple(cam_slots), workspace
        n_cam = len(ctx.cam_slots)
        ctx.like = [(t.shape, t.dtype, t.device) for t in inputs[len(inputs) - n_cam - len(ctx.slots):len(inputs) - n_cam]]
        ctx.cam_like = [(t.shape, t.dtype, t.device) for t in inputs[len(inputs) - n_cam:]]
        vis = out.get("visibility")
        ctx.save_for_backward(out["depth"], out["nearest"], vis)
        ctx.mark_non_differentiable(out["nearest"])
        res = (out["image"], out["depth"], out["nearest"])
        if vis is not None:
            ctx.mark_non_differentiable(vis)
            res += (vis,)
        if call.aux:
            res += (out["normal"], out["pos"])
        return res

    @staticmethod
    def backward(ctx, g_image, g_depth, _g_nearest, *g_rest):
        depth, nearest, vis = ctx.saved_tensors
        call, slots, cam_slots = ctx.call, ctx.slots, ctx.cam_slots
        buf, cams, every = call.buf, call.cams, call.every
        shading = call.shading_kw.get("shading", "numpy")
        keys = _float_keys(buf, shading)
        need = ctx.needs_input_grad[3:]
        n = len(cams)
        g_normal, g_pos = g_rest[-2:] if call.aux else (None, None)
        cam_rows = {slot: i for i, (slot, want) in enumerate(zip(cam_slots, need[len(keys) + len(slots):])) if want}
        extended = g_normal is not None or g_pos is not None or bool(cam_rows)      # srh_render_views_bwd_camera

        def dense(g):
            return g.to(torch.float32).contiguous() if g is not None else None

        if g_image is None and not (extended and (g_depth is not None or g_normal is not None or g_pos is not None)):
            g_image = torch.zeros(tuple(depth.shape) + (3,), dtype=torch.float32, device=buf.device)
        g_image, g_depth, g_normal, g_pos = dense(g_image), dense(g_depth), dense(g_normal), dense(g_pos)
        # one buffer per wanted shared leaf; one stacked buffer per overridden key, a row for every view whose override
        # wants a gradient
        shared = {k: torch.zeros_like(buf.tensors[k]) for k, want in zip(keys, need) if want}
        rows: Dict[str, Dict[int, int]] = {}
        for (v, key), want in zip(slots, need[len(keys):]):
            if want:
                rows.setdefault(key, {})[v] = len(rows.get(key, ()))
        stacked = {k: torch.zeros((len(r),) + tuple(buf.tensors[k].shape), dtype=torch.float32, device=buf.device)
                   for k, r in rows.items()}
        sg = (_lib.SrhGrads * n)()
        for v in range(n):
            own = every.keys[v] if every is not None else {}
            for key in keys:
                if key in own:                              # view v reads its own tensor: the shared leaf gets nothing from it
                    row = rows.get(key, {}).get(v)
                    g = stacked[key][row] if row is not None else None
                else:
                    g = shared.get(key)
                if g is None or key == "disk.radius":       # identically zero (numpy/renderer.py:88: the radius only feeds a mask)
                    continue
                if key in _SCENE_LEAVES:
                    setattr(sg[v], _SCENE_LEAVES[key].grad, g.data_ptr())
                else:
                    kind, name = key.split(".")
                    getattr(sg[v], name)[buf.kinds.index(kind)] = g.data_ptr()
        # the wanted camera gradients: a row of four floats each, written (not added to) by the finish kernel
        cg = cam_out = None
        if cam_rows:
            cam_out = torch.zeros((len(cam_rows), 4), dtype=torch.float32, device=buf.device)
            cg = (_lib.SrhCameraGrads * n)()
            for (v, k), i in cam_rows.items():
                setattr(cg[v], k, cam_out[i].data_ptr())
        step = min(int(call.batch) if int(call.batch) > 0 else 256, 256, n)
        workspace = ctx.workspace
        kw = {k: call.shading_kw[k] for k in ("shading", "double_sided", "use_quartic") if k in call.shading_kw}
        for i in range(0, n, step):
            m = min(step, n - i)
            chunk = (_lib.SrhGrads * m).from_buffer(sg, i * C.sizeof(_lib.SrhGrads))
            more = {}
            if extended:
                more = dict(g_normals=g_normal[i:i + m] if g_normal is not None else None,
                            g_poses=g_pos[i:i + m] if g_pos is not None else None,
                            camera_grads=(_lib.SrhCameraGrads * m).from_buffer(cg, i * C.sizeof(_lib.SrhCameraGrads))
                            if cg is not None else None)
            workspace = render_views_bwd_buffers(buf, cams[i:i + m], g_image[i:i + m] if g_image is not None else None,
                                                 g_depth[i:i + m] if g_depth is not None else None, nearest[i:i + m],
                                                 depth[i:i + m], chunk, workspace=workspace, scenes=every, first_view=i,
                                                 visibility=vis[i:i + m] if vis is not None else None, **more, **kw)
        own_grads = []
        for (v, key), (shape, dtype, device) in zip(slots, ctx.like):
            row = rows.get(key, {}).get(v)
            own_grads.append(None if row is None else stacked[key][row].to(device=device, dtype=dtype).reshape(shape))
        cam_grads = []
        on_host = cam_out.cpu() if cam_out is not None and any(d.type == "cpu" for _, _, d in ctx.cam_like) else None
        for slot, (shape, dtype, device) in zip(cam_slots, ctx.cam_like):
            i = cam_rows.get(slot)
            if i is None:
                cam_grads.append(None)
                continue
            src = on_host if (on_host is not None and device.type == "cpu") else cam_out
            cam_grads.append(src[i][:int(np.prod(shape))].to(device=device, dtype=dtype).reshape(shape))
        return (None, None, None) + tuple(shared.get(k) for k in keys) + tuple(own_grads) + tuple(cam_grads)


def render_views(scene: Dict[str, Any], cameras: Sequence[Dict[str, Any]], device="cuda", mode: str = "auto",
                 streams: int = 4, want_nearest: bool = True, batch: int = 256,
                 overrides: Optional[Sequence[Dict[str, Any]]] = None, aux: bool = False,
                 **shading_kw) -> Dict[str, torch.Tensor]:
    """Many views per call: the batch axis of the reference's real callers (one ``render()`` per view in a
    Python loop, diffrend/torch/GAN/gan.py:325-378, torch/batch_render.py:36-53).  The scene is uploaded once;
    ``overrides[v]`` replaces leaves of it for view v (``{"disk.pos": ..., "disk.normal": ..., "lights.pos": ...}``: what
    the GAN's loop assigns per batch element -- see ``ViewScenes``), so a batch may hold a different splat set and light
    per view.  In the default binned mode the views go to the library ``batch`` at a time (``srh_render_views``): every
    kernel of the frame pipeline is launched once per batch with the view as a grid dimension, so small views neither
    pay three launches each nor leave the GPU idle.  Other modes, or ``batch=0``, issue one call per view round-robin
    over ``streams`` HIP streams.  All cameras must share one viewport size.  ``shadow=True`` (with ``shading='torch'``)
    runs the shadow-ray pass on every view after its batch (torch/batch_render.py:59,104-106 renders that way by
    default); ``visibility`` (B,H,W) int64 is then returned too.  Returns stacked tensors ``image`` (B,H,W,3), ``depth``
    (B,H,W) and ``nearest`` (B,H,W) int32; ``shading`` / ``double_sided`` / ``use_quartic`` as in ``render``.
    ``aux=True`` (``shading='torch'`` only, else ValueError) adds the torch backend's ``normal`` and ``pos`` outputs,
    (B,H,W,3) float32 each, on the batched path (``srh_render_views_aux``) and round-robin alike: the hit's unit normal
    and the hit point, 0 where nothing is hit, equal to ``render``'s per view.  It is off by default: writing them costs
    24 bytes per pixel and view.

    Differentiable: with grad enabled, and a float leaf of ``scene``, a tensor in ``overrides`` or -- under
    ``shading='torch'`` -- a camera's ``eye`` / ``at`` / ``up`` tensor that requires grad, ``image`` and ``depth`` (and
    ``normal`` and ``pos`` with ``aux=True``) carry the analytic HIP backward: one library call and one backward launch
    per chunk of ``batch`` views, at most 256, however the forward ran (``srh_render_views_bwd``; with an upstream
    gradient of ``normal`` / ``pos`` or a camera leaf, ``srh_render_views_bwd_camera``, which adds one finish launch per
    chunk for the cameras).  Gradient semantics are ``render``'s for every view: a shared leaf of ``scene`` receives the
    sum over the views that read it, an override tensor -- a leaf or not, e.g. a slice of a generator's output -- the
    gradient of its own view (zeros, not None, for a view that hits nothing; a tensor given to several views the sum),
    ``disk.radius`` zeros.  Upstream gradients at pixels that hit nothing are ignored, those of ``normal`` and ``pos``
    too.  ``nearest`` is then always returned.
    Cameras: ``cameras[v]['eye' | 'at' | 'up']`` given as tensors that require grad receive their gradient in their own
    shape, dtype and device (w gets 0, a 3-vector ``up`` 3 values; zeros for a view that hits nothing), also when
    nothing else requires grad; every (view, key) pair is an input of its own, so a tensor several views share -- one
    ``up``, or rows of one (B,4) pose tensor -- gets the sum through autograd.  The camera gradients use no atomics and
    are identical from run to run.  ``shading='numpy'`` keeps detaching the cameras; ``fovy`` / ``focal_length`` get
    nothing.
    Otherwise, and under ``torch.no_grad()``, nothing of autograd is touched.  Not covered by a batch:
    ``ResidentScene`` / ``capture_step`` -- the call cannot be stream-captured, like its forward."""
    unknown = set(shading_kw) - {"shading", "double_sided", "use_quartic", "waves_per_tile", "shadow"}
    if unknown:
        raise TypeError(f"render_views() got unexpected keyword arguments {sorted(unknown)}")
    shadow = bool(shading_kw.pop("shadow", False))
    shading = shading_kw.get("shading", "numpy")
    if shadow and shading != "torch":
        raise ValueError("shadow rays exist only in the torch backend's semantics: shading='torch'")
    if aux and shading != "torch":
        raise ValueError("normal / pos outputs exist only in the torch backend's semantics: shading='torch'")
    device = torch.device(device)
    cam_slots = [(v, k) for v, cam in enumerate(cameras) for k in camera_leaves(cam, shading)] if torch.is_grad_enabled() else []

    def wants_grad(x) -> bool:
        return isinstance(x, torch.Tensor) and x.requires_grad and x.is_floating_point()

    differentiable = torch.is_grad_enabled() and (
        bool(cam_slots) or any(wants_grad(x) for x in _source_leaves(scene).values()) or
        any(wants_grad(x) for ov in (overrides or ()) for x in (ov or {}).values()))
    buf = flatten_scene(scene, device, keep_graph=differentiable)
    cams = [camera_struct(c, shading) for c in cameras]
    if not cams:
        raise ValueError("no cameras")
    width, height = frame_size(cams[0])
    if any(frame_size(c) != (width, height) for c in cams):
        raise ValueError("all cameras of a batch must have the same viewport size")
    n = len(cams)
    if overrides is not None and len(overrides) != n:
        raise ValueError(f"{len(overrides)} overrides for {n} cameras")
    every = ViewScenes(buf, overrides) if overrides is not None else None
    # the shadow pass and the backward start from the winners
    call = _ViewsCall(buf, cams, every, mode, streams, want_nearest or shadow or differentiable, batch, shadow, shading_kw,
                      bool(aux))
    if not differentiable:
        return _views_forward(call)[0]
    keys = _float_keys(buf, shading)
    slots = [(v, key) for v, ov in enumerate(overrides or ()) for key, x in (ov or {}).items()
             if key in keys and isinstance(x, torch.Tensor) and x.is_floating_point()]
    res = _RenderViewsFunction.apply(call, tuple(slots), tuple(cam_slots), *[buf.tensors[k] for k in keys],
                                     *[overrides[v][key] for v, key in slots], *[cameras[v][k] for v, k in cam_slots])
    out = {"image": res[0], "depth": res[1], "nearest": res[2]}
    if shadow:
        out["visibility"] = res[3]
    if aux:
        out["normal"], out["pos"] = res[-2], res[-1]
    return out


def _source_leaves(scene: Dict[str, Any]) -> Dict[str, Any]:
    """The caller's own leaf objects under the keys flatten_scene files them under."""
    out: Dict[str, Any] = {}
    for kind, grp in scene["objects"].items():
        for name in _OBJ_FIELDS.get(kind, ()):
            if name in grp:
                out[f"{kind}.{name}"] = grp[name]
    out.update(_scene_leaves(scene))
    return out


class ResidentScene:
    """A scene flattened ONCE and rendered many times -- the shape of an optimisation loop
    (diffrend/torch/test_optimization.py: render, loss, backward, optimiser step, repeat).  ``render(scene)`` pays the
    scene conversion, validation and descriptor building on every call (about as long as the GPU work for a mesh of a
    few thousand triangles); here that happens in the constructor.  Leaves that are contiguous float32 tensors on the
    render device are used IN PLACE: an optimiser that updates them in place (torch.optim does) is seen by the next
    ``render()`` without any copy, and their ``.grad`` is filled by the analytic HIP backward.  ``nearest`` comes back
    as the kernel writes it (int32; ``render(scene)`` widens it to the reference's int64 with one more pass).

        rs = ResidentScene(scene, shading='torch')        # leaves with requires_grad=True stay attached
        for _ in range(steps):
            opt.zero_grad(); loss(rs.render()['image']).backward(); opt.step()

    ``aux=True`` (``shading='torch'`` only) adds the torch backend's ``normal`` and ``pos`` outputs to ``render()``,
    differentiable like ``image`` and ``depth``, and lets a ``capture_step`` loss use them.  It is off by default:
    writing them costs 24 bytes per pixel and frame.

    Camera: with ``shading='torch'``, ``eye`` / ``at`` / ``up`` of the camera dict that are tensors with
    ``requires_grad`` get their ``.grad`` too (``camera_leaves``).  While one of them requires grad, ``render()`` rebuilds
    the camera struct from the tensors' current values on every call, so an optimiser's in-place step is seen: that
    reads three small tensors on the host per call (a device tensor costs a synchronising copy each).  Otherwise the
    camera is read once, here and in ``set_camera``.  ``capture_step`` keeps freezing the camera at capture time and
    produces no camera gradient; ``fovy`` / ``focal_length`` have none.
    """

    def __init__(self, scene: Dict[str, Any], device="cuda", shading: str = "numpy", mode: str = "auto",
                 double_sided: bool = False, use_quartic: bool = False, validate: bool = True, aux: bool = False):
        if shading not in _lib.SHADING:
            raise ValueError(f"shading must be 'numpy' or 'torch', got {shading!r}")
        if aux and shading != "torch":
            raise ValueError("normal / pos outputs exist only in the torch backend's semantics: shading='torch'")
        self.device = torch.device(device)
        self.buf = flatten_scene(scene, self.device, validate=validate, keep_graph=True)
        self.shading, self.mode = shading, mode
        self._camera = scene["camera"]
        self.cam = camera_struct(scene["camera"], shading)
        if self.cam.ortho and shading != "torch":
            raise ValueError("orthographic projection exists only in the torch backend's semantics: shading='torch'")
        self.aux = bool(aux)
        self.shade = _Shade(shading, bool(double_sided), bool(use_quartic), False, self.aux)
        self.inputs = [self.buf.tensors[k] for k in _float_keys(self.buf, shading)]
        self.cam_leaves = camera_leaves(self._camera, shading)
        self.differentiable = any(t.requires_grad for t in self.inputs) or bool(self.cam_leaves)
        # "In place" has to be true for every leaf that is being optimised: a float64, CPU or non-contiguous leaf is
        # COPIED once by flatten_scene (the copy stays attached to autograd, so its gradients still reach the leaf and
        # the optimiser keeps stepping it) -- and every later render() would draw the first iteration's values.
        stale = []
        self.leaves: Dict[str, torch.Tensor] = {}           # the caller's own differentiable leaves, by flat key
        for key, leaf in _source_leaves(scene).items():
            if isinstance(leaf, torch.Tensor) and leaf.requires_grad and key in self.buf.tensors:
                self.leaves[key] = leaf
                t = self.buf.tensors[key]
                if t.data_ptr() != leaf.data_ptr() or t.dtype != leaf.dtype or t.device != leaf.device:
                    stale.append(f"{key} ({str(leaf.dtype).replace('torch.', '')} on {leaf.device}"
                                 f"{'' if leaf.is_contiguous() else ', not contiguous'})")
        if stale:
            raise ValueError("ResidentScene uses differentiable leaves in place, and these would be copied once and "
                             "then never refreshed: " + ", ".join(stale) + f".  Give contiguous float32 tensors on "
                             f"{self.device}, or call render(scene) per iteration (it converts on every call).")

    def set_camera(self, camera: Dict[str, Any]) -> None:
        self._camera = camera
        self.cam = camera_struct(camera, self.shading)
        self.cam_leaves = camera_leaves(camera, self.shading)
        self.differentiable = any(t.requires_grad for t in self.inputs) or bool(self.cam_leaves)

    def render(self, rows: Optional[Tuple[int, int]] = None) -> "RenderResult":
        if self.cam_leaves:
            self.cam = camera_struct(self._camera, self.shading)       # the leaves' current values
        image, depth, nearest, extra = _forward(self.buf, self.cam, rows, self.mode, self.shade, self.inputs,
                                                self.differentiable and torch.is_grad_enabled(),
                                                cam_leaves=self.cam_leaves)
        return RenderResult(self._camera, self.device, image=image, depth=depth, nearest=nearest, **extra)

    def capture_step(self, loss_fn, warmup: int = 3) -> "CapturedStep":
        """One optimisation step's GPU work -- render, ``loss_fn(result)``, backward -- captured as ONE hipGraph and
        replayed per iteration: the Python side of an iteration (autograd bookkeeping, descriptor structs, ~20 kernel
        launches) then costs one graph launch.  See ``CapturedStep``."""
        return CapturedStep(self, loss_fn, warmup)


class CapturedStep:
    """``step = rs.capture_step(loss_fn)``; then per iteration ``loss = step.replay(); optimiser.step()``.

    The whole-step capture recipe of torch.cuda.graphs: a few eager iterations on a side stream, then one iteration
    recorded into a graph -- the library's forward, ``loss_fn`` on the rendered image and depth (and normal and pos
    with ``ResidentScene(aux=True)``), torch's own backward of the loss down to those outputs, and the library's
    backward from there to the leaves, called directly.  (Letting
    the autograd engine run the renderer's autograd.Function inside a capture ends in a segmentation fault in
    hipStreamEndCapture on ROCm 7.2 -- profiles/r03_capture_diag.txt; each of the pieces used here captures fine.)  The
    leaves' ``.grad`` tensors are static: every replay overwrites them (they do not accumulate), ``loss`` and
    ``result`` are static tensors too.
    What a replay reads is device memory only -- the leaves (an optimiser's in-place step is seen by the next replay)
    and whatever tensors ``loss_fn`` closes over (update a target with ``copy_``) -- while the camera and everything
    else on the host was frozen at capture time.  The step holds one frame's scratch of its own (``workspace``), so
    eager ``rs.render()`` calls between replays, at any frame size, leave the replays alone."""

    def __init__(self, rs: ResidentScene, loss_fn, warmup: int = 3):
        if not any(t.requires_grad for t in rs.inputs):
            raise ValueError("capture_step needs at least one scene leaf that requires grad (the camera is frozen at "
                             "capture time and gets no gradient from a captured step)")
        self.rs = rs
        keys = _float_keys(rs.buf, rs.shading)
        # the CALLER's leaves (rs.inputs are reshaped views of them: autograd reaches the leaves through the views, a
        # hand-made .grad has to be put on the leaves themselves)
        self.keys = [k for k in keys if k in rs.leaves]
        self.leaves = [rs.leaves[k] for k in self.keys]
        self.workspace = rs.buf.new_workspace(*frame_size(rs.cam))
        current = torch.cuda.current_stream(rs.device)
        side = torch.cuda.Stream(rs.device)
        side.wait_stream(current)
        cam_leaves, rs.cam_leaves = rs.cam_leaves, {}   # the camera is frozen: its leaves take no part, warm-up included
        with torch.cuda.stream(side):
            for _ in range(max(1, int(warmup))):        # module load, allocator
                for t in self.leaves:
                    t.grad = None
                loss_fn(rs.render()).backward()
            rs.cam_leaves = cam_leaves
            # one frame in the step's own scratch clears its bin counters and leaves them clean: the graph then holds no
            # clearing launch
            _frame(rs.buf, rs.cam, None, rs.mode, rs.shade, workspace=self.workspace)
        current.wait_stream(side)
        torch.cuda.synchronize(rs.device)
        for t in self.leaves:
            t.grad = None
        self.graph = torch.cuda.CUDAGraph()
        need = [k in rs.leaves for k in keys]
        with torch.cuda.graph(self.graph):
            with torch.no_grad():
                image, depth, nearest, aux, _ = _frame(rs.buf, rs.cam, None, rs.mode, rs.shade, workspace=self.workspace)
            outs = [image.requires_grad_(), depth.requires_grad_()]
            extra = {}
            if aux is not None:
                outs += [aux[0].requires_grad_(), aux[1].requires_grad_()]
                extra = {"normal": outs[2], "pos": outs[3]}
            self.result = RenderResult(rs._camera, rs.device, image=outs[0], depth=outs[1], nearest=nearest, **extra)
            self.loss = loss_fn(self.result)
            g = list(torch.autograd.grad(self.loss, outs, allow_unused=True)) + [None, None]
            got = _render_backward(rs.buf, rs.cam, None, rs.mode, rs.shade, depth, nearest, None, g[0], g[1], need,
                                   g[2], g[3], workspace=self.workspace)
        # the static gradient tensors every replay writes, in the order of self.leaves and in the leaves' own shapes
        self.grads = [(got[k] if k in got else torch.zeros_like(rs.buf.tensors[k])).view(leaf.shape)
                      for k, leaf in zip(self.keys, self.leaves)]
        for t, g in zip(self.leaves, self.grads):
            t.grad = g

    def replay(self) -> torch.Tensor:
        self.graph.replay()
        for t, g in zip(self.leaves, self.grads):          # whatever happened to .grad in between (zero_grad(set_to_none))
            t.grad = g
        return self.loss


def _aux_buffers(cam: _lib.SrhCamera, rows, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (rows, W, 3) float32 ``normal`` and ``pos`` outputs of a torch-shading frame (or slab)."""
    width, height = frame_size(cam)
    r0, r1 = _rows(rows, height)
    h = r1 - r0
    return (torch.empty((h, width, 3), dtype=torch.float32, device=device),
            torch.empty((h, width, 3), dtype=torch.float32, device=device))


def _norm_depth_image(depth: torch.Tensor, far: float) -> torch.Tensor:
    """`norm_depth_image_only` of the torch backend (torch/renderer.py:245-249), on the far + 1 background depth:
    background pixels take the minimum depth, then (d - min) / (max - min) -- the same tensor expression, so it is
    differentiable through `depth` like the reference's.  The reference's own path raises before it gets here
    (oracle/check_ref_kwargs.py), so this output is restated from the source, not pinned by a reference fixture."""
    min_depth = depth.min()
    image = torch.where(depth >= far, min_depth, depth)
    return (image - min_depth) / (depth.max() - min_depth)


class RenderResult(dict):
    """The reference's result dict.  ``image`` (H,W,3), ``depth`` (H,W) and ``nearest`` (H,W) are always
    present; ``ray_dir`` (4,N) is produced on first access.  The three O(M*N) entries of the numpy
    backend (``ray_dist``, ``obj_dist``, ``valid_pixels``) do not exist in a streaming renderer."""

    def __init__(self, camera, device, *args, **kw):
        super().__init__(*args, **kw)
        self._camera, self._device = camera, device

    def numpy(self, *keys: str) -> Dict[str, np.ndarray]:
        """Host ndarrays of the named entries (default image, depth, nearest) -- what the reference's numpy backend
        returns.  The copies go through pinned host memory from torch's caching host allocator, asynchronously and
        with one wait at the end: ~10x the rate of ``.cpu()`` on a 2048 x 2048 frame.  The arrays own their memory."""
        keys = keys or ("image", "depth", "nearest")
        stream = torch.cuda.current_stream(self._device)
        host = {}
        for k in keys:
            t = self[k].detach()
            host[k] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            host[k].copy_(t, non_blocking=True)
        stream.synchronize()
        return {k: h.numpy() for k, h in host.items()}

    def __missing__(self, key):
        if key == "ray_dir":
            val = generate_rays(self._camera, self._device)
            self[key] = val
            return val
        if key in ("ray_dist", "obj_dist", "valid_pixels"):
            raise KeyError(f"{key!r}: the hip backend never materialises (primitives x pixels) arrays")
        raise KeyError(key)


def render(scene: Dict[str, Any], **params) -> RenderResult:
    """Drop-in for the reference backends' ``render(scene)``.

    Returns torch tensors on the render device: ``image`` (H,W,3) float32, ``depth`` (H,W) float32 with
    +inf where nothing is hit, ``nearest`` (H,W) int64 (0 where nothing is hit), matching
    ``diffrend.numpy.renderer.render`` within fp32 rounding of the stored outputs.

    Keyword arguments: ``device`` ('cuda'), ``mode`` ('auto' | 'exact' | 'fast' | 'binned'), ``rows`` ((r0, r1) slab),
    ``waves_per_tile`` (0 | 1 | 4: launch shape of the binned kernel, a tuning knob with identical results),
    ``validate`` (host-side index / w checks), ``shading`` ('numpy' | 'torch').  With ``shading='torch'`` the call
    follows ``diffrend.torch.renderer.render`` instead (Phong shading with lights.attenuation / lights.ambient /
    materials.coeffs, ``double_sided``, ``use_quartic``, orthonormal camera basis, far+1 background, extra outputs
    ``normal`` and ``pos`` -- differentiable like ``image`` and ``depth`` when a leaf requires grad (see
    ``_RenderFunction``; their upstream gradients at pixels that hit nothing are ignored, as image's and depth's are);
    ``shadow=True`` adds the all-pairs shadow-ray pass and a ``light_visibility`` bit field;
    ``camera.proj_type = 'ortho'``; ``norm_depth_image_only=True`` returns the normalised depth as ``image``).  The
    torch backend's remaining kwargs are accepted where they change no output of the reference (``tiled``,
    ``tile_size``, ``backface_culling`` -- see ``_TORCH_ONLY_KWARGS``); ``vis_stat=True`` raises as it does there.

    Camera gradients (``shading='torch'``): ``camera['eye'|'at'|'up']`` given as tensors with ``requires_grad`` receive
    ``.grad`` like the scene's leaves (in their own shape, dtype and device; w gets 0), also when nothing else requires
    grad -- autograd through the reference's ray generation, misses contributing nothing.  ``fovy`` and ``focal_length``
    get no gradient, and ``shading='numpy'`` keeps detaching the camera (see ``camera_leaves``).
    """
    unknown = set(params) - _TORCH_ONLY_KWARGS - {"device", "mode", "rows", "validate", "shading", "double_sided",
                                                  "use_quartic", "waves_per_tile"}
    if unknown:
        raise TypeError(f"render() got unexpected keyword arguments {sorted(unknown)}")
    device = torch.device(params.get("device", "cuda"))
    buf = flatten_scene(scene, device, validate=params.get("validate", True), keep_graph=torch.is_grad_enabled())
    shading = params.get("shading", "numpy")
    cam = camera_struct(scene["camera"], shading)
    rows, mode = params.get("rows"), params.get("mode", "auto")
    if shading not in _lib.SHADING:
        raise ValueError(f"shading must be 'numpy' or 'torch', got {shading!r}")
    shadow = bool(params.get("shadow", False))
    if shadow and shading != "torch":
        raise ValueError("shadow rays exist only in the torch backend's semantics: shading='torch'")
    if params.get("vis_stat", False):
        raise RuntimeError("Removed Support for vis_stat")          # torch/renderer.py:235, same message
    norm_depth = bool(params.get("norm_depth_image_only", False))
    if norm_depth and shading != "torch":
        raise ValueError("norm_depth_image_only exists only in the torch backend's semantics: shading='torch'")
    if cam.ortho and shading != "torch":
        raise ValueError("orthographic projection exists only in the torch backend's semantics: shading='torch'")
    inputs = [buf.tensors[k] for k in _float_keys(buf, shading)]
    cam_leaves = camera_leaves(scene["camera"], shading) if torch.is_grad_enabled() else {}
    differentiable = torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or bool(cam_leaves))
    tch = shading == "torch"                    # the torch backend's semantics
    # norm_depth_image_only returns before the fragment stage (torch/renderer.py:245-260): no normal / pos, and outside
    # autograd no shadow pass
    shade = _Shade(shading, tch and bool(params.get("double_sided", False)), tch and bool(params.get("use_quartic", False)),
                   shadow and (differentiable or not norm_depth), tch and not norm_depth)
    image, depth, nearest, extra = _forward(buf, cam, rows, mode, shade, inputs, differentiable,
                                            params.get("waves_per_tile", 0), cam_leaves)
    if norm_depth:
        image = _norm_depth_image(depth, cam.far_clip)
    return RenderResult(scene["camera"], device, image=image, depth=depth, nearest=nearest.to(torch.int64), **extra)
