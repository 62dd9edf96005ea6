"""Resident scenes: an expanded scene dict as device arrays in the layouts of include/srh.h (``flatten_scene`` ->
``SceneBuffers``), the table of the scene's leaves (``_SCENE_LEAVES``, ``_float_keys``), the camera struct and its
differentiable leaves, and the scratch buffers the library asks for.  The bottom layer of the Python host side:
frame.py, views.py and renderer.py build on it, and it imports none of them."""
from __future__ import annotations

import ctypes as C
import threading
from dataclasses import dataclass
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .scene import PRIM_CODE, _OBJ_FIELDS, unit_up


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


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """The device address of ``t``; None (NULL for the library) for None."""
    return t.data_ptr() if t is not None else None


def _scratch(need: int, have: Optional[torch.Tensor], device: torch.device, dtype: torch.dtype = torch.uint8) -> torch.Tensor:
    """A buffer of at least ``need`` bytes, ``need`` being what one of the library's size queries answered: ``have`` if
    it is large enough, else a new one of ``dtype``.  A query answers 0 when it refuses its arguments: that raises with
    the library's message."""
    if need == 0:
        raise _lib.SrhError(-1, _lib.load().srh_last_error().decode())
    if have is None or have.numel() * have.element_size() < need:
        have = torch.empty(-(-need // dtype.itemsize), dtype=dtype, device=device)
    return have


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
            w, h = max(width, self.workspace_frame[0]), max(height, self.workspace_frame[1])
            self.workspace = self.new_workspace(w, h)
            self.workspace_frame = (w, h)
        return self.workspace

    def ensure_shadow_workspace(self, width: int, height: int) -> torch.Tensor:
        """Scratch of the accelerated shadow pass: room for the light views (tile bins in every light's screen space)
        behind the primary frame's scratch."""
        need = _lib.load().srh_shadow_workspace_bytes(C.byref(self.objects), width, height, self.lights.n_lights)
        self.shadow_workspace = _scratch(need, self.shadow_workspace, self.device)
        return self.shadow_workspace

    def ensure_camera_scratch(self, width: int, rows: int) -> torch.Tensor:
        """Scratch of srh_render_bwd_camera for a backward over ``width x rows`` pixels.  Its contents never matter: every
        workgroup of a backward launch overwrites its own slot."""
        need = _lib.load().srh_camera_grad_scratch_bytes(width, rows)
        self.camera_scratch = _scratch(need, self.camera_scratch, self.device, torch.float64)
        return self.camera_scratch

    def ensure_camera_scratch_views(self, width: int, rows: int, n_views: int) -> torch.Tensor:
        """Scratch of srh_render_views_bwd_camera for a backward over ``n_views`` views of ``width x rows`` pixels: the
        views' finish descriptors and a slice of partial sums per view.  Its contents never matter either."""
        need = _lib.load().srh_camera_grad_scratch_bytes_views(width, rows, n_views)
        self.camera_scratch_views = _scratch(need, self.camera_scratch_views, self.device, torch.float64)
        return self.camera_scratch_views

    def new_workspace(self, width: int, height: int) -> torch.Tensor:
        """An additional scratch buffer (one per frame in flight when frames are pipelined over several streams)."""
        return _scratch(_lib.load().srh_workspace_bytes(C.byref(self.objects), width, height), None, self.device)

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


def _float_keys(buf: SceneBuffers, shading: str = "numpy") -> List[str]:
    """Keys of buf.tensors that are differentiable inputs, in a fixed order (the torch shading model adds its own
    inputs where the scene has them)."""
    keys = [f"{kind}.{name}" for kind in buf.kinds for name in _OBJ_FIELDS[kind]]
    return keys + [k for k, leaf in _SCENE_LEAVES.items()
                   if leaf.grad and k in buf.tensors and (shading == "torch" or not leaf.torch_only)]


def _source_leaves(scene: Dict[str, Any]) -> Dict[str, Any]:
    """The caller's own leaf objects under the keys flatten_scene files them under."""
    out: Dict[str, Any] = {}
    for kind, grp in scene["objects"].items():
        for name in _OBJ_FIELDS.get(kind, ()):
            if name in grp:
                out[f"{kind}.{name}"] = grp[name]
    out.update(_scene_leaves(scene))
    return out
