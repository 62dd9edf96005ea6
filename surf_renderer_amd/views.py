"""Many views per call: per-view scenes (``ViewScenes``), the library's batched forward and backward over caller-provided
stacked buffers (``render_views_buffers``, ``render_views_bwd_buffers``) and ``render_views`` with its autograd function."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .buffers import (SceneBuffers, _SCENE_LEAVES, _as_tensor, _float_keys, _ptr, _scratch, _source_leaves, _stream_ptr,
                      camera_leaves, camera_struct, flatten_scene, frame_size)
from .frame import (_OUTPUTS, _Shade, _bind_grad, _layout_key, _like, _outputs, _params, _rows, _upstream, _ws_note, _ws_state,
                    render_buffers, shadow_pass)


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

    def refs(self, buf: SceneBuffers, first_view: int, n: int):
        """What a library call over the ``n`` views from ``first_view`` takes as its scene: references to the objects,
        lights and materials -- this object's arrays from ``first_view`` on where a view overrides something of theirs,
        else the base scene's -- and the SrhParams.per_view mask that says which are arrays."""
        if first_view < 0 or first_view + n > self.n:
            raise ValueError(f"{self.n} per-view scenes for {n} cameras from view {first_view}")
        return (C.byref(self.objects[first_view] if self.mask & _lib.VIEWS_OBJECTS else buf.objects),
                C.byref(self.lights[first_view] if self.mask & _lib.VIEWS_LIGHTS else buf.lights),
                C.byref(self.materials[first_view] if self.mask & _lib.VIEWS_MATERIALS else buf.materials), self.mask)

    def view(self, buf: SceneBuffers, v: int) -> SceneBuffers:
        """The scene of view v as resident buffers of its own (for the per-view passes: shadows)."""
        import copy
        one = copy.copy(buf)
        one.objects, one.lights, one.materials = self.objects[v], self.lights[v], self.materials[v]
        return one


def _scene_refs(buf: SceneBuffers, scenes: Optional[ViewScenes], first_view: int, n: int):
    """``ViewScenes.refs`` for a call that may have no per-view scenes: then the base scene's references and mask 0."""
    if scenes is None:
        return C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials), 0
    return scenes.refs(buf, first_view, n)


def render_views_buffers(buf: SceneBuffers, cams: Sequence[_lib.SrhCamera], images: torch.Tensor, depths: torch.Tensor,
                         nearests: Optional[torch.Tensor] = None, rows: Optional[Tuple[int, int]] = None,
                         workspace: Optional[torch.Tensor] = None, image_row_stride: int = 0,
                         depth_row_stride: int = 0, view_row0: Optional[Sequence[int]] = None,
                         scenes: Optional[ViewScenes] = None, mode: str = "auto", first_view: int = 0,
                         aux: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
                         shading: str = "numpy", double_sided: bool = False, use_quartic: bool = False,
                         waves_per_tile: int = 0) -> torch.Tensor:
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
    params = _params(buf, _rows(rows, height), mode, _Shade(shading, double_sided, use_quartic),
                     waves_per_tile=int(waves_per_tile), image_row_stride=int(image_row_stride),
                     depth_row_stride=int(depth_row_stride))
    row0_arr = None
    if view_row0 is not None:
        if len(view_row0) != n:
            raise ValueError("view_row0 needs one entry per view")
        row0_arr = (C.c_int32 * n)(*[int(r) for r in view_row0])
        params.view_row0 = C.cast(row0_arr, C.c_void_p)
    workspace = _scratch(lib.srh_workspace_bytes_views(C.byref(buf.objects), width, height, n), workspace, buf.device)
    arr = (_lib.SrhCamera * n)(*cams)
    binned = not cams[0].ortho
    key = _layout_key(buf, width, height, ("views", n))
    if binned:
        params.counters_clean = int(_ws_state(workspace) == ("clean", key))
        _ws_note(workspace, None)
    ob, ls, ms, params.per_view = _scene_refs(buf, scenes, first_view, n)
    if aux is not None:
        for t in aux:
            if t is not None and (tuple(t.shape) != (n, params.row1 - params.row0, width, 3) or t.dtype != torch.float32
                                  or not t.is_contiguous() or t.device != buf.device):
                raise ValueError(f"aux buffer mismatch: want contiguous float32 {(n, params.row1 - params.row0, width, 3)} "
                                 f"on {buf.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    with torch.cuda.device(buf.device):
        args = (n, arr, ob, ls, ms, C.byref(params), workspace.data_ptr(), workspace.numel(), images.data_ptr(),
                depths.data_ptr(), _ptr(nearests))
        if aux is None:
            _lib.check(lib.srh_render_views(*args, _stream_ptr(buf.device)))
        else:
            _lib.check(lib.srh_render_views_aux(*args, _ptr(aux[0]), _ptr(aux[1]), _stream_ptr(buf.device)))
    if binned:
        _ws_note(workspace, ("clean", key))
    return workspace


def render_views_bwd_buffers(buf: SceneBuffers, cams: Sequence[_lib.SrhCamera], g_images: Optional[torch.Tensor],
                             g_depths: Optional[torch.Tensor], nearests: torch.Tensor, depths: torch.Tensor, grads,
                             workspace: Optional[torch.Tensor] = None, scenes: Optional[ViewScenes] = None,
                             first_view: int = 0, visibility: Optional[torch.Tensor] = None,
                             g_normals: Optional[torch.Tensor] = None, g_poses: Optional[torch.Tensor] = None,
                             camera_grads=None, camera_scratch: Optional[torch.Tensor] = None, shading: str = "numpy",
                             double_sided: bool = False, use_quartic: bool = False) -> torch.Tensor:
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
    params = _params(buf, (0, height), "auto", _Shade(shading, double_sided, use_quartic), visibility=_ptr(visibility))
    workspace = _scratch(lib.srh_workspace_bytes_views(C.byref(buf.objects), width, height, n), workspace, buf.device)
    state = _ws_state(workspace)
    if state is not None and state[1] != _layout_key(buf, width, height, ("views", n)):
        _ws_note(workspace, None)                           # another batch size's layout: its counters may lie under records
    arr = (_lib.SrhCamera * n)(*cams)
    ob, ls, ms, params.per_view = _scene_refs(buf, scenes, first_view, n)
    with torch.cuda.device(buf.device):
        if g_normals is None and g_poses is None and camera_grads is None and camera_scratch is None:
            _lib.check(lib.srh_render_views_bwd(n, arr, ob, ls, ms, C.byref(params), workspace.data_ptr(),
                                                workspace.numel(), g_images.data_ptr(), _ptr(g_depths),
                                                nearests.data_ptr(), depths.data_ptr(), grads, _stream_ptr(buf.device)))
        else:
            if camera_grads is not None and camera_scratch is None:
                camera_scratch = buf.ensure_camera_scratch_views(width, height, n)
            _lib.check(lib.srh_render_views_bwd_camera(
                n, arr, ob, ls, ms, C.byref(params), workspace.data_ptr(), workspace.numel(), _ptr(g_images), _ptr(g_depths),
                _ptr(g_normals), _ptr(g_poses), nearests.data_ptr(), depths.data_ptr(), grads, camera_grads,
                _ptr(camera_scratch), camera_scratch.numel() * camera_scratch.element_size() if camera_scratch is not None else 0,
                _stream_ptr(buf.device)))
    return workspace


class _ViewsCall(NamedTuple):
    """What one ``render_views`` call renders: the resident scene, the camera structs, the per-view scenes (or None) and
    the call's options (``shade.shadow``: the shadow pass runs on every view; ``shade.aux``: normal and pos are written)."""
    buf: SceneBuffers
    cams: List[_lib.SrhCamera]
    every: Optional[ViewScenes]
    mode: str
    streams: int
    want_nearest: bool
    batch: int
    shade: _Shade
    waves_per_tile: int = 0


def _views_forward(call: _ViewsCall) -> Tuple[Dict[str, torch.Tensor], Optional[torch.Tensor]]:
    """The forward of ``render_views``: the result dict and the workspace of the batched path (None round-robin)."""
    buf, cams, every, mode, shade = call.buf, call.cams, call.every, call.mode, call.shade
    device, want_nearest = buf.device, call.want_nearest
    width, height = frame_size(cams[0])
    n = len(cams)
    names = ("image", "depth") + ("nearest",) * bool(want_nearest) + ("normal", "pos") * bool(shade.aux)
    out = dict(zip(names, _outputs(device, (n, height, width), *names)))
    image, depth, nearest, normal, pos = (out.get(k) for k in _OUTPUTS)
    model = dict(shading=shade.shading, double_sided=shade.double_sided, use_quartic=shade.use_quartic,
                 waves_per_tile=call.waves_per_tile)

    def scene_of(v: int) -> SceneBuffers:
        return every.view(buf, v) if every is not None else buf

    def shadows(first: int, count: int) -> None:
        if not shade.shadow:
            return
        if "visibility" not in out:
            out["visibility"] = torch.empty((n, height, width), dtype=torch.int64, device=device)
        buf.ensure_shadow_workspace(width, height)          # the per-view copies below share it
        for v in range(first, first + count):
            out["visibility"][v] = shadow_pass(scene_of(v), cams[v], None, image[v], depth[v], nearest[v],
                                               double_sided=bool(shade.double_sided), use_quartic=bool(shade.use_quartic))

    if mode in ("auto", "binned") and int(call.batch) > 0:
        step = max(1, min(int(call.batch), n))
        workspace = None                                    # sized by the first (largest) batch, reused by the others
        for i in range(0, n, step):
            m = min(step, n - i)
            workspace = render_views_buffers(buf, cams[i:i + m], image[i:i + m], depth[i:i + m],
                                             nearest[i:i + m] if want_nearest else None, workspace=workspace,
                                             scenes=every, mode=mode, first_view=i,
                                             aux=(normal[i:i + m], pos[i:i + m]) if shade.aux else None, **model)
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
                           workspace=scratch[k], aux=(normal[v], pos[v]) if shade.aux else None, **model)
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
    device, w = 0).  The outputs are image, depth, nearest, then ``visibility`` with ``call.shade.shadow``, then ``normal`` and
    ``pos`` with ``call.shade.aux``.  The backward is srh_render_views_bwd; with an upstream gradient of normal / pos, or a
    camera leaf that needs its gradient, it is srh_render_views_bwd_camera."""

    @staticmethod
    def forward(ctx, call: _ViewsCall, slots, cam_slots, *inputs):
        if call.shade.aux:
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
        if call.shade.aux:
            res += (out["normal"], out["pos"])
        return res

    @staticmethod
    def backward(ctx, g_image, g_depth, _g_nearest, *g_rest):
        depth, nearest, vis = ctx.saved_tensors
        call, slots, cam_slots = ctx.call, ctx.slots, ctx.cam_slots
        buf, cams, every, shade = call.buf, call.cams, call.every, call.shade
        keys = _float_keys(buf, shade.shading)
        need = ctx.needs_input_grad[3:]
        n = len(cams)
        g_normal, g_pos = g_rest[-2:] if shade.aux else (None, None)
        cam_rows = {slot: i for i, (slot, want) in enumerate(zip(cam_slots, need[len(keys) + len(slots):])) if want}
        extended = g_normal is not None or g_pos is not None or bool(cam_rows)      # srh_render_views_bwd_camera
        g_image, g_depth, g_normal, g_pos = _upstream(g_image, g_depth, g_normal, g_pos, bool(cam_rows),
                                                      tuple(depth.shape) + (3,), buf.device)
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
                if g is not None:
                    _bind_grad(sg[v], buf, key, g)
        # the wanted camera gradients: a row of four floats each, written (not added to) by the finish kernel
        cg = cam_out = None
        if cam_rows:
            cam_out = torch.zeros((len(cam_rows), 4), dtype=torch.float32, device=buf.device)
            cg = (_lib.SrhCameraGrads * n)()
            for (v, k), i in cam_rows.items():
                setattr(cg[v], k, cam_out[i].data_ptr())
        step = min(int(call.batch) if int(call.batch) > 0 else 256, 256, n)
        workspace = ctx.workspace
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
                                                 visibility=vis[i:i + m] if vis is not None else None,
                                                 shading=shade.shading, double_sided=shade.double_sided,
                                                 use_quartic=shade.use_quartic, **more)
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
            cam_grads.append(_like(src[i], shape, dtype, device))
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
    shadow = bool(shading_kw.get("shadow", False))
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
    shade = _Shade(shading, shading_kw.get("double_sided", False), shading_kw.get("use_quartic", False), shadow, bool(aux))
    call = _ViewsCall(buf, cams, every, mode, streams, want_nearest or shadow or differentiable, batch, shade,
                      shading_kw.get("waves_per_tile", 0))
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
