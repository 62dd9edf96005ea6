"""One frame from resident buffers: ``render_buffers`` (what bench.py times) with the workspace-state notes, the binning
statistics, ray generation and the shadow pass, and the differentiable frame -- ``_frame``, ``_RenderFunction`` and the
library's backward (``_render_backward``) with the helpers the batched backward of views.py shares."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .buffers import (SceneBuffers, _SCENE_LEAVES, _float_keys, _ptr, _require_gpu, _stream_ptr, camera_struct,
                      frame_size)


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


_OUTPUTS = {"image": (torch.float32, (3,)), "depth": (torch.float32, ()), "nearest": (torch.int32, ()),
            "normal": (torch.float32, (3,)), "pos": (torch.float32, (3,))}


def _outputs(device: torch.device, shape: Tuple[int, ...], *names: Optional[str]):
    """The named outputs of a frame or slab (``shape`` = (h, W)) or of n stacked ones ((n, h, W)), uninitialised and in
    the order asked for: ``image``, ``normal`` and ``pos`` are shape + (3,) f32, ``depth`` shape f32, ``nearest`` shape
    i32.  A name given as None yields None (an output the caller does not want)."""
    return tuple(None if k is None else torch.empty(tuple(shape) + _OUTPUTS[k][1], dtype=_OUTPUTS[k][0], device=device)
                 for k in names)


def _aux_buffers(cam: _lib.SrhCamera, rows, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (rows, W, 3) float32 ``normal`` and ``pos`` outputs of a torch-shading frame (or slab)."""
    width, height = frame_size(cam)
    r0, r1 = _rows(rows, height)
    return _outputs(device, (r1 - r0, width), "normal", "pos")


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
        # an empty slab still reaches the library, which refuses it with its own message
        image, depth, nearest = _outputs(buf.device, (max(h, 0), width), "image", "depth", "nearest" if want_nearest else None)
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
    image, depth = _outputs(buf.device, (r1 - r0, width), "image", "depth")
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
            cam_grads.append(None if g is None else _like(g, shape, dtype, device))
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


def _bind_grad(sg: _lib.SrhGrads, buf: SceneBuffers, key: str, g: torch.Tensor) -> None:
    """Point ``sg`` at ``g`` as the gradient buffer of the input ``key`` (of ``_float_keys``): a scene leaf has a field
    of its own, an object field one slot per segment.  ``disk.radius`` is bound nowhere: its gradient is identically
    zero (numpy/renderer.py:88: the radius only feeds a mask)."""
    if key in _SCENE_LEAVES:
        setattr(sg, _SCENE_LEAVES[key].grad, g.data_ptr())
    elif key != "disk.radius":
        kind, name = key.split(".")
        getattr(sg, name)[buf.kinds.index(kind)] = g.data_ptr()


def _upstream(g_image, g_depth, g_normal, g_pos, camera: bool, zero_shape: Sequence[int], device: torch.device):
    """The upstream gradients of image, depth, normal and pos as the library takes them: dense float32, or None.  A
    missing ``g_image`` becomes zeros of ``zero_shape`` -- the image-and-depth kernels need one -- unless the call goes
    to a kernel that accepts NULL for it (the geometry-only one): an upstream gradient of normal or pos is given, or
    ``camera`` gradients are wanted and one of depth is given."""
    if g_image is None and not (g_normal is not None or g_pos is not None or (camera and g_depth is not None)):
        g_image = torch.zeros(tuple(zero_shape), dtype=torch.float32, device=device)
    return tuple(g.to(torch.float32).contiguous() if g is not None else None for g in (g_image, g_depth, g_normal, g_pos))


def _like(g: torch.Tensor, shape, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """The (4,) camera gradient ``g`` in its leaf's own shape (a 3-vector takes the first 3 values), dtype and device."""
    return g[:int(np.prod(shape))].to(device=device, dtype=dtype).reshape(shape)


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
        if want:
            grads[key] = torch.zeros_like(buf.tensors[key])
            _bind_grad(sg, buf, key, grads[key])
    aux = g_normal is not None or g_pos is not None
    if camera and shade.shading != "torch":
        raise ValueError("camera gradients exist only in the torch backend's semantics: shading='torch'")
    g_image, g_depth, g_normal, g_pos = _upstream(g_image, g_depth, g_normal, g_pos, bool(camera), (r1 - r0, width, 3),
                                                  buf.device)
    params = _params(buf, (r0, r1), mode, shade, visibility=_ptr(vis))
    if workspace is None:
        workspace = buf.ensure_workspace(width, height)
    head = (C.byref(cam), C.byref(buf.objects), C.byref(buf.lights), C.byref(buf.materials), C.byref(params),
            workspace.data_ptr(), workspace.numel())
    upstream = (_ptr(g_image), _ptr(g_depth), _ptr(g_normal), _ptr(g_pos))
    tail = (nearest.data_ptr(), depth.data_ptr(), C.byref(sg))
    with torch.cuda.device(buf.device):
        if camera:
            cg = _lib.SrhCameraGrads()
            for k in camera:
                grads["camera." + k] = torch.empty(4, dtype=torch.float32, device=buf.device)
                setattr(cg, k, grads["camera." + k].data_ptr())
            scratch = buf.ensure_camera_scratch(width, r1 - r0)
            rc = lib.srh_render_bwd_camera(*head, *upstream, *tail, C.byref(cg), scratch.data_ptr(), scratch.numel() * 8,
                                           _stream_ptr(buf.device))
        elif aux:
            rc = lib.srh_render_bwd_aux(*head, *upstream, *tail, _stream_ptr(buf.device))
        else:
            rc = lib.srh_render_bwd(*head, *upstream[:2], *tail, _stream_ptr(buf.device))
    _lib.check(rc)
    return grads
