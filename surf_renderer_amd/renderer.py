"""The hip backend's mirror of the reference backend interface: ``render(scene, **params) -> dict``.

Same call and same scene dict as ``diffrend.numpy.renderer.render`` (numpy/renderer.py:204-272) and
``diffrend.torch.renderer.render`` (torch/renderer.py:136-355); the work is done by hand-written
gfx950 kernels behind the C ABI of include/srh.h.  PyTorch is used for device memory and streams only.

Layers, one module each, every module importing only from those above it
  buffers.py    flatten_scene(): expanded scene dict (lists / ndarrays / tensors) -> SceneBuffers: contiguous fp32 /
                int32 device arrays in the reference's layouts and concatenation order, plus the ctypes descriptors
                libsrh consumes.  Done once per scene; stays resident in HBM.  camera_struct(), the table of the
                scene's differentiable leaves, the scratch buffers.
  frame.py      render_buffers(): one frame from resident buffers and a camera (what bench.py times); the shadow pass;
                the differentiable frame (_RenderFunction over srh_render_bwd*).
  views.py      render_views(): many views per call, batched forward and backward, per-view scenes (ViewScenes).
  renderer.py   render(): the drop-in: flatten + render_buffers + reference-shaped result dict; ResidentScene and
                CapturedStep for optimisation loops.  Every name of the layers below that is used from outside them is
                importable from here.

There is no CPU fallback: without a GPU or without libsrh.so these functions raise.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
# the second group of each list is not used in this file: other modules, the tools and the tests reach it as renderer.<name>
from .buffers import (_float_keys, _source_leaves, camera_leaves, camera_struct, flatten_scene, frame_size,
                      SceneBuffers)  # noqa: F401
from .frame import (_Shade, _forward, _frame, _render_backward, generate_rays,
                    _RenderFunction, _layout_key, _ws_note, _ws_state, bin_statistics, render_buffers,
                    shadow_pass)  # noqa: F401
from .views import ViewScenes, render_views, render_views_buffers, render_views_bwd_buffers  # noqa: F401

# keyword arguments of the torch backend's render() that callers pass routinely (torch/renderer.py:152-168, 233-245,
# 291, 326-327); the hip backend accepts them so call sites need no edits.  What each does here:
#   tiled, tile_size        memory knobs of the reference's (pixels x primitives) arrays: no effect on any output
#   backface_culling        the reference only LABELS primitives (torch/utils.py:515-536) and never reads the labels:
#                           every output is unchanged (oracle/check_ref_kwargs.py ran the reference both ways)
#   vis_stat                True raises in the reference ('Removed Support for vis_stat', :235) and here
#   norm_depth_image_only   `image` becomes the normalised depth of :245-249 (see render())
#   shadow                  shadow rays (:291-314)
_TORCH_ONLY_KWARGS = {"tiled", "tile_size", "backface_culling", "norm_depth_image_only", "vis_stat", "shadow"}


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
