"""The reference's NDC splat renderer on the GPU: ``render_splats_NDC(scene, **params)`` as in
diffrend/torch/renderer.py:358-474 (the renderer behind optimize_NDC_test), and a batched form for its per-view loop.

    from surf_renderer_amd import render_splats_NDC, render_splats_NDC_batch
    res = render_splats_NDC(scene, double_sided=False, use_quartic=False)
    res = render_splats_NDC_batch(scene)   # objects.disk.pos [B, N, 3|4]; normal, camera.eye and lights.pos
                                            # optionally with a leading B as well

Forward and backward are HIP kernels (srh_splat_ndc_fwd / srh_splat_ndc_bwd, surf_renderer_amd/csrc/srh_splat_ndc.h):
a batch is one forward launch and one backward launch.  Differentiable inputs: objects.disk.pos (every column),
objects.disk.normal, lights.pos, colors, lights.attenuation, lights.ambient, materials.albedo, materials.coeffs.

With ``camera_grad=True`` camera['eye'], ['at'] and ['up'] may require grad and receive it through the lights' camera
coordinates, exactly as in render_splats_along_ray (splats.py has the text): srh_splat_ndc_bwd_view sums d loss / d (the
view's world-to-camera matrix) in fp64 without atomics, the chain to the leaves is the reference's lookat on the host.
norm_depth_image_only=True leaves their .grad None (nothing launched), a shaded frame whose loss does not use `image`
gives exact zeros (nothing launched for the camera either).  Without the keyword a camera tensor that requires grad is
refused; fovy, near, far and the viewport are refused either way.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Tuple

import numpy as np
import torch

from . import _lib
from ._camera import camera_entries, check_camera_grad
from ._layer import fill_grads, gpu_device, ptr, stream, view_grad_buffers
from .splats import _f32, _i32, _shape, _value, camera_matrices

_NAME = "render_splats_NDC"
_DIFF = ("pos", "normal", "lights_pos", "colors", "attenuation", "ambient", "albedo", "coeffs")


class _SplatNdc:
    """Everything of one call that is not differentiated: the launch parameters, eye, indices, strides."""

    def __init__(self, params, device, eye, color_idx, material_idx, batched_flags, n_lights, n_colors, n_mat):
        self.params, self.device, self.eye, self.color_idx, self.material_idx = params, device, eye, color_idx, material_idx
        self.batched = batched_flags                      # which of pos / normal / eye / lights.pos carry B
        self.n_lights, self.n_colors, self.n_mat = n_lights, n_colors, n_mat

    def structs(self, pos, normal, lpos, colors, att, amb, albedo, coeffs):
        p = self.params
        N = p.width * p.height
        inp = _lib.SrhSplatNdcInputs(
            pos=pos.data_ptr(), pos_view_stride=N * p.pos_cols,
            normal=ptr(normal), normal_view_stride=(N * 3 if self.batched["normal"] else 0),
            eye=self.eye.data_ptr(), eye_view_stride=(3 if self.batched["eye"] else 0),
            lights_pos_view_stride=(self.n_lights * 4 if self.batched["lights_pos"] else 0),
            material_idx=ptr(self.material_idx))
        ls = _lib.SrhLights(n_lights=self.n_lights, n_colors=self.n_colors, pos=ptr(lpos),
                            color_idx=ptr(self.color_idx), colors=ptr(colors), attenuation=ptr(att), ambient=ptr(amb))
        ms = _lib.SrhMaterials(n_materials=self.n_mat, albedo=ptr(albedo), coeffs=ptr(coeffs))
        return inp, ls, ms


class _SplatNdcFunction(torch.autograd.Function):
    """(pos, normal, lights.pos, colors, attenuation, ambient, albedo, coeffs, view) -> (image, depth, pos), all with
    the leading view axis B.  The `normal` output is the caller's own tensor: autograd carries its gradient.  `view`
    [B, 3, 4] float64 or None is splats.camera_matrices' table: not read by the kernels, it is the input whose gradient
    is srh_splat_ndc_bwd_view's grad_view."""

    @staticmethod
    def forward(ctx, cfg: _SplatNdc, *args):
        *inputs, view = args
        p = cfg.params
        B, H, W = p.n_views, p.height, p.width
        dev = cfg.device
        image = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if p.shade else None
        depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        pos = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        inp, ls, ms = cfg.structs(*inputs)
        _lib.check(_lib.load().srh_splat_ndc_fwd(C.byref(p), C.byref(inp), C.byref(ls), C.byref(ms), ptr(image),
                                                 depth.data_ptr(), pos.data_ptr(), stream(dev)))
        ctx.cfg = cfg
        ctx.view = None if view is None else view.detach()
        ctx.set_materialize_grads(False)                   # an output the loss does not use arrives as None, not zeros
        ctx.save_for_backward(*inputs)
        if image is None:
            image = torch.zeros((B, H, W, 3), dtype=torch.float32, device=dev)
            ctx.mark_non_differentiable(image)
        return image, depth, pos

    @staticmethod
    def backward(ctx, g_image, g_depth, g_pos):
        cfg = ctx.cfg
        p = cfg.params
        inputs = list(ctx.saved_tensors)
        want = dict(zip(_DIFF, [ctx.needs_input_grad[1 + k] for k in range(len(inputs))]))
        if not p.shade:
            # a geometry-only frame (norm_depth_image_only) does not depend on the normals or the shading inputs: no
            # gradient, as under the reference's autograd (srh_splat_ndc_bwd refuses those buffers then)
            for k in _DIFF[1:]:
                want[k] = False
        B, N = p.n_views, p.width * p.height
        dev = cfg.device
        grads = {}
        if want["pos"]:
            grads["pos"] = torch.empty((B, N, p.pos_cols), dtype=torch.float32, device=dev)
        if want["normal"]:
            grads["normal"] = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        for k, t in zip(_DIFF[2:], inputs[2:]):
            if want[k]:
                grads[k] = torch.zeros_like(t)
        ups = [g.contiguous() if g is not None else None for g in (g_image, g_depth, g_pos)]
        if not p.shade:
            ups[0] = None

        lib = _lib.load()
        need_view = ctx.view is not None and ctx.needs_input_grad[-1]
        # only the image carries the camera: without its gradient the table's is zero, and nothing is launched for it
        vgrads, vws = view_grad_buffers(lib, (ctx.view,), (need_view and ups[0] is not None,), p.width, p.height)

        def launch():
            inp, ls, ms = cfg.structs(*inputs)
            sg = _lib.SrhSplatNdcGrads(**{k: v.data_ptr() for k, v in grads.items()})
            args = (C.byref(p), C.byref(inp), C.byref(ls), C.byref(ms), *[ptr(u) for u in ups], C.byref(sg))
            if vws is None:
                _lib.check(lib.srh_splat_ndc_bwd(*args, stream(dev)))
            else:
                _lib.check(lib.srh_splat_ndc_bwd_view(*args, vgrads[0].data_ptr(), vws.data_ptr(), vws.numel(),
                                                      stream(dev)))

        fill_grads(list(grads.values()) + vgrads, ups, launch)
        g_view = vgrads[0].view(B, 3, 4) if vgrads[0] is not None else (torch.zeros_like(ctx.view) if need_view else None)
        out = []
        for k, t in zip(_DIFF, inputs):
            g = grads.get(k)
            if g is not None and k in ("pos", "normal"):
                g = g.view(t.shape) if cfg.batched[k] else g.sum(0).view(t.shape)
            out.append(g)
        return (None, *out, g_view)


def _refuse_camera_grads(camera: Dict[str, Any]) -> None:
    for k, v in camera.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise ValueError(f"{_NAME}: camera['{k}'] requires grad, but the camera is not differentiable on this "
                             "path (detach it)")


def _validate(scene: Dict[str, Any], batched: bool) -> Tuple[int, int]:
    """Every shape and range the kernels rely on, checked on the host before anything reaches the GPU (ValueError).
    Returns the viewport's grid (W, H)."""
    cam, disk, lights = scene["camera"], scene["objects"]["disk"], scene["lights"]
    vp = np.asarray(_value(cam["viewport"])).reshape(-1)
    if vp.size != 4:
        raise ValueError(f"camera.viewport: expected 4 values, got {vp.size}")
    W, H = int(vp[2] - vp[0]), int(vp[3] - vp[1])
    if W < 1 or H < 1:
        raise ValueError(f"camera.viewport: empty {W} x {H} grid")
    N = W * H
    ps = _shape(disk.get("pos"))
    form = "[B, N, 3] or [B, N, 4]" if batched else "[N, 3] or [N, 4]"
    if ps is None or len(ps) != (3 if batched else 2):
        raise ValueError(f"objects.disk.pos: expected {form}, got {ps}")
    B = ps[0] if batched else None
    if ps[-2] != N or ps[-1] not in (3, 4) or (batched and B < 1):
        raise ValueError(f"objects.disk.pos: expected {form} with N = {W} x {H} = {N}, got {ps}")
    lp = _shape(lights.get("pos"))
    if lp is None or len(lp) < 2:
        raise ValueError(f"lights.pos: expected [L, 4]{' or [B, L, 4]' if batched else ''}, got {lp}")
    L = lp[-2]
    if not 1 <= L <= _lib.MAX_LIGHTS:
        raise ValueError(f"lights.pos: {L} lights, expected 1..{_lib.MAX_LIGHTS}")
    M = (_shape(scene["materials"].get("albedo")) or (0,))[0]

    def check(name, x, want, per_view, required=True):
        """`want`: the shape of one view; an entry None = any size >= 1."""
        s = _shape(x)
        if s is None:
            if required:
                raise ValueError(f"{name} is missing")
            return
        one = s
        if per_view and batched and len(s) == len(want) + 1:
            if s[0] != B:
                raise ValueError(f"{name}: leading dimension {s[0]}, the batch is {B}")
            one = s[1:]
        ok = len(one) == len(want) and all((w is None and d >= 1) or d == w for d, w in zip(one, want))
        if not ok:
            shown = "[" + ", ".join("*" if w is None else str(w) for w in want) + "]"
            raise ValueError(f"{name}: expected {shown}{' per view' if per_view and batched else ''}, got {list(s)}")

    nrm = _shape(disk.get("normal"))
    check("objects.disk.normal", disk.get("normal"), (N, nrm[-1] if nrm and nrm[-1] in (3, 4) else 3), True)
    check("objects.disk.material_idx", disk.get("material_idx"), (N,), False, required=False)
    check("lights.pos", lights.get("pos"), (L, 4), True)
    check("lights.color_idx", lights.get("color_idx"), (L,), False)
    check("lights.attenuation", lights.get("attenuation"), (L, 3), False)
    check("lights.ambient", lights.get("ambient"), (3,), False)
    check("colors", scene.get("colors"), (None, 3), False)
    check("materials.albedo", scene["materials"].get("albedo"), (None, 3), False)
    check("materials.coeffs", scene["materials"].get("coeffs"), (M, 3), False)
    eye = _shape(_value(cam.get("eye")))
    check("camera.eye", cam.get("eye"), (eye[-1] if eye and eye[-1] in (3, 4) else 4,), True)
    if eye[-1] == 4 and not np.all(np.asarray(_value(cam["eye"]), dtype=np.float64)[..., 3] == 1.0):
        raise ValueError("camera.eye: a 4-component eye must have w = 1")
    for k in ("at", "up"):
        if np.asarray(_value(cam.get(k))).size not in (3, 4):
            raise ValueError(f"camera.{k}: expected 3 or 4 values")
    near, far = float(_value(cam["near"])), float(_value(cam["far"]))
    if not (0.0 < near < far < math.inf):
        raise ValueError(f"camera.near / camera.far: expected 0 < near < far, got near = {near}, far = {far}")
    fovy = float(_value(cam["fovy"]))
    if not 0.0 < fovy < math.pi:
        raise ValueError(f"camera.fovy: expected a value in (0, pi), got {fovy}")
    return W, H


def _render(scene: Dict[str, Any], batched: bool, double_sided: bool = False, use_quartic: bool = False,
            norm_depth_image_only: bool = False, camera_grad: bool = False, **_unused) -> Dict[str, torch.Tensor]:
    cam = scene["camera"]
    if check_camera_grad(_NAME, camera_grad):
        camera_entries(_NAME, cam, (), camera_grad=True)
    else:
        _refuse_camera_grads(cam)
    W, H = _validate(scene, batched)
    disk, lights = scene["objects"]["disk"], scene["lights"]
    device = gpu_device(_NAME, (disk["pos"], disk["normal"]))
    pos = _f32(disk["pos"], device, "objects.disk.pos")
    if not batched:
        pos = pos.unsqueeze(0)
    B, N, pos_cols = pos.shape
    flags = {"pos": True}

    def per_view(x, name, dims):
        t = _f32(x, device, name)
        flags[name] = batched and t.dim() == dims + 1
        return t

    normal_in = per_view(disk["normal"], "normal", 2)         # all its columns: what norm_depth_image_only returns
    normal = normal_in[..., :3].contiguous()
    lpos = per_view(lights["pos"], "lights_pos", 2)
    L = lpos.shape[-2]
    eye = _f32(_value(cam["eye"]), device, "camera.eye")
    flags["eye"] = batched and eye.dim() == 2
    eye = eye[..., :3].contiguous()
    at = np.asarray(_value(cam["at"]), dtype=np.float64).reshape(-1)[:3]
    up = np.asarray(_value(cam["up"]), dtype=np.float64).reshape(-1)[:3]
    mat = disk.get("material_idx")
    mat = _i32(mat, device) if mat is not None else None
    colors = _f32(scene["colors"], device, "colors")
    albedo = _f32(scene["materials"]["albedo"], device, "materials.albedo")
    coeffs = _f32(scene["materials"]["coeffs"], device, "materials.coeffs")
    att = _f32(lights["attenuation"], device, "lights.attenuation")
    amb = _f32(lights["ambient"], device, "lights.ambient")
    far = float(_value(cam["far"]))
    params = _lib.SrhSplatNdcParams(n_views=B, width=W, height=H, pos_cols=pos_cols,
                                    use_quartic=int(bool(use_quartic)), double_sided=int(bool(double_sided)),
                                    shade=int(not norm_depth_image_only), fovy=float(_value(cam["fovy"])),
                                    near_clip=float(_value(cam["near"])), far_clip=far)
    params.at[:] = [float(v) for v in at]
    params.up[:] = [float(v) for v in up]
    cfg = _SplatNdc(params, device, eye, _i32(lights["color_idx"], device), mat, flags, L, colors.shape[0],
                    albedo.shape[0])
    # a frame without lights does not depend on the camera: no table, nothing launched for it
    view = camera_matrices(cam, B, device) if camera_grad and not norm_depth_image_only else None
    image, depth, pos_out = _SplatNdcFunction.apply(cfg, pos, normal, lpos, colors, att, amb, albedo, coeffs, view)
    if norm_depth_image_only:
        flat = depth.view(B, -1)
        mn = flat.min(dim=1).values.view(B, 1, 1)
        mx = flat.max(dim=1).values.view(B, 1, 1)
        nd = torch.where(depth >= far, mn.expand_as(depth), depth)
        pos4 = torch.cat((pos_out.view(B, N, 3), torch.ones((B, N, 1), dtype=torch.float32, device=device)), dim=2)
        nrm = normal_in if flags["normal"] else normal_in.unsqueeze(0).expand(B, *normal_in.shape)
        res = {"image": (nd - mn) / (mx - mn), "depth": depth, "pos": pos4, "normal": nrm}
    else:
        nrm = normal if flags["normal"] else normal.unsqueeze(0).expand(B, N, 3)
        res = {"image": image, "depth": depth, "pos": pos_out, "normal": nrm.reshape(B, H, W, 3)}
    if not torch.is_grad_enabled():
        # indexing a [N, 3] leaf with [..., :3] returns an alias that still says requires_grad under no_grad
        res["normal"] = res["normal"].detach()
    if not batched:
        res = {k: v[0] for k, v in res.items()}
    return res


def render_splats_NDC(scene: Dict[str, Any], **params) -> Dict[str, torch.Tensor]:
    """The reference's render_splats_NDC(scene, **params) on the GPU: image (H,W,3), depth (H,W), pos (H,W,3), normal
    (H,W,3) -- the given normals' first three columns, as they are.  With norm_depth_image_only=True the image (H,W) is
    the normalised depth, pos the homogeneous [N,4] (last column 1) and normal the input normals untouched.  Keywords:
    double_sided, use_quartic, norm_depth_image_only, and camera_grad: True lets camera['eye'], ['at'] and ['up'] require
    grad and gives them their gradient (see the module's text), its default False refuses them; others are ignored."""
    return _render(scene, batched=False, **params)


def render_splats_NDC_batch(scene: Dict[str, Any], **params) -> Dict[str, torch.Tensor]:
    """render_splats_NDC for B views in one forward launch and one backward launch: objects.disk.pos is [B, N, 3] or
    [B, N, 4]; objects.disk.normal [B, N, 3|4], camera.eye [B, 3|4] and lights.pos [B, L, 4] may carry the batch axis
    too (otherwise shared: a shared leaf's gradient is the sum over the views).  Every output has the leading axis B.
    camera_grad=True: a per-view eye gets its rows, a shared eye, at and up the sum over the views."""
    return _render(scene, batched=True, **params)
