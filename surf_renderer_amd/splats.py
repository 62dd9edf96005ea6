"""The reference's splat renderer on the GPU: ``render_splats_along_ray(scene, **params)`` as in
diffrend/torch/renderer.py:537-751, and a batched form for the GAN's per-element loop (diffrend/torch/GAN/gan.py:563-600).

    from surf_renderer_amd import render_splats_along_ray, render_splats_along_ray_batch
    res = render_splats_along_ray(scene, samples=1, normal_estimation_method='plane')
    res = render_splats_along_ray_batch(scene)   # objects.disk.pos [B, N] or [B, N, 3]; normal, light_vis,
                                                  # camera.eye and lights.pos optionally with a leading B as well

Forward and backward are HIP kernels (srh_splat_fwd / srh_splat_bwd, surf_renderer_amd/csrc/srh_splat.h): a batch is one
forward launch and one backward pass.  Differentiable inputs: objects.disk.pos (only z), objects.disk.normal,
objects.disk.light_vis, lights.pos, colors, lights.attenuation, lights.ambient, materials.albedo, materials.coeffs.

The camera enters only through the lights' camera coordinates, light_pos @ lookat(eye, at, up).T.  With
``camera_grad=True`` camera['eye'], ['at'] and ['up'] may require grad and receive it, in their own shape, dtype and
device (a fourth component gets 0; a leaf shared by the views of a batch gets the sum over the views, a per-view eye
[B, 3|4] its rows): srh_splat_bwd_view sums d loss / d (the view's 3 x 4 world-to-camera matrix) in fp64 without atomics,
and the chain from the matrix to eye / at / up is the reference's lookat in float64 on the host (camera_matrices).
Outputs and every other gradient are those of the same call with the camera detached.  A frame without lights
(norm_depth_image_only=True) does not depend on the camera: nothing is launched for it and the leaves' .grad stays None,
as under the reference's autograd; a shaded frame whose loss does not use `image` gives them exact zeros.  Without the
keyword a camera tensor that requires grad is refused, and fovy, focal_length and the viewport are refused either way.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._camera import VIEW_KEYS, _host, camera_entries, check_camera_grad, differentiable_vectors, view_matrices
from ._layer import f32, fill_grads, gpu_device, ptr, scratch, stream, view_grad_buffers

_DIFF = ("pos", "normal", "light_vis", "lights_pos", "colors", "attenuation", "ambient", "albedo", "coeffs")


def _value(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def _f32(x, device, name) -> torch.Tensor:
    if x is None:
        raise ValueError(f"render_splats_along_ray: scene value {name} is missing")
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
    return f32(t, device)


def _i32(x, device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=torch.int32).contiguous()


class _Splat:
    """Everything of one call that is not differentiated: the launch parameters, eye, indices, strides."""

    def __init__(self, params, device, eye, color_idx, material_idx, batched_flags, n_lights, n_colors, n_mat):
        self.params, self.device, self.eye, self.color_idx, self.material_idx = params, device, eye, color_idx, material_idx
        self.batched = batched_flags                      # which of pos / normal / light_vis / eye / lights.pos carry B
        self.n_lights, self.n_colors, self.n_mat = n_lights, n_colors, n_mat

    def structs(self, pos, normal, light_vis, lpos, colors, att, amb, albedo, coeffs):
        p = self.params
        N = p.width * p.height
        inp = _lib.SrhSplatInputs(
            pos=pos.data_ptr(), pos_view_stride=N * p.pos_cols,
            normal=ptr(normal), normal_view_stride=(N * 3 if self.batched["normal"] else 0),
            light_vis=ptr(light_vis), light_vis_view_stride=(self.n_lights * N if self.batched["light_vis"] else 0),
            eye=self.eye.data_ptr(), eye_view_stride=(3 if self.batched["eye"] else 0),
            lights_pos_view_stride=(self.n_lights * 4 if self.batched["lights_pos"] else 0),
            material_idx=ptr(self.material_idx))
        ls = _lib.SrhLights(n_lights=self.n_lights, n_colors=self.n_colors, pos=ptr(lpos),
                            color_idx=ptr(self.color_idx), colors=ptr(colors), attenuation=ptr(att), ambient=ptr(amb))
        ms = _lib.SrhMaterials(n_materials=self.n_mat, albedo=ptr(albedo), coeffs=ptr(coeffs))
        return inp, ls, ms

    def stream(self):
        return stream(self.device)


class _SplatFunction(torch.autograd.Function):
    """(pos, normal, light_vis, lights.pos, colors, attenuation, ambient, albedo, coeffs, view) -> (image, depth, pos,
    normal), all with the leading view axis B.  normal / light_vis may be None.  `view` [B, 3, 4] float64 or None is
    camera_matrices' table: the kernels do not read it (they build their basis from eye / at / up as ever), it is the
    input whose gradient is srh_splat_bwd_view's grad_view."""

    @staticmethod
    def forward(ctx, cfg: _Splat, *args):
        *inputs, view = args
        p = cfg.params
        B, K = p.n_views, p.samples
        KH, KW = K * p.height, K * p.width
        dev = cfg.device
        image = torch.empty((B, KH, KW, 3), dtype=torch.float32, device=dev) if p.shade else None
        depth = torch.empty((B, KH, KW), dtype=torch.float32, device=dev)
        pos = torch.empty((B, KH, KW, 3), dtype=torch.float32, device=dev)
        normal = torch.empty((B, KH, KW, 3), dtype=torch.float32, device=dev)
        inp, ls, ms = cfg.structs(*inputs)
        _lib.check(_lib.load().srh_splat_fwd(C.byref(p), C.byref(inp), C.byref(ls), C.byref(ms), ptr(image),
                                             depth.data_ptr(), pos.data_ptr(), normal.data_ptr(), cfg.stream()))
        ctx.cfg = cfg
        ctx.view = None if view is None else view.detach()
        ctx.present = [t is not None for t in inputs]
        ctx.save_for_backward(*[t for t in inputs if t is not None])
        if image is None:
            image = torch.zeros((B, KH, KW, 3), dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(*(() if p.shade else (image,)))
        return image, depth, pos, normal

    @staticmethod
    def backward(ctx, g_image, g_depth, g_pos, g_normal):
        cfg = ctx.cfg
        p = cfg.params
        saved = iter(ctx.saved_tensors)
        inputs = [next(saved) if present else None for present in ctx.present]
        want = dict(zip(_DIFF, [t is not None and ctx.needs_input_grad[1 + k] for k, t in enumerate(inputs)]))
        if not p.shade:
            # a geometry-only frame (norm_depth_image_only) does not depend on light_vis or the shading inputs: no
            # gradient, as under the reference's autograd (srh_splat_bwd refuses those buffers then)
            for k in _DIFF[2:]:
                want[k] = False
        B, N = p.n_views, p.width * p.height
        dev = cfg.device
        grads = {}
        if want["pos"]:
            grads["pos"] = torch.empty((B, N, p.pos_cols), dtype=torch.float32, device=dev)
        if want["normal"]:
            grads["normal"] = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        if want["light_vis"]:
            grads["light_vis"] = torch.empty((B, cfg.n_lights, N), dtype=torch.float32, device=dev)
        for k, t in zip(_DIFF[3:], inputs[3:]):
            if want[k]:
                grads[k] = torch.zeros_like(t)
        ups = [g.contiguous() if g is not None else None for g in (g_image, g_depth, g_pos, g_normal)]
        if not p.shade:
            ups[0] = None

        lib = _lib.load()
        vgrads, vws = view_grad_buffers(lib, (ctx.view,), (ctx.view is not None and ctx.needs_input_grad[-1],),
                                        p.width, p.height)

        def launch():
            inp, ls, ms = cfg.structs(*inputs)
            ws = scratch(max(lib.srh_splat_workspace_bytes(C.byref(p), C.byref(inp)), 8), dev)
            sg = _lib.SrhSplatGrads(**{k: v.data_ptr() for k, v in grads.items()})
            args = (C.byref(p), C.byref(inp), C.byref(ls), C.byref(ms), ws.data_ptr(), ws.numel(),
                    *[ptr(u) for u in ups], C.byref(sg))
            if vws is None:
                _lib.check(lib.srh_splat_bwd(*args, cfg.stream()))
            else:
                _lib.check(lib.srh_splat_bwd_view(*args, vgrads[0].data_ptr(), vws.data_ptr(), vws.numel(),
                                                  cfg.stream()))

        fill_grads(list(grads.values()) + vgrads, ups, launch)
        out = []
        for k, t in zip(_DIFF, inputs):
            g = grads.get(k)
            if g is not None and k in ("pos", "normal", "light_vis"):
                g = g.view(t.shape) if cfg.batched[k] else g.sum(0).view(t.shape)
            out.append(g)
        return (None, *out, None if vgrads[0] is None else vgrads[0].view(B, 3, 4))


def camera_matrices(camera: Dict[str, Any], B: int, device) -> Optional[torch.Tensor]:
    """The reference's lookat(eye, at, up) of every view, [B, 3, 4] float64 on `device`, attached to those of
    camera['eye' | 'at' | 'up'] that require grad -- eye [3|4] or [B, 3|4], at / up [3|4]; a shared one is expanded over
    the views, so it gets the sum, and the w column is dropped before lookat, so it gets 0.  None when none of them
    requires grad.  What the two splat renderers pass through autograd under camera_grad=True."""
    if not any(isinstance(camera[k], torch.Tensor) and camera[k].requires_grad for k in VIEW_KEYS):
        return None
    host = {k: np.asarray(_host(camera[k]), dtype=np.float64) for k in VIEW_KEYS}
    host = {k: torch.from_numpy(np.array(np.broadcast_to(v.reshape(-1, v.shape[-1]), (B, v.shape[-1]))[:, :3]))
            for k, v in host.items()}
    per_view = {k: (camera[k].reshape(1, -1).expand(B, -1) if isinstance(camera[k], torch.Tensor) and camera[k].dim() == 1
                    else camera[k]) for k in VIEW_KEYS}
    vec = differentiable_vectors(per_view, host)
    return view_matrices(vec["eye"], vec["at"], vec["up"]).to(device)


def _refuse_camera_grads(camera: Dict[str, Any]) -> None:
    for k, v in camera.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise ValueError(f"render_splats_along_ray: camera['{k}'] requires grad, but the camera is not "
                             "differentiable on this path (detach it)")


def _shape(x):
    return None if x is None else (tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x))


def _validate(scene: Dict[str, Any], batched: bool) -> Tuple[int, int]:
    """Every shape the kernels index by, checked on the host before anything reaches the GPU (ValueError).  Returns the
    viewport's grid (W, H)."""
    cam, disk, lights = scene["camera"], scene["objects"]["disk"], scene["lights"]
    vp = np.asarray(_value(cam["viewport"])).reshape(-1)
    if vp.size != 4:
        raise ValueError(f"camera.viewport: expected 4 values, got {vp.size}")
    W, H = int(vp[2] - vp[0]), int(vp[3] - vp[1])
    if W < 1 or H < 1:
        raise ValueError(f"camera.viewport: empty {W} x {H} grid")
    N = W * H
    ps = _shape(disk.get("pos"))
    if ps is None or (batched and len(ps) < 2):
        raise ValueError(f"objects.disk.pos: expected {'[B, N] or [B, N, 3]' if batched else '[N] or [N, 3]'}, got {ps}")
    B = ps[0] if batched else None
    if (ps[1:] if batched else ps) not in ((N,), (N, 3)):
        raise ValueError(f"objects.disk.pos: expected [N] or [N, 3] per view with N = {W} x {H} = {N}, got {ps}")
    lp = _shape(lights.get("pos"))
    if lp is None or len(lp) < 2:
        raise ValueError(f"lights.pos: expected [L, 4]{' or [B, L, 4]' if batched else ''}, got {lp}")
    L = lp[-2]
    if L > _lib.MAX_LIGHTS:
        raise ValueError(f"lights.pos: {L} lights, at most {_lib.MAX_LIGHTS}")
    M = (_shape(scene["materials"].get("albedo")) or (0,))[0]

    def check(name, x, want, per_view, required=True):
        """`want`: the shape of one view; entries None = any size >= 1, or a predicate on the whole shape."""
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
    if nrm is not None:
        check("objects.disk.normal", disk["normal"], (N, nrm[-1] if len(nrm) and nrm[-1] >= 3 else 3), True)
    check("objects.disk.light_vis", disk.get("light_vis"), (L, N), True, required=False)
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
    for k in ("at", "up"):
        if np.asarray(_value(cam.get(k))).size not in (3, 4):
            raise ValueError(f"camera.{k}: expected 3 or 4 values")
    return W, H


def _render(scene: Dict[str, Any], batched: bool, samples: int = 1, normal_estimation_method: str = "plane",
            normal_estimation_kernel_size: int = 3, use_quartic: bool = False, norm_depth_image_only: bool = False,
            camera_grad: bool = False, **_unused) -> Dict[str, torch.Tensor]:
    if normal_estimation_method != "plane":
        raise ValueError(f"render_splats_along_ray: normal_estimation_method {normal_estimation_method!r} is not "
                         "supported (only 'plane')")
    cam = scene["camera"]
    if check_camera_grad("render_splats_along_ray", camera_grad):
        camera_entries("render_splats_along_ray", cam, (), camera_grad=True)
    else:
        _refuse_camera_grads(cam)
    W, H = _validate(scene, batched)
    disk = scene["objects"]["disk"]
    pos_in = disk["pos"]
    device = gpu_device("render_splats_along_ray", (pos_in,))
    N = W * H
    pos = _f32(pos_in, device, "objects.disk.pos")
    if not batched:
        pos = pos.unsqueeze(0)
    B = pos.shape[0]
    if pos.dim() == 2:
        pos_cols = 1
    elif pos.dim() == 3 and pos.shape[2] == 3:
        pos_cols = 3
    else:
        raise ValueError(f"objects.disk.pos: expected [N] or [N, 3] per view, got {tuple(pos.shape)}")
    if pos.shape[1] != N:
        raise ValueError(f"objects.disk.pos holds {pos.shape[1]} splats per view, the {W} x {H} viewport needs {N}")
    flags = {}

    def per_view(x, name, dims):
        """(tensor, batched?) for an input with `dims` dimensions per view."""
        if x is None:
            flags[name] = False
            return None
        t = _f32(x, device, name)
        flags[name] = batched and t.dim() == dims + 1
        if flags[name] and t.shape[0] != B:
            raise ValueError(f"{name}: leading dimension {t.shape[0]}, batch is {B}")
        return t

    normal = disk.get("normal")
    normal = per_view(normal[..., :3] if normal is not None else None, "normal", 2)
    light_vis = per_view(disk.get("light_vis"), "light_vis", 2)
    flags["pos"] = True
    lights = scene["lights"]
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
    params = _lib.SrhSplatParams(n_views=B, width=W, height=H, samples=int(samples), pos_cols=pos_cols,
                                 use_quartic=int(bool(use_quartic)), shade=int(not norm_depth_image_only),
                                 fovy=float(_value(cam["fovy"])), focal_length=float(_value(cam["focal_length"])))
    params.at[:] = [float(v) for v in at]
    params.up[:] = [float(v) for v in up]
    cfg = _Splat(params, device, eye, _i32(lights["color_idx"], device), mat, flags, L, colors.shape[0],
                 albedo.shape[0])
    # a frame without lights does not depend on the camera: no table, nothing launched for it
    view = camera_matrices(cam, B, device) if camera_grad and not norm_depth_image_only else None
    image, depth, pos_out, normal_out = _SplatFunction.apply(cfg, pos, normal, light_vis, lpos, colors, att, amb,
                                                             albedo, coeffs, view)
    if norm_depth_image_only:
        far = float(_value(cam["far"]))
        flat = depth.view(B, -1)
        mn = flat.min(dim=1).values.view(B, 1, 1)
        mx = flat.max(dim=1).values.view(B, 1, 1)
        nd = torch.where(depth >= far, mn.expand_as(depth), depth)
        res = {"image": (nd - mn) / (mx - mn), "depth": depth, "pos": pos_out.view(B, -1, 3),
               "normal": normal_out.view(B, -1, 3)}
    else:
        res = {"image": image, "depth": depth, "pos": pos_out, "normal": normal_out}
    if not batched:
        res = {k: v[0] for k, v in res.items()}
    return res


def render_splats_along_ray(scene: Dict[str, Any], **params) -> Dict[str, torch.Tensor]:
    """The reference's render_splats_along_ray(scene, **params) on the GPU: image (KH,KW,3), depth (KH,KW),
    pos (KH,KW,3), normal (KH,KW,3); with norm_depth_image_only=True the image is the normalised depth and pos / normal
    are (KH KW, 3).  Keywords: samples, normal_estimation_method ('plane' only), normal_estimation_kernel_size (ignored,
    as in the reference), use_quartic, norm_depth_image_only, and camera_grad: True lets camera['eye'], ['at'] and ['up']
    require grad and gives them their gradient (see the module's text); its default False refuses them."""
    return _render(scene, batched=False, **params)


def render_splats_along_ray_batch(scene: Dict[str, Any], **params) -> Dict[str, torch.Tensor]:
    """render_splats_along_ray for B views in one forward launch and one backward pass: objects.disk.pos is [B, N] or
    [B, N, 3]; objects.disk.normal [B, N, 3], objects.disk.light_vis [B, L, N], camera.eye [B, 4] and lights.pos
    [B, L, 4] may carry the batch axis too (otherwise shared).  Every output has the leading axis B.  camera_grad=True:
    a per-view eye gets its rows, a shared eye, at and up the sum over the views."""
    return _render(scene, batched=True, **params)
