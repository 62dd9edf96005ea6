"""Gradient oracle -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A differentiable fp64 PyTorch restatement of the reference's numpy forward (``diffrend/numpy/renderer.py:204-272``)
used to check the hip backend's analytic backward.  Which primitive wins each pixel is taken from the numpy oracle
(``np_oracle.render``): the argmin and every mask of the reference are piecewise constant, so -- exactly as in the
reference's own differentiable backend (``diffrend/torch/renderer.py:136-355`` with ``torch/utils.py:238-366``,
where ``where`` is ``cond.float()*x + (1-cond)*y`` and ``min(0)`` routes the gradient to the winner) -- gradients flow
only through the winner's hit distance, hit point, normal, albedo and the lights.  Consequences that the analytic
backward reproduces (SURVEY.md section 8, row a-B): there are no silhouette gradients; a disc's radius gets zero
gradient; of a triangle only vertex 0 (the plane point, ``torch/utils.py:340``) and the supplied normal get
gradients.

Parity status: forward PINNED by the golden vectors (``tests/test_oracle_golden.py``); gradients PINNED by
``tests/golden/g9_torch_autograd.npz``, produced by running the reference's torch backend under autograd on a scene
where its shading model coincides with the numpy one (``oracle/golden_g9_g11.py``).
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import torch

from . import np_oracle

LEAF_KEYS = {
    "disk": ("pos", "normal", "radius"),
    "plane": ("pos", "normal"),
    "sphere": ("pos", "radius"),
    "triangle": ("face", "normal"),
}


def make_leaves(scene: Dict[str, Any], requires_grad: bool = True) -> Dict[str, torch.Tensor]:
    """fp64 leaf tensors for every differentiable input of an ndarray-leaf scene, keyed '<kind>.<field>',
    'lights.pos', 'colors', 'materials.albedo'."""
    leaves: Dict[str, torch.Tensor] = {}
    for kind, grp in scene["objects"].items():
        for name in LEAF_KEYS[kind]:
            leaves[f"{kind}.{name}"] = torch.tensor(np.asarray(grp[name], dtype=np.float64), requires_grad=requires_grad)
    leaves["lights.pos"] = torch.tensor(np.asarray(scene["lights"]["pos"], dtype=np.float64), requires_grad=requires_grad)
    leaves["colors"] = torch.tensor(np.asarray(scene["colors"], dtype=np.float64), requires_grad=requires_grad)
    leaves["materials.albedo"] = torch.tensor(np.asarray(scene["materials"]["albedo"], dtype=np.float64),
                                              requires_grad=requires_grad)
    return leaves


def _unit(v: torch.Tensor) -> torch.Tensor:
    """ops.normalize: divide by the norm, by 1 where it is 0 (numpy/ops.py:18-26)."""
    n = torch.sqrt(torch.sum(v * v, dim=-1, keepdim=True))
    return v / torch.where(n > 0, n, torch.ones_like(n))


def _norm(v: torch.Tensor) -> torch.Tensor:
    """|v| over the last axis (kept), with a zero gradient -- not sqrt's 0 * inf = NaN -- where v = 0: a pixel that hits
    nothing is given t = 0 below, so a light placed exactly at the eye coincides with its 'fragment', and the NaN would
    reach the light's gradient through the masked-out pixel."""
    sq = torch.sum(v * v, dim=-1, keepdim=True)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def _tap(taps, key: str, index, t: torch.Tensor) -> torch.Tensor:
    """With ``taps``: keep the gradient of ``t`` -- the per-pixel copy of leaf ``key`` (rows ``index`` of it; None: the
    whole leaf once per pixel; ('columns', index): per pixel the rows ``index`` of it, one term per pixel and column)
    -- so that its rows are the pixels' own terms of the leaf's gradient."""
    if taps is not None:
        t.retain_grad()
        taps.setdefault(key, []).append((index, t))
    return t


def render(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], ref: Optional[Dict[str, np.ndarray]] = None,
           taps=None):
    """Differentiable image (H,W,3) and depth (H,W).  ``ref`` = {'nearest', 'depth'} of the same scene (which
    primitive wins each pixel, and -- through depth being finite -- whether the pixel is hit at all); computed with
    the numpy oracle if not given.  ``scene`` supplies camera, index arrays and tonemap; ``leaves`` the
    differentiable arrays.  ``taps``: see _tap (gradient_terms)."""
    cam = scene["camera"]
    eye_np, ray_np, H, W = np_oracle.generate_rays(cam)
    if ref is None:
        ref = np_oracle.render(scene)
    nearest = np.asarray(ref["nearest"]).reshape(-1)
    hit_np = np.isfinite(np.asarray(ref["depth"]).reshape(-1))
    npix = H * W
    eye = torch.tensor(eye_np[:3])
    d = torch.tensor(ray_np[:3].T.copy())                                   # (N,3)
    orig = eye[None, :].expand(npix, 3)                                      # the numpy backend is perspective only

    t = torch.zeros(npix, dtype=torch.float64)
    nrm = torch.zeros((npix, 3), dtype=torch.float64)
    mat = np.zeros(npix, dtype=np.int64)
    start = 0
    for kind, grp in scene["objects"].items():
        count = (grp["face"] if kind == "triangle" else grp["pos"]).shape[0]
        sel = np.nonzero((nearest >= start) & (nearest < start + count))[0]
        if sel.size:
            loc = torch.as_tensor(nearest[sel] - start)
            ds = d[sel]
            mat[sel] = np.asarray(grp["material_idx"])[nearest[sel] - start]
            if kind == "sphere":
                c = _tap(taps, "sphere.pos", loc, leaves["sphere.pos"][loc])[:, :3]
                r = _tap(taps, "sphere.radius", loc, leaves["sphere.radius"][loc])
                oc = orig[sel] - c
                a = torch.sum(ds * ds, dim=-1)
                b = 2 * torch.sum(oc * ds, dim=-1)
                cc = torch.sum(oc * oc, dim=-1) - r * r
                disc = b * b - 4 * a * cc
                ok = disc >= 0
                root = torch.sqrt(torch.where(ok, disc, torch.zeros_like(disc)))
                t1 = (-b - root) / (2 * a)
                t2 = (-b + root) / (2 * a)
                one = torch.ones_like(t1)
                t1 = torch.where(ok & (t1 >= 0), t1, one)
                t2 = torch.where(ok & (t2 >= 0), t2, one)
                ts = torch.where(ok, torch.minimum(t1, t2), torch.zeros_like(t1))
                p = orig[sel] + ts[:, None] * ds
                v = p - c
                n = v / torch.sqrt(torch.sum(v * v, dim=-1, keepdim=True))
                n = torch.where(ok[:, None], n, torch.zeros_like(n))
            else:
                q = (_tap(taps, "triangle.face", loc, leaves["triangle.face"][loc])[:, 0, :3] if kind == "triangle"
                     else _tap(taps, f"{kind}.pos", loc, leaves[f"{kind}.pos"][loc])[:, :3])
                n = _unit(_tap(taps, f"{kind}.normal", loc, leaves[f"{kind}.normal"][loc]))[:, :3]
                ts = torch.sum(n * (q - orig[sel]), dim=-1) / torch.sum(n * ds, dim=-1)
            t = t.index_put((torch.as_tensor(sel),), ts)
            nrm = nrm.index_put((torch.as_tensor(sel),), n)
        start += count

    hit = torch.as_tensor(hit_np)
    # pixels that are not hit are background: depth inf, image tonemap(0)
    p = orig + t[:, None] * d
    cidx = torch.as_tensor(np.asarray(scene["lights"]["color_idx"]).astype(np.int64))
    if taps is None:
        lpos = leaves["lights.pos"][None, :, :3]
        lcol = leaves["colors"][cidx][None, :, :]
        alb = leaves["materials.albedo"][mat]
    else:
        # every pixel its own copy of the lights, and every (pixel, light) its own copy of the light's colour row: the
        # numpy shading has no per-light clip, so two lights that share a colour row can cancel within one pixel
        lpos = _tap(taps, "lights.pos", None, leaves["lights.pos"][None].expand(npix, *leaves["lights.pos"].shape))[:, :, :3]
        lcol = _tap(taps, "colors", ("columns", cidx), leaves["colors"][cidx][None].expand(npix, cidx.numel(), 3))
        alb = _tap(taps, "materials.albedo", torch.as_tensor(mat), leaves["materials.albedo"][mat])
    l = lpos - p[:, None, :]
    ln = _norm(l)
    l = l / torch.where(ln > 0, ln, torch.ones_like(ln))
    s = torch.sum(nrm[:, None, :] * l, dim=-1)                               # (N,L)
    im = torch.sum(s[:, :, None] * lcol * alb[:, None, :], dim=1)
    im = torch.where(hit[:, None], im, torch.zeros_like(im))
    im = torch.where(im < 0, torch.zeros_like(im), im)
    if "tonemap" in scene:
        g = float(np.ravel(scene["tonemap"]["gamma"])[0])
        im = torch.where(im > 0, im.clamp_min(1e-300) ** g, torch.zeros_like(im) if g > 0 else torch.ones_like(im))
    depth = torch.where(hit, t, torch.full_like(t, float("inf")))
    return im.reshape(H, W, 3), depth.reshape(H, W), hit.reshape(H, W)


def gradients(scene: Dict[str, Any], grad_image: np.ndarray, grad_depth: Optional[np.ndarray] = None,
              ref: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """d(sum(image*grad_image) + sum(depth*grad_depth over hit pixels)) / d(each leaf), as fp64 ndarrays."""
    leaves = make_leaves(scene)
    image, depth, hit = render(scene, leaves, ref)
    loss = torch.sum(image * torch.as_tensor(grad_image))
    if grad_depth is not None:
        gd = torch.as_tensor(grad_depth)
        loss = loss + torch.sum(torch.where(hit, depth * gd, torch.zeros_like(gd)))
    loss.backward()
    return {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in leaves.items()}


def _sum_taps(leaves: Dict[str, torch.Tensor], taps):
    """(total, absolute) per leaf from the retained gradients of its per-pixel copies."""
    total = {k: torch.zeros_like(v) for k, v in leaves.items()}
    absolute = {k: torch.zeros_like(v) for k, v in leaves.items()}
    for key, copies in taps.items():
        for index, t in copies:
            if t.grad is None:
                continue
            if index is None:
                total[key] += t.grad.sum(dim=0)
                absolute[key] += t.grad.abs().sum(dim=0)
            elif isinstance(index, tuple):
                total[key].index_add_(0, index[1], t.grad.sum(dim=0))
                absolute[key].index_add_(0, index[1], t.grad.abs().sum(dim=0))
            else:
                total[key].index_add_(0, index, t.grad)
                absolute[key].index_add_(0, index, t.grad.abs())
    return {k: v.numpy() for k, v in total.items()}, {k: v.numpy() for k, v in absolute.items()}


def gradient_terms(scene: Dict[str, Any], grad_image: Optional[np.ndarray], grad_depth: Optional[np.ndarray] = None,
                   ref: Optional[Dict[str, np.ndarray]] = None):
    """gradient_terms_tch for ``render`` (numpy shading): (total, absolute) per leaf -- the sum over the pixels of each
    pixel's own term of gradients()'s loss, and the sum of the terms' absolute values.  A light's colour row has one
    term per pixel AND light that reads it.  ``grad_image`` None: the depth term alone."""
    leaves = make_leaves(scene)
    taps: Dict[str, Any] = {}
    image, depth, hit = render(scene, leaves, ref, taps=taps)
    loss = torch.zeros((), dtype=torch.float64)
    if grad_image is not None:
        loss = loss + torch.sum(image * torch.as_tensor(np.asarray(grad_image, dtype=np.float64)))
    if grad_depth is not None:
        gd = torch.as_tensor(np.asarray(grad_depth, dtype=np.float64))
        loss = loss + torch.sum(torch.where(hit, depth * gd, torch.zeros_like(gd)))
    if loss.requires_grad:
        loss.backward()
    return _sum_taps(leaves, taps)


# ------------------------------------------------------------------------------------------------------------------
# torch-backend semantics (render(scene, shading='torch')): fp64 torch restatement of np_oracle_tch.render
# ------------------------------------------------------------------------------------------------------------------
TCH_EXTRA_LEAVES = ("lights.attenuation", "lights.ambient", "materials.coeffs")


def make_leaves_tch(scene: Dict[str, Any], requires_grad: bool = True) -> Dict[str, torch.Tensor]:
    leaves = make_leaves(scene, requires_grad)
    leaves["lights.attenuation"] = torch.tensor(np.asarray(scene["lights"]["attenuation"], dtype=np.float64),
                                                requires_grad=requires_grad)
    leaves["lights.ambient"] = torch.tensor(np.asarray(scene["lights"]["ambient"], dtype=np.float64),
                                            requires_grad=requires_grad)
    leaves["materials.coeffs"] = torch.tensor(np.asarray(scene["materials"]["coeffs"], dtype=np.float64),
                                              requires_grad=requires_grad)
    return leaves


def _unit3_eps(v: torch.Tensor) -> torch.Tensor:
    """torch/utils.py:131-135: v / sqrt(sum(v^2 + 1e-10)) over xyz."""
    return v / torch.sqrt(torch.sum(v * v + 1e-10, dim=-1, keepdim=True))


OUTPUTS = ("image", "depth", "normal", "pos")
CAMERA_KEYS = ("camera.eye", "camera.at", "camera.up")


def make_camera_leaves(camera: Dict[str, Any], requires_grad: bool = True) -> Dict[str, torch.Tensor]:
    """eye, at, up as fp64 leaves holding the float32 values the torch backend holds (np_oracle_tch.cam_vec)."""
    from . import np_oracle_tch
    return {"camera." + k: torch.tensor(np_oracle_tch.cam_vec(camera[k]), requires_grad=requires_grad)
            for k in ("eye", "at", "up")}


def rays_np(camera: Dict[str, Any]):
    """(eye (3), origin (N,3), direction (N,3), H, W) as fp64 constants from np_oracle_tch's ray generators: the graph
    is cut at the camera.  This is the default path, and its values are the numpy oracle's to the bit."""
    from . import np_oracle_tch
    if np_oracle_tch.is_ortho(camera):
        # torch/utils.py:461-468: every ray has its own origin on the image plane and the one direction at - eye
        eye_np, orig_np, dvec, H, W = np_oracle_tch.generate_rays_ortho(camera)
        orig = torch.tensor(np.ascontiguousarray(orig_np))                  # (N,3)
        d = torch.tensor(np.broadcast_to(dvec[None, :], orig_np.shape).copy())
    else:
        eye_np, ray_np, H, W = np_oracle_tch.generate_rays(camera)
        d = torch.tensor(ray_np.T.copy())                                   # (N,3), unit
        orig = torch.tensor(eye_np[:3])[None, :].expand(d.shape[0], 3)
    return torch.tensor(eye_np[:3]), orig, d, H, W


def rays(camera: Dict[str, Any], cam_leaves: Dict[str, torch.Tensor]):
    """(eye (3), origin (N,3), direction (N,3), H, W), differentiable in the camera leaves: the CAMERA inside the
    graph.  The rays are built with torch from ``eye`` / ``at`` / ``up`` by the reference's formulae
    (torch/utils.py:402-427 lookat_rot_inv, :439-478 generate_rays, its in-place ``ray_dir /=`` read as d = v / |v|).
    rays_np builds the same rays in numpy, which cuts the graph at the camera; this builder exists for that reason
    alone, and tests/test_camera_grad_golden_cpu.py holds the two to 1e-12 of each other."""
    from . import np_oracle_tch
    vp = camera["viewport"]
    W, H = vp[2] - vp[0], vp[3] - vp[1]
    h = np.tan(camera["fovy"] / 2) * 2 * camera["focal_length"]
    w = h * (float(W) / float(H))
    xg, yg = np.meshgrid(np.linspace(-1, 1, W), np.linspace(1, -1, H))
    x = torch.tensor(xg.ravel() * (w / 2))
    y = torch.tensor(yg.ravel() * (h / 2))
    eye = cam_leaves["camera.eye"][:3]
    at = cam_leaves["camera.at"][:3]
    up = cam_leaves["camera.up"][:3]
    z = _unit3_eps(eye - at)
    xb = _unit3_eps(torch.linalg.cross(_unit3_eps(up), z))
    yb = torch.linalg.cross(z, xb)
    if np_oracle_tch.is_ortho(camera):
        orig = eye[None, :] + x[:, None] * xb[None, :] + y[:, None] * yb[None, :]
        d = _unit3_eps(at - eye)[None, :].expand(orig.shape[0], 3)
    else:
        rot = torch.stack((xb, yb, z), dim=-1)
        v = rot @ torch.stack((x, y, -torch.ones_like(x) * camera["focal_length"]), dim=0)
        d = (v / torch.sqrt(torch.sum(v ** 2, dim=0))).T
        orig = eye[None, :].expand(d.shape[0], 3)
    return eye, orig, d, H, W


def _render_core(ray_set, scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], ref: Optional[Dict[str, np.ndarray]],
                 double_sided: bool, use_quartic: bool, visibility: Optional[np.ndarray], outputs=OUTPUTS, taps=None,
                 only_light: Optional[int] = None):
    """The one fp64 autograd restatement of the torch backend (diffrend/torch/renderer.py:82-125,136-355; see
    oracle/np_oracle_tch.py for the forward restatement and its two documented deviations) on the rays of rays_np or
    rays: (image (H,W,3), depth (H,W), normal (H,W,3), pos (H,W,3), hit (H,W)).  The shading is built -- and image is
    not None -- only if 'image' is among ``outputs``, so a geometry-only loss pays for no light.

    Winners are taken as given (``ref`` = {'nearest', 'depth'}: np_oracle_tch's, a reference fixture's or a GPU
    frame's); selection and every mask (per-light relu, double_sided sign, clip) are piecewise constant, as under the
    reference's autograd, and light ``visibility`` is an optional (L,N) constant.  At a hit pixel with winner m:
    normal = n^ = n / sqrt(|n|^2 + 3e-10) (sphere: p - c likewise), NOT flipped by double_sided, which flips only
    inside the shading; pos = origin + t d (per-pixel origin for orthographic cameras).  Misses: normal and pos are 0,
    depth is far + 1, and upstream gradients there are ignored (the reference differentiates object 0's intersection
    there; the hip backend does not -- the one deliberate difference).  Misses contribute nothing, which is also how
    the sphere case is defined where the reference itself yields NaN.

    ``only_light`` = l: the image is replaced by its linearisation in light l's own contribution (its weight times
    colour times albedo plus its share of the ambient term) -- d out / d im, taken at the full image and held constant,
    times that contribution -- so a loss on it has light l's share of the image path's gradients, and the shares of all
    lights add up to the whole (gradient_terms_tch)."""
    from . import np_oracle_tch
    cam = scene["camera"]
    eye, orig, d, H, W = ray_set
    if ref is None:
        ref = np_oracle_tch.render(scene, double_sided=double_sided, use_quartic=use_quartic)
    nearest = np.asarray(ref["nearest"]).reshape(-1)
    hit_np = np.asarray(ref["depth"]).reshape(-1) <= cam["far"]
    npix = H * W

    t = torch.zeros(npix, dtype=torch.float64)
    nrm = torch.zeros((npix, 3), dtype=torch.float64)
    mat = np.zeros(npix, dtype=np.int64)
    start = 0
    for kind, grp in scene["objects"].items():
        count = (grp["face"] if kind == "triangle" else grp["pos"]).shape[0]
        sel = np.nonzero(hit_np & (nearest >= start) & (nearest < start + count))[0]
        if sel.size:
            loc = torch.as_tensor(nearest[sel] - start)
            ds = d[sel]
            mat[sel] = np.asarray(grp["material_idx"])[nearest[sel] - start]
            if kind == "sphere":
                c = _tap(taps, "sphere.pos", loc, leaves["sphere.pos"][loc])[:, :3]
                r = _tap(taps, "sphere.radius", loc, leaves["sphere.radius"][loc])
                oc = orig[sel] - c
                a = torch.sum(ds * ds, dim=-1)
                b = 2 * torch.sum(oc * ds, dim=-1)
                cc = torch.sum(oc * oc, dim=-1) - r * r
                root = torch.sqrt(torch.clamp_min(b * b - 4 * a * cc, 0.0))
                t1 = (-b - root) / (2 * a)
                t2 = (-b + root) / (2 * a)
                ts = torch.where(t1 >= 0, t1, t2)                             # the smaller non-negative root
                n = _unit3_eps(orig[sel] + ts[:, None] * ds - c)
            else:
                q = (_tap(taps, "triangle.face", loc, leaves["triangle.face"][loc])[:, 0, :3] if kind == "triangle"
                     else _tap(taps, f"{kind}.pos", loc, leaves[f"{kind}.pos"][loc])[:, :3])
                n = _unit3_eps(_tap(taps, f"{kind}.normal", loc, leaves[f"{kind}.normal"][loc])[:, :3])
                ts = torch.sum(n * (q - orig[sel]), dim=-1) / torch.sum(n * ds, dim=-1)
            t = t.index_put((torch.as_tensor(sel),), ts)
            nrm = nrm.index_put((torch.as_tensor(sel),), n)
        start += count

    hit = torch.as_tensor(hit_np)
    p = orig + t[:, None] * d
    im = None
    if "image" in outputs:
        if taps is None:
            lpos = leaves["lights.pos"][None, :, :3]
            lcol = leaves["colors"][np.asarray(scene["lights"]["color_idx"])][None, :, :]
            att = leaves["lights.attenuation"][None]
            amb = leaves["lights.ambient"][None, None, :]
        else:                                                                # every pixel its own copy of the shared leaves
            def per_pixel(key):
                return _tap(taps, key, None, leaves[key][None].expand(npix, *leaves[key].shape))
            lpos = per_pixel("lights.pos")[:, :, :3]
            lcol = per_pixel("colors")[:, np.asarray(scene["lights"]["color_idx"])]
            att = per_pixel("lights.attenuation")
            amb = per_pixel("lights.ambient")[:, None, :]
        mat_t = torch.as_tensor(mat)
        alb = _tap(taps, "materials.albedo", mat_t, leaves["materials.albedo"][mat])
        cf = _tap(taps, "materials.coeffs", mat_t, leaves["materials.coeffs"][mat])
        ldir = lpos - p[:, None, :]                                          # (N,L,3)
        lnorm = _norm(ldir)                                                  # a light exactly at a fragment: gradient 0
        ldir = ldir / torch.where(lnorm > 0, lnorm, torch.ones_like(lnorm))
        powv = 4 if use_quartic else 2
        den = att[:, :, 0:1] + lnorm * att[:, :, 1:2] + (lnorm ** powv) * att[:, :, 2:3]
        afac = 1.0 / torch.where(den.abs() > 0, den, torch.ones_like(den))
        ldn = torch.sum(nrm[:, None, :] * ldir, dim=-1)                      # (N,L)
        ndotl = afac[..., 0] * ldn
        cdir = _unit3_eps(eye[None, :] - p)                                  # (N,3): the eye, not the ray origin
        cdotn = torch.sum(cdir * nrm, dim=-1)
        rdotc = 2.0 * ldn * cdotn[:, None] - torch.sum(cdir[:, None, :] * ldir, dim=-1)
        if double_sided:
            sgn = torch.sign(cdotn).detach()[:, None]
            ndotl = sgn * ndotl
            rdotc = sgn * rdotc
        ndotl = torch.relu(ndotl)
        rdotc = torch.relu(rdotc)
        spec = cf[:, None, 1] * rdotc ** cf[:, None, 2]                      # torch.pow: 0 ** 0 = 1, masked gradients at 0
        w = cf[:, None, 0] * ndotl + spec                                    # (N,L)
        if visibility is not None:                                           # (L,N) constants: shadow rays
            w = w * torch.as_tensor(np.asarray(visibility, dtype=np.float64).reshape(w.shape[1], -1).T)
        col = w[:, :, None] * (lcol * alb[:, None, :]) + amb * alb[:, None, :]
        im = torch.sum(col, dim=1)
        im = torch.where(hit[:, None], im, torch.zeros_like(im))
        if only_light is not None:
            full = im.detach()
            slope = (full > 0).to(full.dtype)
            if "tonemap" in scene:
                g = float(np.ravel(scene["tonemap"]["gamma"])[0])
                slope = torch.where(full > 0, g * full.clamp_min(1e-300) ** (g - 1.0), torch.zeros_like(full))
            im = slope * torch.where(hit[:, None], col[:, only_light], torch.zeros_like(full))
        else:
            im = torch.relu(im)
            if "tonemap" in scene:
                g = float(np.ravel(scene["tonemap"]["gamma"])[0])
                im = torch.where(im > 0, im.clamp_min(1e-300) ** g, torch.zeros_like(im) if g > 0 else torch.ones_like(im))
        im = im.reshape(H, W, 3)
    # after the shading: autograd runs later-created nodes first, so this placement fixes the order in which p collects
    # its gradients (profiles/grad_oracle_unify_ab.txt)
    depth = torch.where(hit, t, torch.full_like(t, float(cam["far"]) + 1.0))
    pos = torch.where(hit[:, None], p, torch.zeros_like(p))
    return im, depth.reshape(H, W), nrm.reshape(H, W, 3), pos.reshape(H, W, 3), hit.reshape(H, W)


def render_tch(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], ref: Optional[Dict[str, np.ndarray]] = None,
               double_sided: bool = False, use_quartic: bool = False, visibility: Optional[np.ndarray] = None):
    """Differentiable image (H,W,3), depth (H,W) and hit mask under the torch backend's semantics, on numpy rays."""
    image, depth, _, _, hit = _render_core(rays_np(scene["camera"]), scene, leaves, ref, double_sided, use_quartic,
                                           visibility)
    return image, depth, hit


def render_aux(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], ref: Optional[Dict[str, np.ndarray]] = None,
               double_sided: bool = False, use_quartic: bool = False):
    """Differentiable normal (H,W,3), pos (H,W,3) and the hit mask (H,W), zeros at misses, on numpy rays: the torch
    backend's extra outputs (diffrend/torch/renderer.py:185-189, 342-355), without the shading.  Pinned to the
    reference by tests/test_aux_grad_golden_cpu.py (tests/golden/n1_*.npz, oracle/golden_n1.py)."""
    _, _, normal, pos, hit = _render_core(rays_np(scene["camera"]), scene, leaves, ref, double_sided, use_quartic, None,
                                          outputs=("normal", "pos"))
    return normal, pos, hit


def render_camera(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], cam_leaves: Dict[str, torch.Tensor],
                  ref: Dict[str, np.ndarray], double_sided: bool = False, use_quartic: bool = False,
                  visibility: Optional[np.ndarray] = None):
    """Differentiable image, depth, normal, pos and the hit mask on the rays of the camera leaves.  Pinned to the
    reference by tests/test_camera_grad_golden_cpu.py (tests/golden/c1_*.npz, oracle/golden_c1_c2.py)."""
    return _render_core(rays(scene["camera"], cam_leaves), scene, leaves, ref, double_sided, use_quartic, visibility)


def loss_camera(scene, leaves, cam_leaves, ref, grad_image=None, grad_depth=None, grad_normal=None, grad_pos=None,
                double_sided=False, use_quartic=False, visibility=None, taps=None, only_light=None) -> torch.Tensor:
    """sum image g_i + sum_hit (depth g_d + normal . g_n + pos . g_p) of ONE graph; None terms are left out, and so is
    the shading without g_i.  ``cam_leaves`` None: numpy rays, the camera outside the graph."""
    grads = dict(zip(OUTPUTS, (grad_image, grad_depth, grad_normal, grad_pos)))
    ray_set = rays_np(scene["camera"]) if cam_leaves is None else rays(scene["camera"], cam_leaves)
    *outs, hit = _render_core(ray_set, scene, leaves, ref, double_sided, use_quartic, visibility,
                              outputs=[k for k, g in grads.items() if g is not None], taps=taps, only_light=only_light)
    loss = torch.zeros((), dtype=torch.float64)
    for out, (name, g) in zip(outs, grads.items()):
        if g is not None:
            term = out * torch.as_tensor(np.asarray(g, dtype=np.float64))
            if name != "image":
                term = torch.where(hit if name == "depth" else hit[..., None], term, torch.zeros_like(term))
            loss = loss + torch.sum(term)
    return loss


def gradients_tch(scene: Dict[str, Any], grad_image: Optional[np.ndarray] = None,
                  grad_depth: Optional[np.ndarray] = None, grad_normal: Optional[np.ndarray] = None,
                  grad_pos: Optional[np.ndarray] = None, *, ref: Optional[Dict[str, np.ndarray]] = None,
                  double_sided: bool = False, use_quartic: bool = False, visibility: Optional[np.ndarray] = None,
                  camera: bool = False) -> Dict[str, np.ndarray]:
    """d loss_camera / d leaf as fp64 ndarrays for every scene leaf and, with ``camera``, for 'camera.eye',
    'camera.at', 'camera.up' (4 values each, w = 0 -- the reference slices [:3] before anything else)."""
    leaves = make_leaves_tch(scene)
    cam_leaves = make_camera_leaves(scene["camera"]) if camera else None
    loss = loss_camera(scene, leaves, cam_leaves, ref, grad_image, grad_depth, grad_normal, grad_pos, double_sided,
                       use_quartic, visibility)
    if loss.requires_grad:
        loss.backward()
    out = {}
    for k, v in {**leaves, **(cam_leaves or {})}.items():
        g = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
        out[k] = np.append(g, 0.0) if (k in CAMERA_KEYS and g.size == 3) else g
    return out


def gradient_terms_tch(scene: Dict[str, Any], grad_image: Optional[np.ndarray] = None,
                       grad_depth: Optional[np.ndarray] = None, grad_normal: Optional[np.ndarray] = None,
                       grad_pos: Optional[np.ndarray] = None, *, ref: Optional[Dict[str, np.ndarray]] = None,
                       double_sided: bool = False, use_quartic: bool = False, visibility: Optional[np.ndarray] = None,
                       only_light: Optional[int] = None):
    """(total, absolute): per scene leaf the sum over the pixels of each pixel's own term of d loss_camera / d leaf --
    gradients_tch's values -- and the sum of the terms' absolute values, which says how hard that sum cancels: an fp32
    accumulation of the terms in an arbitrary order is uncertain by about ``absolute`` x 2^-23.  Numpy rays.
    ``only_light``: one light's share of the image path (_render_core); the shares' totals add up to the whole's."""
    leaves = make_leaves_tch(scene)
    taps: Dict[str, Any] = {}
    loss = loss_camera(scene, leaves, None, ref, grad_image, grad_depth, grad_normal, grad_pos, double_sided,
                       use_quartic, visibility, taps=taps, only_light=only_light)
    if loss.requires_grad:
        loss.backward()
    return _sum_taps(leaves, taps)
