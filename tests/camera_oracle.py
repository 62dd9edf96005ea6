"""fp64 autograd restatement of the torch backend with the CAMERA inside the graph: the rays are built with torch from
``eye`` / ``at`` / ``up`` leaves by the reference's formulae (torch/utils.py:402-427 lookat_rot_inv, :439-478
generate_rays, its in-place division read as d = v / |v|), and everything after the rays is term for term what
oracle/torch_oracle.render_tch (image, depth) and tests/aux_oracle.render_aux (normal, pos) compute.  Those two build
their rays in numpy, which cuts the graph at the camera; this helper exists for that reason alone.

Winners are taken as given (``ref`` -- a reference fixture's or the GPU frame's ``nearest`` and ``depth``), light
visibility is optional; selection and every mask are piecewise constant.  Misses contribute nothing, which is also
how the sphere case is defined where the reference itself yields NaN.  Pinned to the reference by
tests/test_camera_grad_golden_cpu.py (tests/golden/c1_*.npz, tools/gen_golden_camera_grad.py)."""
from typing import Any, Dict, Optional

import numpy as np
import torch

from oracle import np_oracle_tch, torch_oracle

CAMERA_KEYS = ("camera.eye", "camera.at", "camera.up")


def make_camera_leaves(camera: Dict[str, Any], requires_grad: bool = True) -> Dict[str, torch.Tensor]:
    """eye, at, up as fp64 leaves holding the float32 values the torch backend holds (np_oracle_tch.cam_vec)."""
    return {"camera." + k: torch.tensor(np_oracle_tch.cam_vec(camera[k]), requires_grad=requires_grad)
            for k in ("eye", "at", "up")}


def _unit3(v: torch.Tensor) -> torch.Tensor:
    return torch_oracle._unit3_eps(v)


def rays(camera: Dict[str, Any], cam_leaves: Dict[str, torch.Tensor]):
    """(eye (3), origin (N,3), direction (N,3), H, W), differentiable in the camera leaves."""
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
    z = _unit3(eye - at)
    xb = _unit3(torch.linalg.cross(_unit3(up), z))
    yb = torch.linalg.cross(z, xb)
    if np_oracle_tch.is_ortho(camera):
        orig = eye[None, :] + x[:, None] * xb[None, :] + y[:, None] * yb[None, :]
        d = _unit3(at - eye)[None, :].expand(orig.shape[0], 3)
    else:
        rot = torch.stack((xb, yb, z), dim=-1)
        v = rot @ torch.stack((x, y, -torch.ones_like(x) * camera["focal_length"]), dim=0)
        d = (v / torch.sqrt(torch.sum(v ** 2, dim=0))).T
        orig = eye[None, :].expand(d.shape[0], 3)
    return eye, orig, d, H, W


def render_camera(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], cam_leaves: Dict[str, torch.Tensor],
                  ref: Dict[str, np.ndarray], double_sided: bool = False, use_quartic: bool = False,
                  visibility: Optional[np.ndarray] = None):
    """Differentiable image (H,W,3), depth (H,W), normal (H,W,3), pos (H,W,3) and the hit mask (H,W)."""
    cam = scene["camera"]
    eye, orig, d, H, W = rays(cam, cam_leaves)
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
                c = leaves["sphere.pos"][loc][:, :3]
                r = leaves["sphere.radius"][loc]
                oc = orig[sel] - c
                a = torch.sum(ds * ds, dim=-1)
                b = 2 * torch.sum(oc * ds, dim=-1)
                cc = torch.sum(oc * oc, dim=-1) - r * r
                root = torch.sqrt(torch.clamp_min(b * b - 4 * a * cc, 0.0))
                t1 = (-b - root) / (2 * a)
                t2 = (-b + root) / (2 * a)
                ts = torch.where(t1 >= 0, t1, t2)                             # the smaller non-negative root
                n = _unit3(orig[sel] + ts[:, None] * ds - c)
            else:
                q = (leaves["triangle.face"][loc][:, 0, :3] if kind == "triangle" else leaves[f"{kind}.pos"][loc][:, :3])
                n = _unit3(leaves[f"{kind}.normal"][loc][:, :3])
                ts = torch.sum(n * (q - orig[sel]), dim=-1) / torch.sum(n * ds, dim=-1)
            t = t.index_put((torch.as_tensor(sel),), ts)
            nrm = nrm.index_put((torch.as_tensor(sel),), n)
        start += count

    hit = torch.as_tensor(hit_np)
    p = orig + t[:, None] * d
    lpos = leaves["lights.pos"][:, :3]
    lcol = leaves["colors"][np.asarray(scene["lights"]["color_idx"])]
    att = leaves["lights.attenuation"]
    amb = leaves["lights.ambient"]
    alb = leaves["materials.albedo"][mat]
    cf = leaves["materials.coeffs"][mat]
    ldir = lpos[None, :, :] - p[:, None, :]                                  # (N,L,3)
    lnorm = torch.sqrt(torch.sum(ldir * ldir, dim=-1, keepdim=True))
    ldir = ldir / torch.where(lnorm > 0, lnorm, torch.ones_like(lnorm))
    powv = 4 if use_quartic else 2
    den = att[None, :, 0:1] + lnorm * att[None, :, 1:2] + (lnorm ** powv) * att[None, :, 2:3]
    afac = 1.0 / torch.where(den.abs() > 0, den, torch.ones_like(den))
    ldn = torch.sum(nrm[:, None, :] * ldir, dim=-1)                          # (N,L)
    ndotl = afac[..., 0] * ldn
    cdir = _unit3(eye[None, :] - p)                                          # (N,3): the eye, not the ray origin
    cdotn = torch.sum(cdir * nrm, dim=-1)
    rdotc = 2.0 * ldn * cdotn[:, None] - torch.sum(cdir[:, None, :] * ldir, dim=-1)
    if double_sided:
        sgn = torch.sign(cdotn).detach()[:, None]
        ndotl = sgn * ndotl
        rdotc = sgn * rdotc
    ndotl = torch.relu(ndotl)
    rdotc = torch.relu(rdotc)
    spec = cf[:, None, 1] * rdotc ** cf[:, None, 2]
    wgt = cf[:, None, 0] * ndotl + spec                                      # (N,L)
    if visibility is not None:                                               # (L,N) constants: shadow rays
        wgt = wgt * torch.as_tensor(np.asarray(visibility, dtype=np.float64).reshape(wgt.shape[1], -1).T)
    col = wgt[:, :, None] * (lcol[None, :, :] * alb[:, None, :]) + amb[None, None, :] * alb[:, None, :]
    im = torch.sum(col, dim=1)
    im = torch.where(hit[:, None], im, torch.zeros_like(im))
    im = torch.relu(im)
    if "tonemap" in scene:
        g = float(np.ravel(scene["tonemap"]["gamma"])[0])
        im = torch.where(im > 0, im.clamp_min(1e-300) ** g, torch.zeros_like(im) if g > 0 else torch.ones_like(im))
    depth = torch.where(hit, t, torch.full_like(t, float(cam["far"]) + 1.0))
    pos = torch.where(hit[:, None], p, torch.zeros_like(p))
    return (im.reshape(H, W, 3), depth.reshape(H, W), nrm.reshape(H, W, 3), pos.reshape(H, W, 3), hit.reshape(H, W))


def loss_camera(scene, leaves, cam_leaves, ref, grad_image=None, grad_depth=None, grad_normal=None, grad_pos=None,
                double_sided=False, use_quartic=False, visibility=None) -> torch.Tensor:
    """sum image g_i + sum_hit (depth g_d + normal . g_n + pos . g_p); None terms are left out."""
    image, depth, normal, pos, hit = render_camera(scene, leaves, cam_leaves, ref, double_sided, use_quartic, visibility)
    loss = torch.zeros((), dtype=torch.float64)
    if grad_image is not None:
        loss = loss + torch.sum(image * torch.as_tensor(np.asarray(grad_image, dtype=np.float64)))
    if grad_depth is not None:
        gd = torch.as_tensor(np.asarray(grad_depth, dtype=np.float64))
        loss = loss + torch.sum(torch.where(hit, depth * gd, torch.zeros_like(gd)))
    for out, g in ((normal, grad_normal), (pos, grad_pos)):
        if g is not None:
            loss = loss + torch.sum(torch.where(hit[..., None], out * torch.as_tensor(np.asarray(g, dtype=np.float64)),
                                                torch.zeros_like(out)))
    return loss


def gradients_camera(scene: Dict[str, Any], ref: Dict[str, np.ndarray], grad_image=None, grad_depth=None,
                     grad_normal=None, grad_pos=None, double_sided: bool = False, use_quartic: bool = False,
                     visibility: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """d loss / d leaf for every scene leaf (keys and shapes as torch_oracle.gradients_tch) and for 'camera.eye',
    'camera.at', 'camera.up' (4 values each, w = 0 -- the reference slices [:3] before anything else)."""
    leaves = torch_oracle.make_leaves_tch(scene)
    cam_leaves = make_camera_leaves(scene["camera"])
    loss = loss_camera(scene, leaves, cam_leaves, ref, grad_image, grad_depth, grad_normal, grad_pos, double_sided,
                       use_quartic, visibility)
    if loss.requires_grad:
        loss.backward()
    out = {}
    for k, v in {**leaves, **cam_leaves}.items():
        g = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
        out[k] = np.append(g, 0.0) if (k in CAMERA_KEYS and g.size == 3) else g
    return out
