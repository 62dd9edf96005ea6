"""fp64 autograd restatement of the torch backend's extra outputs ``normal`` and ``pos`` (diffrend/torch/renderer.py:
185-189, 342-355), beside oracle/torch_oracle.render_tch's image and depth, for the gradients of losses on all four.

At a hit pixel with winner m:  normal = n^ = n / sqrt(|n|^2 + 3e-10) (sphere: p - c likewise), NOT flipped by
double_sided (which flips only inside the shading);  pos = origin + t d (per-pixel origin for orthographic cameras).
Misses: both are 0 and their upstream gradients are ignored (the reference differentiates object 0's intersection
there; the hip backend does not -- the one deliberate difference).  The geometry is torch_oracle.render_tch's, term
for term; the winners come from oracle/np_oracle_tch.  Pinned to the reference by tests/test_aux_grad_golden_cpu.py
(tests/golden/n1_*.npz, tools/gen_golden_aux_grad.py)."""
from typing import Any, Dict, Optional

import numpy as np
import torch

from oracle import np_oracle_tch, torch_oracle


def render_aux(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], ref: Optional[Dict[str, np.ndarray]] = None,
               double_sided: bool = False, use_quartic: bool = False):
    """Differentiable normal (H,W,3), pos (H,W,3) and the hit mask (H,W), zeros at misses."""
    cam = scene["camera"]
    if np_oracle_tch.is_ortho(cam):
        _, orig_np, dvec, H, W = np_oracle_tch.generate_rays_ortho(cam)
        orig = torch.tensor(np.ascontiguousarray(orig_np))
        d = torch.tensor(np.broadcast_to(dvec[None, :], orig_np.shape).copy())
    else:
        eye_np, ray_np, H, W = np_oracle_tch.generate_rays(cam)
        d = torch.tensor(ray_np.T.copy())
        orig = torch.tensor(eye_np[:3])[None, :].expand(d.shape[0], 3)
    if ref is None:
        ref = np_oracle_tch.render(scene, double_sided=double_sided, use_quartic=use_quartic)
    nearest = np.asarray(ref["nearest"]).reshape(-1)
    hit_np = np.asarray(ref["depth"]).reshape(-1) <= cam["far"]
    npix = H * W
    t = torch.zeros(npix, dtype=torch.float64)
    nrm = torch.zeros((npix, 3), dtype=torch.float64)
    start = 0
    for kind, grp in scene["objects"].items():
        count = (grp["face"] if kind == "triangle" else grp["pos"]).shape[0]
        sel = np.nonzero(hit_np & (nearest >= start) & (nearest < start + count))[0]
        if sel.size:
            loc = torch.as_tensor(nearest[sel] - start)
            ds = d[sel]
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
                ts = torch.where(t1 >= 0, t1, t2)
                n = torch_oracle._unit3_eps(orig[sel] + ts[:, None] * ds - c)
            else:
                q = (leaves["triangle.face"][loc][:, 0, :3] if kind == "triangle" else leaves[f"{kind}.pos"][loc][:, :3])
                n = torch_oracle._unit3_eps(leaves[f"{kind}.normal"][loc][:, :3])
                ts = torch.sum(n * (q - orig[sel]), dim=-1) / torch.sum(n * ds, dim=-1)
            t = t.index_put((torch.as_tensor(sel),), ts)
            nrm = nrm.index_put((torch.as_tensor(sel),), n)
        start += count
    hit = torch.as_tensor(hit_np)
    pos = torch.where(hit[:, None], orig + t[:, None] * d, torch.zeros_like(nrm))
    return nrm.reshape(H, W, 3), pos.reshape(H, W, 3), hit.reshape(H, W)


def gradients_aux(scene: Dict[str, Any], grad_image: Optional[np.ndarray] = None,
                  grad_depth: Optional[np.ndarray] = None, grad_normal: Optional[np.ndarray] = None,
                  grad_pos: Optional[np.ndarray] = None, ref: Optional[Dict[str, np.ndarray]] = None,
                  double_sided: bool = False, use_quartic: bool = False,
                  visibility: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """d loss / d leaf for loss = sum image g_i + sum_hit (depth g_d + normal . g_n + pos . g_p); None terms are left
    out.  Keys and shapes as torch_oracle.gradients_tch."""
    if ref is None:
        ref = np_oracle_tch.render(scene, double_sided=double_sided, use_quartic=use_quartic)
    leaves = torch_oracle.make_leaves_tch(scene)
    loss = torch.zeros((), dtype=torch.float64)
    if grad_image is not None or grad_depth is not None:
        image, depth, hit = torch_oracle.render_tch(scene, leaves, ref, double_sided, use_quartic, visibility)
        if grad_image is not None:
            loss = loss + torch.sum(image * torch.as_tensor(grad_image))
        if grad_depth is not None:
            gd = torch.as_tensor(grad_depth)
            loss = loss + torch.sum(torch.where(hit, depth * gd, torch.zeros_like(gd)))
    if grad_normal is not None or grad_pos is not None:
        normal, pos, hit = render_aux(scene, leaves, ref, double_sided, use_quartic)
        for out, g in ((normal, grad_normal), (pos, grad_pos)):
            if g is not None:
                loss = loss + torch.sum(torch.where(hit[..., None], out * torch.as_tensor(g), torch.zeros_like(out)))
    if loss.requires_grad:
        loss.backward()
    return {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in leaves.items()}
