"""A numpy fp64 restatement of surf_renderer_amd.mesh_sampling, one view at a time -- test infrastructure.  The forward
follows the reference's own order of operations (diffrend/utils/sample_generator.py:112-194, model.py:18-32,
numpy/ops.py:233-253), so that on inputs the reference accepts it reproduces the reference's samples
(tests/test_mesh_sampling_oracle_cpu.py pins it to recorded ones); the differentiable part is restated in torch float64
under autograd with `face` and `bary` held fixed.

  n      = c / |c|, c = np.cross(v1 - v0, v2 - v0), the divisor 1 where |c| = 0
  area2  = sqrt(d0^2 + d1^2 + d2^2), d* the 2 x 2 determinants of r = v0 - v2, s = v1 - v2 over the column pairs
           (1, 2), (2, 0), (0, 1)
  keep   = n . normalize(eye - v0) >= 0 (every face without an eye)
  weight = area2 where it is finite and positive and the face is kept, else 0
  cdf    = cumsum(weight / sum(weight)) / its last value           numpy's choice(p=...)
  face   = cdf.searchsorted(r0, side='right')
  bary   = (1 - q, (1 - t) q, t q), q = sqrt(s);  pos = sum_c bary_c v_c;  normal = n[face]
A view whose weights are all 0: face = -1, NaN pos, normal and bary, zero gradient.

With every value comes S, the sum of the absolute values of the terms of that entry's sum, which scales its rounding
bound."""
import numpy as np
import torch


def widen(a):
    """the float32 values of `a` in float64: what the kernels and the reference are both given"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def face_quantities(v, f, eye=None):
    """{normal [F, 3], area2 [F], keep [F] bool, weight [F], facing [F] or None, conditioning [F]} of one view"""
    v, f = widen(v), np.asarray(f, np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = v1 - v0, v2 - v0
        c = np.cross(e1, e2)
        length = np.sqrt(np.sum(c ** 2, axis=-1))
        denom = length[:, None].copy()
        denom[denom == 0] = 1
        n = c / denom
        r, s = v0 - v2, v1 - v2
        d0 = r[:, 1] * s[:, 2] - r[:, 2] * s[:, 1]
        d1 = r[:, 2] * s[:, 0] - r[:, 0] * s[:, 2]
        d2 = r[:, 0] * s[:, 1] - r[:, 1] * s[:, 0]
        area2 = np.sqrt(d0 ** 2 + d1 ** 2 + d2 ** 2)
        keep, facing = np.ones(len(f), bool), None
        if eye is not None:
            d = np.asarray(eye, np.float64) - v0
            dn = np.sqrt(np.sum(d ** 2, axis=-1))[:, None]
            cam_dir = np.where(dn != 0, d / np.where(dn != 0, dn, 1), 0.0)
            facing = np.sum(n * cam_dir, axis=-1)
            keep = facing >= 0
        ok = np.isfinite(area2) & (area2 > 0) & keep
        weight = np.where(ok, area2, 0.0)
        # sum of |product terms| of the cross product over |c|: how many bits the normal of a sliver loses
        a1, a2 = np.abs(e1), np.abs(e2)
        terms = np.stack([a1[:, 1] * a2[:, 2] + a1[:, 2] * a2[:, 1], a1[:, 2] * a2[:, 0] + a1[:, 0] * a2[:, 2],
                          a1[:, 0] * a2[:, 1] + a1[:, 1] * a2[:, 0]], axis=1)
        conditioning = np.sum(terms, axis=1) / np.where(length > 0, length, np.nan)
    return {"normal": n, "area2": area2, "keep": keep, "weight": weight, "facing": facing, "length": length,
            "normal_terms": terms, "conditioning": conditioning}


def cdf_numpy(weight):
    """numpy's choice(p=weight / sum(weight)): p.cumsum() over its last value"""
    p = weight / np.sum(weight)
    cdf = p.cumsum()
    return cdf / cdf[-1]


def cdf_plain(weight):
    """a plain left-to-right fp64 prefix sum over its total"""
    run = np.cumsum(weight)
    return run / run[-1]


def barycentric(uniforms):
    """(bary [S, 3], S_bary [S, 3]) of uniforms [S, 3] = (r0, s, t)"""
    s, t = uniforms[:, 1], uniforms[:, 2]
    q = np.sqrt(s)
    return (np.stack((1 - q, (1 - t) * q, t * q), axis=1),
            np.stack((1 + q, (1 + t) * q, t * q), axis=1))


def forward(v, f, uniforms, eye=None):
    """{face [S] int64, bary, pos, normal [S, 3] fp64, S_bary, S_pos, S_normal, quantities, cdf} of one view"""
    v, f, uniforms = widen(v), np.asarray(f, np.int64), np.asarray(uniforms, np.float64)
    q = face_quantities(v, f, eye)
    n_s = len(uniforms)
    if not (q["weight"] > 0).any():
        nan = np.full((n_s, 3), np.nan)
        return {"face": np.full(n_s, -1, np.int64), "bary": nan, "pos": nan, "normal": nan, "S_bary": nan, "S_pos": nan,
                "S_normal": nan, "quantities": q, "cdf": None}
    cdf = cdf_numpy(q["weight"])
    face = cdf.searchsorted(uniforms[:, 0], side="right").astype(np.int64)
    bary, s_bary = barycentric(uniforms)
    tri = v[f[face]]                                                  # [S, 3 corners, 3]
    pos = np.sum(bary[..., None] * tri, axis=1)
    s_pos = np.sum(np.abs(bary[..., None] * tri), axis=1)
    normal = q["normal"][face]
    with np.errstate(invalid="ignore"):                              # the non-finite faces, which are never chosen
        s_normal = (q["normal_terms"] / np.where(q["length"] > 0, q["length"], 1)[:, None])[face]
    return {"face": face, "bary": bary, "pos": pos, "normal": normal, "S_bary": s_bary, "S_pos": s_pos,
            "S_normal": s_normal, "quantities": q, "cdf": cdf}


def _abs_cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)


def gradients(v, f, face, bary, g_pos=None, g_normal=None):
    """{grad_v [V, 3], S_v [V, 3]} of one view for the loss sum(pos g_pos) + sum(normal g_normal) with `face` and `bary`
    held fixed; either upstream may be None = zero.  torch float64 autograd for the gradient; S by hand: per sample
    |b_c g_pos| for the point, and for the normal the absolute values along n = c / |c| and c = e1 x e2."""
    v, f = widen(v), np.asarray(f, np.int64)
    face = np.asarray(face, np.int64)
    grad, S = np.zeros_like(v), np.zeros_like(v)
    hit = face >= 0
    if not hit.any() or (g_pos is None and g_normal is None):
        return {"grad_v": grad, "S_v": S}
    face, bary = face[hit], np.asarray(bary, np.float64)[hit]
    corners = f[face]                                                 # [S, 3]
    vt = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    tri = vt[torch.tensor(corners)]                                   # [S, 3, 3]
    loss = torch.zeros((), dtype=torch.float64)                      # only the chosen faces' vertices enter it
    if g_pos is not None:
        g = np.asarray(g_pos, np.float64)[hit]
        loss = loss + ((torch.tensor(bary)[..., None] * tri).sum(1) * torch.tensor(g)).sum()
        for c in range(3):
            np.add.at(S, corners[:, c], np.abs(bary[:, c:c + 1] * g))
    if g_normal is not None:
        g = np.asarray(g_normal, np.float64)[hit]
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        c = torch.linalg.cross(e1, e2)
        length = torch.sqrt((c * c).sum(-1, keepdim=True))
        good = (length > 0) & torch.isfinite(length)
        n = torch.where(good, c / torch.where(good, length, torch.ones_like(length)), torch.zeros_like(c))
        loss = loss + (n * torch.tensor(g)).sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            tri_np = v[corners]
            a1, a2 = tri_np[:, 1] - tri_np[:, 0], tri_np[:, 2] - tri_np[:, 0]
            cn = np.cross(a1, a2)
            ln = np.sqrt(np.sum(cn ** 2, axis=-1, keepdims=True))
            ok = (ln > 0) & np.isfinite(ln)
            nn = np.where(ok, cn / np.where(ok, ln, 1), 0.0)
            s_dc = np.where(ok, (np.abs(g) + np.abs(nn) * np.sum(np.abs(nn * g), axis=-1, keepdims=True))
                            / np.where(ok, ln, 1), 0.0)
            s1, s2 = _abs_cross(np.abs(a2), s_dc), _abs_cross(s_dc, np.abs(a1))
        np.add.at(S, corners[:, 1], s1)
        np.add.at(S, corners[:, 2], s2)
        np.add.at(S, corners[:, 0], s1 + s2)
    loss.backward()
    return {"grad_v": vt.grad.numpy().copy(), "S_v": S}
