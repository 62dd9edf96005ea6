"""The project's own restatement of the reference's SH9 lighting (diffrend/numpy/sph.py:5-181) -- test infrastructure.

fp64 numpy for the values, in the reference's order of operations, with A = the sum of |terms| beside every sum: the
coefficients of order >= 1 of a non-negative probe cancel heavily, so an error is only meaningful relative to A.  The
same formulas in torch float64 give the gradients through CPU autograd (the reference has none); the A of a gradient
entry is the gradient's formula with every factor replaced by its absolute value.

One deliberate difference from the reference, which the layer documents: a pixel outside the disc is selected away,
not multiplied by 0, so a NaN there reaches nothing.  On finite probes the two are the same numbers
(tests/test_sh9_oracle_cpu.py holds this restatement to the reference's recorded values)."""
import numpy as np
import torch

C1, C2, C3, C4, C5 = 0.429043, 0.511664, 0.743125, 0.886227, 0.247708
# (r, s) -> (index into the nine coefficients, factor); mirrored to (s, r)
ZONAL = {(0, 0): (8, C1), (0, 1): (4, C1), (0, 2): (7, C1), (0, 3): (3, C2), (1, 1): (8, -C1), (1, 2): (5, C1),
         (1, 3): (1, C2), (2, 2): (6, C3), (2, 3): (2, C2)}


def real_sh9_cart(X, Y, Z, lib=np):
    s1, s3, s5, s15 = (np.sqrt(k / np.pi) for k in (1, 3, 5, 15))
    return lib.stack((1 / 2. * s1 * lib.ones_like(X), 1 / 2. * s3 * Y, 1 / 2. * s3 * Z, 1 / 2. * s3 * X,
                      1 / 2. * s15 * X * Y, 1 / 2. * s15 * Y * Z, 1 / 4. * s5 * (3 * Z ** 2 - 1), 1 / 2. * s15 * X * Z,
                      1 / 4. * s15 * (X ** 2 - Y ** 2)), -1)


def grid(H, W):
    """{theta, phi, inside, domega [H, W], Y [H, W, 9]} of the projection's pixel grid, rows scaled by W and columns by
    H as the reference scales them."""
    i, j = np.mgrid[0:H, 0:W]
    v = (W / 2.0 - i) / (W / 2.0)
    u = (j - H / 2.0) / (H / 2.0)
    r = np.sqrt(u ** 2 + v ** 2)
    theta, phi = np.pi * r, np.arctan2(v, u)
    domega = (2 * np.pi / W) * (2 * np.pi / H) * np.sinc(theta)
    X, Y, Z = np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)
    return {"theta": theta, "phi": phi, "inside": r <= 1.0, "domega": domega, "Y": real_sh9_cart(X, Y, Z)}


def project(envmap):
    """envmap [H, W, C] -> (L [C, 9], A [C, 9]): the pixels inside the disc, summed rows first as the reference sums."""
    envmap = np.asarray(envmap, np.float64)
    H, W, _ = envmap.shape
    g = grid(H, W)
    with np.errstate(invalid="ignore"):
        term = envmap[..., np.newaxis] * g["Y"][..., np.newaxis, :] * g["domega"][..., np.newaxis, np.newaxis]
    term = np.where(g["inside"][..., None, None], term, 0.0)
    return np.sum(np.sum(term, axis=0), axis=0), np.sum(np.abs(term), axis=(0, 1))


def project_grad(shape, g_L):
    """(grad_envmap, A) [H, W, C] of sum(L g_L): domega sum_k Y_k g_L[c][k] inside the disc, 0 outside."""
    H, W, _ = shape
    g = grid(H, W)
    term = g["Y"][..., None, :] * np.asarray(g_L, np.float64)[None, None] * g["domega"][..., None, None]
    term = np.where(g["inside"][..., None, None], term, 0.0)
    return term.sum(-1), np.abs(term).sum(-1)


def zonal_matrix(L, lib=np):
    """L [C, 9] -> M [4, 4, C], the reference's literals"""
    rows = [[None] * 4 for _ in range(4)]
    for (r, s), (k, w) in ZONAL.items():
        rows[r][s] = rows[s][r] = w * L[:, k]
    rows[3][3] = C4 * L[:, 0] - C5 * L[:, 6]
    return lib.stack([lib.stack(row, 0) for row in rows], 0)


def zonal_abs(L):
    """A of M's entries: |T| |L|, L [C, 9] -> [4, 4, C]"""
    L = np.abs(np.asarray(L, np.float64))
    M = np.abs(zonal_matrix(L))
    M[3, 3] = C4 * L[:, 0] + C5 * L[:, 6]
    return M


def zonal_abs_transpose(A_M):
    """A of L's gradient behind M's: |T|^T A_M, A_M [4, 4, C] -> [C, 9]"""
    out = np.zeros((A_M.shape[-1], 9))
    for (r, s), (k, w) in ZONAL.items():
        out[:, k] += abs(w) * (A_M[r, s] + (A_M[s, r] if r != s else 0.0))
    out[:, 0] += C4 * A_M[3, 3]
    out[:, 6] += C5 * A_M[3, 3]
    return out


def irradiance(M, normal, lib=np):
    """M [4, 4, C], normal [..., 3] -> E [..., C]: a = n M[:3, :] + M[3, :], E = a[:3] . n + a[3]"""
    out = []
    for ch in range(M.shape[-1]):
        a = lib.matmul(normal, M[:3, :, ch]) + M[3, :, ch]
        out.append((a[..., :3] * normal).sum(-1) + a[..., 3])
    return lib.stack(out, -1)


def irradiance_abs(M, normal):
    """A of E: every product of the quadratic form in absolute value"""
    return irradiance(np.abs(np.asarray(M, np.float64)), np.abs(np.asarray(normal, np.float64)))


def irradiance_view(M, normal, g_E=None):
    """One view, M [4, 4, C] and normal [N, 3] (their float32 values): {E, A_E} and, with an upstream gradient g_E [N, C],
    {grad_normal, A_normal [N, 3], grad_M, A_M [4, 4, C]} of sum(E g_E)."""
    M64, n64 = np.asarray(M, np.float64), np.asarray(normal, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = {"E": irradiance(M64, n64), "A_E": irradiance_abs(M64, n64)}
    if g_E is None:
        return out
    tM, tn = torch.tensor(M64, requires_grad=True), torch.tensor(n64, requires_grad=True)
    g = torch.tensor(np.asarray(g_E, np.float64))
    (irradiance(tM, tn, torch) * g).sum().backward()
    out["grad_M"], out["grad_normal"] = tM.grad.numpy(), tn.grad.numpy()
    aM, an, ag = np.abs(M64), np.abs(n64), np.abs(np.asarray(g_E, np.float64))
    h = np.concatenate([an, np.ones_like(an[:, :1])], axis=1)                       # |[n, 1]|
    out["A_M"] = np.einsum("nc,nr,ns->rsc", ag, h, h)
    sym = aM[:3, :3] + aM[:3, :3].transpose(1, 0, 2)                                # |M_rs| + |M_sr|
    out["A_normal"] = np.einsum("nc,rsc,ns->nr", ag, sym, an) + ag @ (aM[:3, 3] + aM[3, :3]).T
    return out


def chain_view(L, normal, g_E):
    """L [C, 9] -> M = zonal_matrix(L) rounded to float32 (what the kernels take) -> E -> sum(E g_E): {M, E, A_E, grad_L,
    A_L [C, 9], grad_normal, A_normal}.  The rounding is passed straight through: its derivative is taken as 1."""
    tL = torch.tensor(np.asarray(L, np.float64), requires_grad=True)
    M = zonal_matrix(tL, torch)
    M_used = M + (M.detach().float().double() - M.detach())
    tn = torch.tensor(np.asarray(normal, np.float64), requires_grad=True)
    (irradiance(M_used, tn, torch) * torch.tensor(np.asarray(g_E, np.float64))).sum().backward()
    view = irradiance_view(M_used.detach().numpy(), normal, g_E)
    return {"M": M_used.detach().numpy(), "E": view["E"], "A_E": view["A_E"], "grad_L": tL.grad.numpy(),
            "A_L": zonal_abs_transpose(view["A_M"]), "grad_normal": tn.grad.numpy(), "A_normal": view["A_normal"]}


def irrad_Z(L, dim):
    g = grid(*dim)
    X, Y, Z = np.cos(g["phi"]) * np.sin(g["theta"]), np.sin(g["phi"]) * np.sin(g["theta"]), np.cos(g["theta"])
    return irradiance(zonal_matrix(np.asarray(L, np.float64)), np.stack((X, Y, Z), axis=-1))


def reconstruct(L, dim):
    g = grid(*dim)
    L = np.asarray(L, np.float64)
    return np.sum(L[np.newaxis, np.newaxis, ...] * g["Y"][..., np.newaxis, :] * g["domega"][..., np.newaxis, np.newaxis],
                  axis=-1)


def load_lightprobe_bytes(raw, dim=None, endian="big", datatype="f4", flipud=True, clip_lb_thresh=0, normalize=True):
    """what the reference's loader makes of a file holding the bytes `raw`"""
    data = np.frombuffer(raw, dtype=("<" if endian == "big" else ">") + datatype)
    if dim is None:
        w = int(np.sqrt(data.size / 3))
        dim = (w, w, 3)
    data = data.reshape(dim)
    if flipud:
        data = data[::-1, ...]
    d = data[data > clip_lb_thresh]
    processed = (data - d.min()).astype(np.float64)
    if normalize:
        processed /= (d.max() - d.min())
    processed[processed < 0] = 0
    return data, processed
