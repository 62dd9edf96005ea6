"""fp64 autograd restatement of the reference's splat renderer, render_splats_along_ray (diffrend/torch/renderer.py:
537-751): per-pixel shading of one splat per pixel, given by its camera-space depth, with no intersection.

One view, W x H base pixels, f = focal_length, h = 2 f tan(fovy / 2), w = h W / H:
    grid       x_j = linspace(-1, 1, W)_j w / 2,  y_i = linspace(1, -1, H)_i h / 2   (float32 values, as the reference's)
    position   Z = -relu(-z),  P = (-Z x / f, -Z y / f, Z)
    normals    given ([:, :3], as is), or the plane fit over the 3x3 stencil of P with reflection at the borders:
               u_k = d_k / sqrt(|d_k|^2 + 3e-10) for the 8 neighbour differences, (nx, ny) = (M^T M)^-1 M^T (-u_z) with
               the adjugate over det + 1e-12, n = (nx, ny, 1) / sqrt(nx^2 + ny^2 + 1 + 3e-10)
    samples K  sub-ray r = unit((x + sx dx / 2, y + sy dy / 2, -f)), sx = linspace(-1, 1, K)_c, sy = linspace(1, -1, K)_r,
               dx = w / (K W - 1), dy = h / (K H - 1); pos = (P.n / r.n) r; the sub-pixel (c, r) of base pixel (i, j)
               lands at output (i K + c, j K + r) (the reference's reshape_upsampled_data order)
    shading    the torch backend's Phong (fragment_shader) with double_sided off, lights in camera coordinates through
               the orthonormal lookat basis, light_vis multiplying colour x albedo, relu over the light sum
Written in this project's own terms; pinned to the reference by tests/test_splat_oracle_cpu.py
(tests/golden/p1_*.npz, oracle/golden_p1.py)."""
import json
from typing import Any, Dict

import numpy as np
import torch

LEAVES = ("disk.pos", "disk.normal", "disk.light_vis", "lights.pos", "colors", "lights.attenuation",
          "lights.ambient", "materials.albedo", "materials.coeffs")
OUTPUTS = ("image", "depth", "normal", "pos")


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def _unit(v: torch.Tensor, eps: float = 1e-10) -> torch.Tensor:
    return v / torch.sqrt(torch.sum(v * v + eps, dim=-1, keepdim=True))


def grid(camera: Dict[str, Any]):
    """(x (W,), y (H,), f, w, h, W, H) of a camera dict: x, y in float64 holding float32 values."""
    vp = [int(v) for v in np.asarray(camera["viewport"]).reshape(-1)]
    W, H = vp[2] - vp[0], vp[3] - vp[1]
    f = float(camera["focal_length"])
    h = np.tan(float(camera["fovy"]) / 2) * 2 * f
    w = h * (W / H)
    x = (np.linspace(-1, 1, W) * (w / 2)).astype(np.float32).astype(np.float64)
    y = (np.linspace(1, -1, H) * (h / 2)).astype(np.float32).astype(np.float64)
    return x, y, f, w, h, W, H


def camera_basis(eye, at, up) -> torch.Tensor:
    """R = [x y z] (columns) of the reference's torch lookat: z = unit(eye - at), x = unit(unit(up) x z), y = z x x."""
    e, a, u = (torch.as_tensor(np.asarray(v, dtype=np.float64).reshape(-1)[:3]) for v in (eye, at, up))
    z = _unit(e - a)
    x = _unit(torch.cross(_unit(u), z, dim=0))
    y = torch.cross(z, x, dim=0)
    return torch.stack((x, y, z), dim=1), e


def plane_fit_normals(P: torch.Tensor) -> torch.Tensor:
    """(H, W, 3) camera-space points -> (H, W, 3) unit normals with nz > 0 (3x3 reflected stencil)."""
    H, W = P.shape[:2]
    ri = torch.arange(-1, H + 1, device=P.device).abs()
    ri = torch.where(ri > H - 1, 2 * (H - 1) - ri, ri)
    ci = torch.arange(-1, W + 1, device=P.device).abs()
    ci = torch.where(ci > W - 1, 2 * (W - 1) - ci, ci)
    Pp = P[ri][:, ci]
    d = [Pp[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] - P for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
    u = _unit(torch.stack(d, dim=0))                         # (8, H, W, 3)
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    a, b, dd = torch.sum(ux * ux, 0), torch.sum(ux * uy, 0), torch.sum(uy * uy, 0)
    r0, r1 = -torch.sum(ux * uz, 0), -torch.sum(uy * uz, 0)
    det = a * dd - b * b + 1e-12
    nx = (dd * r0 - b * r1) / det
    ny = (a * r1 - b * r0) / det
    return _unit(torch.stack((nx, ny, torch.ones_like(nx)), dim=-1))


def render(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], samples: int = 1, use_quartic: bool = False,
           norm_depth_image_only: bool = False, _copies: Dict[str, torch.Tensor] = None, _probe: Dict[str, Any] = None,
           **_ignored) -> Dict[str, torch.Tensor]:
    """The reference's outputs for one view, in fp64, differentiable in `leaves` (fp64 tensors named as LEAVES).
    `_copies` (gradient_terms) replaces shading leaves by one copy per pixel, the arithmetic unchanged: lights.pos
    (KH, KW, L, 4), colors (KH, KW, L, 3: the lights' rows), lights.attenuation (KH, KW, L, 3) per output pixel and light;
    lights.ambient, materials.albedo, materials.coeffs (H, W, 3: the splat's row) per base pixel; disk.light_vis (L, KH, KW)
    per sub-pixel.  `_probe` (decision_margin) receives the argument of every relu."""
    cp = _copies or {}
    cam = scene["camera"]
    x, y, f, w, h, W, H = grid(cam)
    K = int(samples)
    pos_in = leaves["disk.pos"]
    dt, dev = pos_in.dtype, pos_in.device                    # fp64 on the CPU here; tools/bench_splats.py runs fp32 GPU
    z = pos_in if pos_in.dim() == 1 else pos_in[:, 2]
    Z = -torch.relu(-z).view(H, W)
    X = torch.as_tensor(x, dtype=dt, device=dev)[None, :]
    Y = torch.as_tensor(y, dtype=dt, device=dev)[:, None]
    P = torch.stack((-Z * X / f, -Z * Y / f, Z), dim=-1)     # (H, W, 3)
    N = leaves["disk.normal"][:, :3].reshape(H, W, 3) if "disk.normal" in leaves else plane_fit_normals(P)
    vis = leaves.get("disk.light_vis")
    vis = vis.reshape(vis.shape[0], H, W) if vis is not None else None
    mat = scene["objects"]["disk"].get("material_idx")
    mat = torch.as_tensor(np.asarray(_np(mat), dtype=np.int64), device=dev).view(H, W) if mat is not None else \
        torch.zeros((H, W), dtype=torch.int64, device=dev)
    if _probe is not None:
        _probe["-z"] = -z

    def up(a):
        return a.repeat_interleave(K, 0).repeat_interleave(K, 1) if K > 1 else a
    if K > 1:
        dx, dy = w / (K * W - 1), h / (K * H - 1)
        d0 = torch.sum(P * N, dim=-1)
        rows = []
        for c, sx in enumerate(np.linspace(-1, 1, K)):
            cols = []
            for r, sy in enumerate(np.linspace(1, -1, K)):
                ray = torch.stack(torch.broadcast_tensors(X + sx * dx / 2, Y + sy * dy / 2,
                                                          torch.full((1, 1), -f, dtype=dt, device=dev)), dim=-1)
                ray = _unit(ray)
                t = d0 / torch.sum(ray * N, dim=-1)
                cols.append(t[..., None] * ray)                # (H, W, 3) for sub-pixel (c, r)
            rows.append(torch.stack(cols, dim=2))             # (H, W, K_r, 3)
        pos = torch.stack(rows, dim=1).reshape(H * K, W * K, 3)        # (H, K_c, W, K_r, 3)
        N, mat = up(N), up(mat)
        vis = up(vis.permute(1, 2, 0)).permute(2, 0, 1) if vis is not None else None
        H, W = H * K, W * K
    else:
        pos = P
    depth = torch.sqrt(torch.sum(pos * pos, dim=-1))
    if norm_depth_image_only:
        mn = torch.min(depth)
        nd = torch.where(depth >= float(cam["far"]), mn, depth)
        return {"image": (nd - mn) / (torch.max(depth) - mn), "depth": depth, "pos": pos.reshape(-1, 3),
                "normal": N.reshape(-1, 3)}
    R, eye = camera_basis(_np(cam["eye"]), _np(cam["at"]), _np(cam["up"]))
    R, eye = R.to(dtype=dt, device=dev), eye.to(dtype=dt, device=dev)
    lp = cp.get("lights.pos", leaves["lights.pos"])
    lcc = (lp[..., :3] - lp[..., 3:4] * eye) @ R                 # R^T (l - w eye), one row per light
    cidx = torch.as_tensor(np.asarray(_np(scene["lights"]["color_idx"]), dtype=np.int64), device=dev)
    colors = cp["colors"] if "colors" in cp else leaves["colors"][cidx]
    att = cp.get("lights.attenuation", leaves["lights.attenuation"])
    alb = up(cp["materials.albedo"]) if "materials.albedo" in cp else leaves["materials.albedo"][mat]
    cf = up(cp["materials.coeffs"]) if "materials.coeffs" in cp else leaves["materials.coeffs"][mat]
    amb = up(cp["lights.ambient"]) if "lights.ambient" in cp else leaves["lights.ambient"]
    vis = cp.get("disk.light_vis", vis)
    cdir = -_unit(pos)
    im = torch.zeros((H, W, 3), dtype=dt, device=dev)
    for l in range(lp.shape[-2]):
        v = lcc[..., l, :] - pos
        dist = torch.sqrt(torch.sum(v * v, dim=-1))
        lh = v / torch.where(dist > 0, dist, torch.ones_like(dist))[..., None]
        den = att[..., l, 0] + dist * att[..., l, 1] + dist ** (4 if use_quartic else 2) * att[..., l, 2]
        afac = 1.0 / torch.where(den.abs() > 0, den, torch.ones_like(den))
        ldn = torch.sum(lh * N, dim=-1)
        nd = torch.relu(afac * ldn)
        refl = 2 * ldn[..., None] * N - lh
        rdot = torch.sum(cdir * refl, dim=-1)
        rd = torch.relu(rdot)
        wgt = cf[..., 0] * nd + cf[..., 1] * rd ** cf[..., 2]
        term = wgt[..., None] * colors[..., l, :] * alb
        if vis is not None:
            term = term * vis[l][..., None]
        im = im + term + amb * alb
        if _probe is not None:
            _probe.setdefault("afac * ldn", []).append(afac * ldn)
            _probe.setdefault("reflection", []).append(rdot)
            _probe.setdefault("den", []).append(den)
    if _probe is not None:
        _probe["light sum"] = im
    return {"image": torch.relu(im), "depth": depth, "pos": pos, "normal": N}


def make_leaves(scene: Dict[str, Any], requires_grad: bool = True) -> Dict[str, torch.Tensor]:
    """fp64 leaves for every differentiable input present in the scene dict."""
    disk, lights = scene["objects"]["disk"], scene["lights"]
    src = {"disk.pos": disk["pos"], "disk.normal": disk.get("normal"), "disk.light_vis": disk.get("light_vis"),
           "lights.pos": lights["pos"], "colors": scene["colors"], "lights.attenuation": lights["attenuation"],
           "lights.ambient": lights["ambient"], "materials.albedo": scene["materials"]["albedo"],
           "materials.coeffs": scene["materials"]["coeffs"]}
    out = {}
    for k, v in src.items():
        if v is None:
            continue
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v
        out[k] = torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=requires_grad)
    return out


def gradients(scene: Dict[str, Any], upstream: Dict[str, np.ndarray], **params):
    """(outputs, {leaf: d loss / d leaf}) for loss = sum over outputs o of sum(o * upstream[o])."""
    leaves = make_leaves(scene)
    out = render(scene, leaves, **params)
    loss = sum(torch.sum(out[k] * torch.as_tensor(np.asarray(g, dtype=np.float64))) for k, g in upstream.items())
    loss.backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}
    return {k: v.detach().numpy() for k, v in out.items()}, grads


def clamped_color_idx(scene: Dict[str, Any]) -> np.ndarray:
    """lights.color_idx as the kernels read it: clamped to the rows of `colors`."""
    return np.clip(np.asarray(_np(scene["lights"]["color_idx"]), dtype=np.int64), 0, len(_np(scene["colors"])) - 1)


def material_idx(scene: Dict[str, Any], n: int) -> np.ndarray:
    """objects.disk.material_idx as the kernels read it: (n,), clamped to the rows of materials.albedo, 0 if absent."""
    mat = scene["objects"]["disk"].get("material_idx")
    if mat is None:
        return np.zeros(n, dtype=np.int64)
    return np.clip(np.asarray(_np(mat), dtype=np.int64).reshape(-1), 0, len(_np(scene["materials"]["albedo"])) - 1)


def per_output_gradients(scene: Dict[str, Any], upstream: Dict[str, np.ndarray], **params):
    """{output: {leaf: d sum(output * upstream[output]) / d leaf}}: one backward pass per output of the loss."""
    return {k: gradients(scene, {k: g}, **params)[1] for k, g in upstream.items()}


def gradient_terms(scene: Dict[str, Any], upstream: Dict[str, np.ndarray], _raw: Dict[str, np.ndarray] = None, **params):
    """(total, absolute) per leaf: `total` is what gradients() returns; `absolute` the sum of the |terms| that
    k_splat_bwd (csrc/srh_splat.h) adds in fp32 on the way to the entry, in the kernel's own grouping:
      lights.pos[l], lights.attenuation[l], colors[color_idx[l]]   one term per (output pixel, light): wave_add sits inside
                                                                   the sub-pixel and the light loop; a colour row shared by
                                                                   several lights takes the terms of each of them
      lights.ambient, materials.albedo[m], materials.coeffs[m]     one term per base pixel (sub-pixels and lights are summed
                                                                   in fp64 registers first)
      disk.light_vis[l, n]                                         one term per sub-pixel of splat n (written once at K = 1,
                                                                   an fp32 read-modify-write chain over K^2 at K > 1)
      disk.pos, disk.normal                                        written once from fp64: the |gradient| per output of the
                                                                   loss (image, depth, normal, pos), added -- within one
                                                                   output the paths may cancel, between them they need not
    All terms of the shading leaves come from ONE backward pass over per-pixel copies of the leaves (render's _copies);
    disk.pos and disk.normal take one more pass per output (per_output_gradients), a non-finite entry of which (the
    oracle's sqrt'(0) * 0 through the depth of an origin splat) counts as 0.  `_raw` receives the copies' gradients."""
    leaves = make_leaves(scene)
    x, y, f, w, h, W, H = grid(scene["camera"])
    K = int(params.get("samples", 1))
    KH, KW = K * H, K * W
    L = leaves["lights.pos"].shape[0]
    cidx, mat = clamped_color_idx(scene), material_idx(scene, H * W)
    shade = not params.get("norm_depth_image_only", False)

    def copies(t, *lead):
        return t.detach().expand(*lead, *t.shape).clone().requires_grad_(True)
    cp = {}
    if shade:
        cp = {"lights.pos": copies(leaves["lights.pos"], KH, KW),
              "lights.attenuation": copies(leaves["lights.attenuation"], KH, KW),
              "colors": copies(leaves["colors"].detach()[torch.as_tensor(cidx)], KH, KW),
              "lights.ambient": copies(leaves["lights.ambient"], H, W),
              "materials.albedo": leaves["materials.albedo"].detach()[torch.as_tensor(mat)].view(H, W, 3).clone().requires_grad_(True),
              "materials.coeffs": leaves["materials.coeffs"].detach()[torch.as_tensor(mat)].view(H, W, 3).clone().requires_grad_(True)}
        if "disk.light_vis" in leaves:
            v = leaves["disk.light_vis"].detach().view(L, H, W)
            cp["disk.light_vis"] = v.repeat_interleave(K, 1).repeat_interleave(K, 2).clone().requires_grad_(True)
    out = render(scene, leaves, _copies=cp, **params)
    loss = sum(torch.sum(out[k] * torch.as_tensor(np.asarray(g, dtype=np.float64))) for k, g in upstream.items())
    loss.backward()
    g = {k: (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in cp.items()}
    if _raw is not None:
        _raw.update(g)
    total, absolute = {}, {}
    for k in ("disk.pos", "disk.normal"):
        if k in leaves:
            t = leaves[k]
            total[k] = t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))
    parts = per_output_gradients(scene, upstream, **params)
    for k in total:
        absolute[k] = sum(np.where(np.isfinite(p[k]), np.abs(p[k]), 0.0) for p in parts.values())
    for k, t in leaves.items():
        if k in total:
            continue
        shape = tuple(t.shape)
        total[k], absolute[k] = np.zeros(shape), np.zeros(shape)
        if k not in g:
            continue
        for fn, dst in ((lambda a: a, total[k]), (np.abs, absolute[k])):
            a = fn(g[k])
            if k in ("lights.pos", "lights.attenuation"):
                dst += a.sum(axis=(0, 1))
            elif k == "colors":
                np.add.at(dst, cidx, a.sum(axis=(0, 1)))
            elif k == "lights.ambient":
                dst += a.sum(axis=(0, 1))
            elif k in ("materials.albedo", "materials.coeffs"):
                np.add.at(dst, mat, a.reshape(H * W, 3))
            else:                                             # disk.light_vis: (L, KH, KW) -> the K x K block of a splat
                dst += a.reshape(L, H, K, W, K).sum(axis=(2, 4)).reshape(shape)
    return total, absolute


def light_vis_terms(scene: Dict[str, Any], upstream: Dict[str, np.ndarray], **params) -> np.ndarray:
    """(L, N, K^2): the terms of disk.light_vis[l, n] in the order k_splat_bwd adds them, sub = c K + r for the sub-pixel
    at output (i K + c, j K + r)."""
    raw = {}
    gradient_terms(scene, upstream, _raw=raw, **params)
    x, y, f, w, h, W, H = grid(scene["camera"])
    K = int(params.get("samples", 1))
    a = raw["disk.light_vis"]
    return a.reshape(a.shape[0], H, K, W, K).transpose(0, 1, 3, 2, 4).reshape(a.shape[0], H * W, K * K)


def decision_margin(scene: Dict[str, Any], **params):
    """{relu: (margin, zeros)} for every relu of the restatement -- '-z', 'afac * ldn' and 'reflection' (per light), 'light
    sum' (per channel) -- with margin the smallest non-zero |argument| over the largest, and zeros the sorted indices of
    the base splats at which an argument is exactly 0.  A comparison in fp64 on the GPU decides as the oracle does as long
    as the margin is far above the chains' rounding (1e-13 of the largest argument and less)."""
    probe = {}
    render(scene, make_leaves(scene, requires_grad=False), _probe=probe, **params)
    x, y, f, w, h, W, H = grid(scene["camera"])
    K = int(params.get("samples", 1))
    out = {}
    for name in ("-z", "afac * ldn", "reflection", "light sum"):
        if name not in probe:
            continue
        a = probe[name]
        a = (torch.stack(a, dim=-1) if isinstance(a, list) else a).numpy()
        if name == "-z":
            a = a.reshape(H, 1, W, 1, 1)
        else:
            a = a.reshape(H, K, W, K, -1)
        mag = np.abs(a)
        nonzero = mag[mag > 0]
        margin = float(nonzero.min() / mag.max()) if nonzero.size else np.inf
        zeros = np.where((mag == 0).any(axis=(1, 3, 4)).reshape(-1))[0]
        out[name] = (margin, zeros)
    return out


# --- golden files (tests/golden/p1_*.npz) ----------------------------------------------------------------------------
_CAMERA = ("eye", "at", "up", "viewport", "fovy", "focal_length", "far")
_ARRAYS = {"lights.pos": ("lights", "pos"), "lights.color_idx": ("lights", "color_idx"),
           "lights.attenuation": ("lights", "attenuation"), "lights.ambient": ("lights", "ambient"),
           "colors": (None, "colors"), "materials.albedo": ("materials", "albedo"),
           "materials.coeffs": ("materials", "coeffs"), "disk.pos": ("disk", "pos"), "disk.normal": ("disk", "normal"),
           "disk.light_vis": ("disk", "light_vis"), "disk.material_idx": ("disk", "material_idx")}


def pack(scene: Dict[str, Any]) -> Dict[str, np.ndarray]:
    out = {"in/camera." + k: np.asarray(scene["camera"][k]) for k in _CAMERA if k in scene["camera"]}
    for key, (grp, name) in _ARRAYS.items():
        d = scene if grp is None else (scene["objects"]["disk"] if grp == "disk" else scene[grp])
        if d.get(name) is not None:
            v = d[name]
            out["in/" + key] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return out


def unpack(npz) -> Dict[str, Any]:
    """A scene dict of numpy arrays (camera scalars as Python floats) from a p1_ golden file."""
    cam = {}
    for k in _CAMERA:
        if "in/camera." + k in npz.files:
            v = np.asarray(npz["in/camera." + k])
            cam[k] = float(v) if v.ndim == 0 else v
    cam["viewport"] = [int(v) for v in cam["viewport"]]
    scene = {"camera": cam, "lights": {}, "materials": {}, "objects": {"disk": {}}}
    for key, (grp, name) in _ARRAYS.items():
        if "in/" + key not in npz.files:
            continue
        v = np.asarray(npz["in/" + key])
        if grp is None:
            scene[name] = v
        elif grp == "disk":
            scene["objects"]["disk"][name] = v
        else:
            scene[grp][name] = v
    return scene


def kwargs_of(npz) -> Dict[str, Any]:
    return json.loads(str(npz["kwargs"]))
