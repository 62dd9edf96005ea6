"""fp64 autograd restatement of the reference's NDC splat renderer, render_splats_NDC (diffrend/torch/renderer.py:
358-474): one splat per pixel, given by its position in normalised device coordinates and a normal.

One view, W x H pixels, N = W H splats in row-major order, aspect = W / H (true division):
    un-projection  m00 = 1 / (aspect tan(fovy / 2)), m11 = 1 / tan(fovy / 2), m22 = (near + far) / (far - near),
                   m23 = -2 near far / (far - near);  q = (x / m00, y / m11, -w, (z - m22 w) / m23),  P = q.xyz / q.w
                   (w = 1 for three-column positions; every column is differentiable)
    depth          |P|
    normal         the given normals' first three columns, as they are: neither transformed nor normalised
    lights         camera coordinates through the inverse of the lookat basis R = [x y z]: R^-1 (l_xyz - l_w eye)
    shading        the torch backend's Phong (fragment_shader) with the view direction -P NOT normalised; double_sided:
                   sgn = sign(view . n), a constant, multiplies the diffuse and the specular dot before their relus; a
                   light at the fragment and a zero attenuation denominator divide by 1; the ambient term once per
                   light; relu over the light sum; no near / far mask, no tonemap
    norm_depth_image_only   image = (d' - min d) / (max d - min d) with d' = min d where d >= far; pos the homogeneous
                   [N, 4] after the divide; normal the input untouched
Written in this project's own terms; pinned to the reference by tests/test_splats_ndc_oracle_cpu.py
(tests/golden/splats_ndc/sn1_*.npz, tools/gen_splats_ndc_golden.py)."""
import json
from typing import Any, Dict

import numpy as np
import torch

from splat_oracle import camera_basis

LEAVES = ("disk.pos", "disk.normal", "lights.pos", "colors", "lights.attenuation", "lights.ambient",
          "materials.albedo", "materials.coeffs")
OUTPUTS = ("image", "depth", "normal", "pos")
WRITTEN = ("disk.pos", "disk.normal")                     # gradients the backward kernel writes; the others are atomic sums


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def _index(x, dev) -> torch.Tensor:
    if isinstance(x, torch.Tensor):                        # stays on its device: no host round trip per call
        return x.to(device=dev, dtype=torch.int64)
    return torch.as_tensor(np.asarray(x, dtype=np.int64), device=dev)


def grid(camera: Dict[str, Any]):
    vp = [int(v) for v in np.asarray(_np(camera["viewport"])).reshape(-1)]
    return vp[2] - vp[0], vp[3] - vp[1]


def unprojection(camera: Dict[str, Any]):
    """(m00, m11, m22, m23) of the camera dict."""
    W, H = grid(camera)
    t = np.tan(float(camera["fovy"]) / 2.0)
    near, far = float(camera["near"]), float(camera["far"])
    return 1.0 / ((W / H) * t), 1.0 / t, (near + far) / (far - near), -2.0 * near * far / (far - near)


def render(scene: Dict[str, Any], leaves: Dict[str, torch.Tensor], double_sided: bool = False, use_quartic: bool = False,
           norm_depth_image_only: bool = False, _probe: Dict[str, Any] = None, **_ignored) -> Dict[str, torch.Tensor]:
    """The reference's outputs for one view, differentiable in `leaves` (tensors named as LEAVES; fp64 on the CPU in the
    tests, fp32 on the GPU in tools/bench_splats_ndc.py).  `_probe` (decisions) receives every decision quantity."""
    cam = scene["camera"]
    W, H = grid(cam)
    m00, m11, m22, m23 = unprojection(cam)
    pos_in, nrm_in = leaves["disk.pos"], leaves["disk.normal"]
    dt, dev = pos_in.dtype, pos_in.device
    x, y, z = pos_in[:, 0], pos_in[:, 1], pos_in[:, 2]
    w = pos_in[:, 3] if pos_in.shape[1] == 4 else torch.ones_like(z)
    q3 = (z - m22 * w) / m23
    P = torch.stack((x / m00, y / m11, -w), dim=-1) / q3[:, None]           # (N, 3)
    depth = torch.sqrt(torch.sum(P * P, dim=-1))
    if norm_depth_image_only:
        far = float(cam["far"])
        mn = torch.min(depth)
        # the reference selects with a float32 mask, m * min + (1 - m) * d: in float32 that is the plain selection; run in
        # float64, torch's promotion rules round the product of the mask and the 0-dim minimum to float32, so where
        # d >= far the recorded float64 image is (fp32(min) - min) / (max - min), about 1e-8, not 0.  Restated as it
        # is, so that the comparison with the float64 recording holds at 1e-9; the GPU path gives the 0 of float32
        far_mask = (depth >= far).to(torch.float32)
        nd = far_mask * mn + (1 - far_mask) * depth
        if _probe is not None:
            _probe["depth - far"] = depth - far
        return {"image": ((nd - mn) / (torch.max(depth) - mn)).view(H, W), "depth": depth.view(H, W),
                "pos": torch.cat((P, (q3 / q3)[:, None]), dim=1), "normal": nrm_in}
    n = nrm_in[:, :3]
    R, eye = camera_basis(_np(cam["eye"]), _np(cam["at"]), _np(cam["up"]))
    # the reference INVERTS its 4x4 inverse-lookat matrix: R^-1 (l - w eye).  R's columns are unit only up to the 1e-10
    # of their normalisation, so R^-1 and the R^T of the kernels differ by about that much -- visible at this file's
    # 1e-9 through a specular exponent of 12, far below the fp32 stores of the GPU comparison
    Rinv, eye = torch.linalg.inv(R).to(dtype=dt, device=dev), eye.to(dtype=dt, device=dev)
    lp = leaves["lights.pos"]
    lcc = (lp[:, :3] - lp[:, 3:4] * eye) @ Rinv.T                          # one row per light
    cidx = _index(scene["lights"]["color_idx"], dev)
    mat = scene["objects"]["disk"].get("material_idx")
    mat = _index(mat, dev) if mat is not None else torch.zeros((H * W,), dtype=torch.int64, device=dev)
    colors, att, amb = leaves["colors"][cidx], leaves["lights.attenuation"], leaves["lights.ambient"]
    alb, cf = leaves["materials.albedo"][mat], leaves["materials.coeffs"][mat]
    cdir = -P
    cdotn = torch.sum(cdir * n, dim=-1)
    sgn = torch.sign(cdotn).detach() if double_sided else torch.ones_like(cdotn)
    im = torch.zeros((H * W, 3), dtype=dt, device=dev)
    for l in range(lp.shape[0]):
        v = lcc[l] - P
        dist = torch.sqrt(torch.sum(v * v, dim=-1))
        lh = v / torch.where(dist > 0, dist, torch.ones_like(dist))[:, None]
        den = att[l, 0] + dist * att[l, 1] + dist ** (4 if use_quartic else 2) * att[l, 2]
        afac = 1.0 / torch.where(den.abs() > 0, den, torch.ones_like(den))
        ldn = torch.sum(lh * n, dim=-1)
        diffuse = sgn * (afac * ldn)
        specular = sgn * torch.sum(cdir * (2 * ldn[:, None] * n - lh), dim=-1)
        wgt = cf[:, 0] * torch.relu(diffuse) + cf[:, 1] * torch.relu(specular) ** cf[:, 2]
        im = im + wgt[:, None] * colors[l] * alb + amb * alb
        if _probe is not None:
            _probe.setdefault("diffuse", []).append(diffuse)
            _probe.setdefault("specular", []).append(specular)
    if _probe is not None:
        _probe["light sum"] = im
        if double_sided:
            _probe["cam_dir . n"] = cdotn
    return {"image": torch.relu(im).view(H, W, 3), "depth": depth.view(H, W), "pos": P.view(H, W, 3),
            "normal": n.reshape(H, W, 3)}


def make_leaves(scene: Dict[str, Any], requires_grad: bool = True) -> Dict[str, torch.Tensor]:
    """fp64 leaves for every differentiable input of the scene dict."""
    disk, lights = scene["objects"]["disk"], scene["lights"]
    src = {"disk.pos": disk["pos"], "disk.normal": disk["normal"], "lights.pos": lights["pos"], "colors": scene["colors"],
           "lights.attenuation": lights["attenuation"], "lights.ambient": lights["ambient"],
           "materials.albedo": scene["materials"]["albedo"], "materials.coeffs": scene["materials"]["coeffs"]}
    return {k: torch.tensor(np.asarray(_np(v), dtype=np.float64), requires_grad=requires_grad) for k, v in src.items()}


def gradients(scene: Dict[str, Any], upstream: Dict[str, np.ndarray], **params):
    """(outputs, {leaf: d loss / d leaf}) for loss = sum over outputs o of sum(o * upstream[o]); a leaf the loss does not
    depend on gets zeros."""
    leaves = make_leaves(scene)
    out = render(scene, leaves, **params)
    loss = sum(torch.sum(out[k] * torch.as_tensor(np.asarray(g, dtype=np.float64))) for k, g in upstream.items())
    loss.backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}
    return {k: v.detach().numpy() for k, v in out.items()}, grads


def decisions(scene: Dict[str, Any], **params) -> Dict[str, np.ndarray]:
    """{name: values} of every decision quantity of one view: 'diffuse' and 'specular' (N, L: the arguments of the two
    relus), 'light sum' (N, 3: the argument of the last relu), 'cam_dir . n' (N) under double_sided, 'depth - far' (N)
    under norm_depth_image_only."""
    probe = {}
    render(scene, make_leaves(scene, requires_grad=False), _probe=probe, **params)
    return {k: (torch.stack(v, dim=-1) if isinstance(v, list) else v).numpy() for k, v in probe.items()}


def view(scene: Dict[str, Any], b: int) -> Dict[str, Any]:
    """View b of a batched scene dict (a leading axis on disk.pos, and optionally on disk.normal, camera.eye and
    lights.pos) as a single-view scene."""
    disk, cam, lights = scene["objects"]["disk"], scene["camera"], scene["lights"]
    out = dict(scene)
    out["objects"] = {"disk": dict(disk, pos=disk["pos"][b],
                                   normal=disk["normal"][b] if np.ndim(disk["normal"]) == 3 else disk["normal"])}
    out["camera"] = dict(cam, eye=cam["eye"][b] if np.ndim(cam["eye"]) == 2 else cam["eye"])
    out["lights"] = dict(lights, pos=lights["pos"][b] if np.ndim(lights["pos"]) == 3 else lights["pos"])
    return out


def n_views(scene: Dict[str, Any]) -> int:
    """0 for a single-view scene, else B."""
    p = scene["objects"]["disk"]["pos"]
    return p.shape[0] if np.ndim(p) == 3 else 0


def batch_gradients(scene: Dict[str, Any], upstream: Dict[str, np.ndarray], **params):
    """gradients() for a scene that may be batched, in the batch's layout: outputs and the leaves that carry the view
    axis stacked, a shared leaf's gradient summed over the views."""
    B = n_views(scene)
    if not B:
        return gradients(scene, upstream, **params)
    runs = [gradients(view(scene, b), {k: g[b] for k, g in upstream.items()}, **params) for b in range(B)]
    outs = {k: np.stack([r[0][k] for r in runs]) for k in runs[0][0]}
    per_view = {"disk.pos": True, "disk.normal": np.ndim(scene["objects"]["disk"]["normal"]) == 3,
                "lights.pos": np.ndim(scene["lights"]["pos"]) == 3}
    grads = {k: (np.stack([r[1][k] for r in runs]) if per_view.get(k) else sum(r[1][k] for r in runs)) for k in LEAVES}
    return outs, grads


# --- golden files (tests/golden/splats_ndc/sn1_*.npz) ------------------------------------------------------------------
_CAMERA = ("eye", "at", "up", "viewport", "fovy", "near", "far")
_ARRAYS = {"lights.pos": ("lights", "pos"), "lights.color_idx": ("lights", "color_idx"),
           "lights.attenuation": ("lights", "attenuation"), "lights.ambient": ("lights", "ambient"),
           "colors": (None, "colors"), "materials.albedo": ("materials", "albedo"),
           "materials.coeffs": ("materials", "coeffs"), "disk.pos": ("disk", "pos"), "disk.normal": ("disk", "normal"),
           "disk.material_idx": ("disk", "material_idx")}


def pack(scene: Dict[str, Any]) -> Dict[str, np.ndarray]:
    out = {"in/camera." + k: np.asarray(scene["camera"][k]) for k in _CAMERA}
    for key, (grp, name) in _ARRAYS.items():
        d = scene if grp is None else (scene["objects"]["disk"] if grp == "disk" else scene[grp])
        out["in/" + key] = np.asarray(_np(d[name]))
    return out


def unpack(npz) -> Dict[str, Any]:
    """A scene dict of numpy arrays (camera scalars as Python floats) from an sn1_ golden file."""
    cam = {}
    for k in _CAMERA:
        v = np.asarray(npz["in/camera." + k])
        cam[k] = float(v) if v.ndim == 0 else v
    cam["viewport"] = [int(v) for v in cam["viewport"]]
    scene = {"camera": cam, "lights": {}, "materials": {}, "objects": {"disk": {}}}
    for key, (grp, name) in _ARRAYS.items():
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
