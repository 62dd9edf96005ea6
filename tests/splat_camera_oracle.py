"""The two splat renderers' fp64 restatements with the camera's eye / at / up as leaves (tests/golden/splat_camera/
sc1_*.npz, tools/gen_splat_camera_golden.py).

tests/splat_oracle.py and tests/splats_ndc_oracle.py restate the renderers for a fixed camera: both take the view's
lookat basis from their module-level ``camera_basis(eye, at, up)``, on detached numpy values.  This module runs them
UNCHANGED with that one name pointing, for the duration of a call, at the same arithmetic on float64 leaf tensors, so
that autograd reaches eye, at and up: z = unit(eye - at), x = unit(unit(up) x z), y = z x x, unit(v) = v / sqrt(sum(v^2
+ 1e-10)) -- the reference's lookat.  A fourth component of a leaf is sliced off, so it gets 0.

The camera enters only through the lights' camera coordinates, so only the upstream gradient of `image` matters; the
fixtures hold that one alone."""
import contextlib
import json
from typing import Any, Dict

import numpy as np
import torch

import splat_oracle
import splats_ndc_oracle

KINDS = {"along_ray": splat_oracle, "ndc": splats_ndc_oracle}
CAMERA_LEAVES = ("camera.eye", "camera.at", "camera.up")


def camera_leaves(camera: Dict[str, Any]) -> Dict[str, torch.Tensor]:
    return {"camera." + k: torch.tensor(np.asarray(splat_oracle._np(camera[k]), dtype=np.float64), requires_grad=True)
            for k in ("eye", "at", "up")}


def basis(leaves: Dict[str, torch.Tensor]):
    """(R = [x y z] as columns, eye) of splat_oracle.camera_basis, differentiable in the camera leaves."""
    e, a, u = (leaves["camera." + k].reshape(-1)[:3] for k in ("eye", "at", "up"))
    z = splat_oracle._unit(e - a)
    x = splat_oracle._unit(torch.cross(splat_oracle._unit(u), z, dim=0))
    y = torch.cross(z, x, dim=0)
    return torch.stack((x, y, z), dim=1), e


@contextlib.contextmanager
def _attached(module, leaves):
    """The reference INVERTS its 4 x 4 inverse-lookat matrix, so the lights meet R^-1, which differs from R^T by about
    the 1e-10 of the normalisations.  splats_ndc_oracle inverts the basis itself; splat_oracle multiplies by R (= R^T
    from the right) and so is handed (R^-1)^T here -- through the camera's derivative the difference would reach 1e-8
    of the gradients, above the 1e-9 these restatements are pinned at."""
    saved = module.camera_basis

    def attached(*_):
        R, e = basis(leaves)
        return (torch.linalg.inv(R).T if module is splat_oracle else R), e
    module.camera_basis = attached
    try:
        yield
    finally:
        module.camera_basis = saved


def n_views(kind: str, scene: Dict[str, Any]) -> int:
    """0 for a single-view scene, else B."""
    p = np.asarray(scene["objects"]["disk"]["pos"])
    if kind == "ndc":                                     # [N, 3|4] or [B, N, 3|4]
        return p.shape[0] if p.ndim == 3 else 0
    vp = [int(v) for v in np.asarray(scene["camera"]["viewport"]).reshape(-1)]
    N = (vp[2] - vp[0]) * (vp[3] - vp[1])                 # [N] or [N, 3], or [B, N] or [B, N, 3]; the cases have N > 3
    return p.shape[0] if p.ndim >= 2 and p.shape[1] == N else 0


def view(kind: str, scene: Dict[str, Any], b: int) -> Dict[str, Any]:
    """View b of a batched scene dict as a single-view scene: disk.pos carries the view axis, disk.normal, disk.light_vis,
    camera.eye and lights.pos may."""
    disk, cam, lights = scene["objects"]["disk"], scene["camera"], scene["lights"]
    own = {"pos": disk["pos"][b]}
    for k, dims in (("normal", 2), ("light_vis", 2)):
        if disk.get(k) is not None:
            own[k] = disk[k][b] if np.ndim(disk[k]) == dims + 1 else disk[k]
    out = dict(scene)
    out["objects"] = {"disk": dict(disk, **own)}
    out["camera"] = dict(cam, eye=cam["eye"][b] if np.ndim(cam["eye"]) == 2 else cam["eye"])
    out["lights"] = dict(lights, pos=lights["pos"][b] if np.ndim(lights["pos"]) == 3 else lights["pos"])
    return out


def gradients(kind: str, scene: Dict[str, Any], g_image: np.ndarray, **params) -> Dict[str, np.ndarray]:
    """{leaf: d loss / d leaf} of one view for loss = sum(image * g_image), the camera leaves among them (zeros where
    the loss does not depend on a leaf)."""
    module = KINDS[kind]
    leaves = module.make_leaves(scene)
    leaves.update(camera_leaves(scene["camera"]))
    with _attached(module, leaves):
        out = module.render(scene, leaves, **params)
    torch.sum(out["image"] * torch.as_tensor(np.asarray(g_image, dtype=np.float64))).backward()
    return {k: (t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}


def batch_gradients(kind: str, scene: Dict[str, Any], g_image: np.ndarray, **params) -> Dict[str, np.ndarray]:
    """gradients() for a scene that may be batched: the camera leaves in the batch's layout -- a per-view eye [B, 3|4]
    gets its rows, a shared leaf the sum over the views; the other leaves per view, stacked."""
    B = n_views(kind, scene)
    if not B:
        return gradients(kind, scene, g_image, **params)
    runs = [gradients(kind, view(kind, scene, b), g_image[b], **params) for b in range(B)]
    out = {k: np.stack([r[k] for r in runs]) for k in runs[0] if k not in CAMERA_LEAVES}
    for k in CAMERA_LEAVES:
        per_view = np.ndim(scene["camera"][k.split(".")[1]]) == 2
        out[k] = np.stack([r[k] for r in runs]) if per_view else sum(r[k] for r in runs)
    return out


# --- golden files (tests/golden/splat_camera/sc1_*.npz) ----------------------------------------------------------------
def pack(kind: str, scene: Dict[str, Any]) -> Dict[str, np.ndarray]:
    return dict(KINDS[kind].pack(scene), kind=np.asarray(kind))


def load(path: str):
    """(kind, scene, kwargs, g_image, {precision: {leaf: gradient}}, meta) of a fixture."""
    z = np.load(path, allow_pickle=False)
    kind = str(z["kind"])
    grads = {p: {k: np.asarray(z[f"grad{p}/{k}"]) for k in CAMERA_LEAVES} for p in ("64", "32")}
    return kind, KINDS[kind].unpack(z), json.loads(str(z["kwargs"])), np.asarray(z["grad_in/image"]), grads, \
        json.loads(str(z["meta"]))
