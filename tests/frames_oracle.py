"""fp64 restatement of the reference's frame transforms and point projection -- world_to_cam[_batched],
cam_to_world[_batched] (diffrend/torch/utils.py:539-647), project_surfels and project_image_coordinates
(diffrend/torch/projection_layer.py:19-85) -- in torch on the CPU, with the camera's eye, at and up as possible autograd
leaves, so that autograd supplies the gradient oracle, the camera's included.  Test infrastructure:
tests/test_frames_oracle_cpu.py pins it to the reference's own float64 and float32 results
(tests/golden/frames/fr1_*.npz), tests/test_hip_frames.py compares the kernels with it.

lookat, nonzero_divide and the camera leaves are projection_oracle's and camera_chain_oracle's, by import.  A camera
entry may be an array or a tensor, [B, 3] or [B, 4]; the w column is dropped before lookat.  `dtype` and `device` follow
the inputs: tools/bench_frames.py times this composition in float32 on the GPU."""
from typing import Dict, Mapping, Optional

import numpy as np
import torch

import camera_chain_oracle as cco
import projection_oracle as po

CAMERA_KEYS = cco.CAMERA_KEYS


def homogeneous(p):
    """[..., 3] -> [..., 4] with w = 1; [..., 4] as it is."""
    return p if p.shape[-1] == 4 else torch.cat((p, torch.ones_like(p[..., :1])), dim=-1)


def _tables(camera: Mapping, like):
    """(world-to-camera [B, 3, 4], camera-to-world [B, 3, 4]) in the dtype and on the device of `like`."""
    dt, dev = like.dtype, like.device
    R, eye = cco.camera_to_world(camera, dt)
    return cco.world_to_camera(camera, dt)[:, :3].to(dev), torch.cat((R, eye[..., None]), dim=-1).to(dev)


def _apply(pos, normal, m_pos, m_normal) -> Dict[str, Optional[torch.Tensor]]:
    """pos -> [M p | w] (four columns), normal -> n^T A with A the 3 x 3 of the OTHER direction's matrix."""
    out = {"pos": None, "normal": None}
    if pos is not None:
        h = homogeneous(pos)
        out["pos"] = torch.cat((h @ m_pos.transpose(-1, -2), h[..., 3:]), dim=-1)
    if normal is not None:
        out["normal"] = normal[..., :3] @ m_normal[..., :3, :3]
    return out


def world_to_cam_batched(pos, normal, camera: Mapping):
    like = pos if pos is not None else normal
    w2c, c2w = _tables(camera, like)
    return _apply(pos, normal, w2c, c2w)


def cam_to_world_batched(pos, normal, camera: Mapping):
    like = pos if pos is not None else normal
    w2c, c2w = _tables(camera, like)
    return _apply(pos, normal, c2w, w2c)


TRANSFORMS = {"to_cam": world_to_cam_batched, "to_world": cam_to_world_batched}


def project_surfels(surfels, camera: Mapping):
    cc = world_to_cam_batched(surfels, None, camera)["pos"]
    f = float(camera["focal_length"])
    return torch.stack((f * po.nonzero_divide(cc[..., 0], cc[..., 2]), f * po.nonzero_divide(cc[..., 1], cc[..., 2]),
                        -cc[..., 2]), dim=-1)


def frame_scales(camera: Mapping):
    """((sx, sy), (W / 2, H / 2)) of px_coord = plane * scale + half."""
    W, H = po.frame(camera)
    f, fovy = float(camera["focal_length"]), float(camera["fovy"])
    h = np.tan(fovy / 2) * 2 * f
    w = h * (float(W) / float(H))
    return (-(W - 1) / w, (H - 1) / h), (W / 2.0, H / 2.0)


def project_image_coordinates(surfels, camera: Mapping):
    """(px_idx [B, N] int64 with W H the dump slot, px_coord [B, N, 3])."""
    W, H = po.frame(camera)
    plane = project_surfels(surfels, camera)
    (sx, sy), (hx, hy) = frame_scales(camera)
    px = torch.stack((plane[..., 0] * sx + hx, plane[..., 1] * sy + hy, plane[..., 2]), dim=-1)
    r = torch.round(px[..., :2].detach() - 0.5)                 # ties to even
    inside = (r[..., 0] >= 0) & (r[..., 0] <= W - 1) & (r[..., 1] >= 0) & (r[..., 1] <= H - 1)   # false for NaN
    safe = torch.where(inside[..., None], r, torch.zeros_like(r)).long()
    idx = torch.where(inside, safe[..., 1] * W + safe[..., 0], torch.full_like(safe[..., 0], W * H))
    return idx, px


def transform_gradients(direction, inputs, camera: Mapping, upstream, camera_wrt=CAMERA_KEYS):
    """({'pos', 'normal'} of those given, {input: gradient}, {entry: gradient}) of TRANSFORMS[direction]."""
    def fn(x, c):
        res = TRANSFORMS[direction](x.get("pos"), x.get("normal"), c["camera"])
        return {k: v for k, v in res.items() if v is not None}
    vals, grads, cams = cco.autograd(fn, inputs, ("pos", "normal"), {"camera": camera}, upstream, ("pos", "normal"),
                                     camera_wrt)
    return vals, grads, cams["camera"]


def _np_tables(camera: Mapping):
    """(world-to-camera, camera-to-world) [B, 3, 4] as fp64 arrays."""
    return tuple(t.numpy() for t in _tables(camera, torch.zeros(1, dtype=torch.float64)))


def _np_homogeneous(p):
    p = np.asarray(p, np.float64)
    return p if p.shape[-1] == 4 else np.concatenate((p, np.ones_like(p[..., :1])), -1)


def _w2c_table(eye, at, up):
    return po.lookat(eye, at, up)[:, :3]


def _c2w_table(eye, at, up):
    R, eye = cco.camera_to_world({"eye": eye, "at": at, "up": up}, eye.dtype)
    return torch.cat((R, eye[..., None]), dim=-1)


def transform_magnitudes(direction, inputs, camera: Mapping, upstream):
    """The sums of the absolute values of the terms of every entry transform_gradients returns, in the same three dicts
    (tests/entry_checks.py's A), numpy fp64.  Only the sums are restated, not the function:
        out_pos[r]     sum_c |P[r][c]| |v_c|,  v = [p, w];  out_pos[3] = |w|
        out_normal[j]  sum_i |n_i| |A[i][j]|
        grad_pos[c]    sum_r |g_r| |P[r][c]|, column 3 of a four-column input one more term, |g_3|
        grad_normal[i] sum_j |g_j| |A[i][j]|, column 3 of a four-column input 0
        camera         entry_checks.camera_magnitudes of d loss / dP (sum over the points of |g_r| |v_c|) and
                       d loss / dA (sum of |n_i| |g_j|, column 3 exactly 0)"""
    w2c, c2w = _np_tables(camera)
    P, A = (w2c, c2w) if direction == "to_cam" else (c2w, w2c)
    fns = (_w2c_table, _c2w_table) if direction == "to_cam" else (_c2w_table, _w2c_table)
    vals, grads, tables = {}, {}, []
    if inputs.get("pos") is not None:
        v = np.abs(_np_homogeneous(inputs["pos"]))
        vals["pos"] = np.concatenate((np.einsum("brc,bnc->bnr", np.abs(P), v), v[..., 3:]), -1)
        if "pos" in upstream:
            g = np.abs(np.asarray(upstream["pos"], np.float64))
            gp = np.einsum("bnr,brc->bnc", g[..., :3], np.abs(P))
            gp[..., 3] += g[..., 3]
            grads["pos"] = gp[..., :np.asarray(inputs["pos"]).shape[-1]]
            tables.append((fns[0], np.einsum("bnr,bnc->brc", g[..., :3], v)))
        else:
            grads["pos"] = np.zeros(np.asarray(inputs["pos"]).shape)
    if inputs.get("normal") is not None:
        n = np.abs(np.asarray(inputs["normal"], np.float64))
        vals["normal"] = np.einsum("bni,bij->bnj", n[..., :3], np.abs(A[..., :3]))
        grads["normal"] = np.zeros(n.shape)
        if "normal" in upstream:
            h = np.abs(np.asarray(upstream["normal"], np.float64))
            grads["normal"][..., :3] = np.einsum("bnj,bij->bni", h, np.abs(A[..., :3]))
            A_dA = np.zeros(A.shape)
            A_dA[..., :3] = np.einsum("bni,bnj->bij", n[..., :3], h)
            tables.append((fns[1], A_dA))
    import entry_checks
    return vals, grads, entry_checks.camera_magnitudes(tables, camera)


def project_magnitudes(coords: bool, surfels, camera: Mapping, upstream):
    """As transform_magnitudes, for what project_gradients returns (px_idx has no magnitude).  (X, Y, Z) are sums of
    four products with A_X, A_Y, A_Z = sum_c |M[r][c]| |v_c|, and Z is itself a cancelling sum: its own fp64 error is
    2^-53 A_Z and not 2^-53 |Z|, and it reaches every quotient through 1 / Zd.  So every derived A carries the forward
    A of X, Y and Z, by the product and quotient rules on (value, A) pairs:
        plane_x        |f| (A_X / |Zd| + |X| A_Z / Zd^2), plane_y alike;  the third component A_Z
        px_coord_x     A_plane_x |sx| + W / 2, px_coord_y alike
        gx, gy, gz     |g_plane| + |g_coord| |s|
        dX             |f| (|gx| / |Zd| + |gx| A_Z / Zd^2), dY alike
        dZ             |gz| + |f| (|gx| A_X + |gy| A_Y) / Zd^2 + 2 |f| (|gx| |X| + |gy| |Y|) A_Z / |Zd|^3; |gz| at Z == 0
        grad_surfels   sum_r A_d[r] |M[r][c]|;   d loss / dM[r][c] = sum over the points of A_d[r] |v_c|
    These are upper bounds on the sums of |terms|, above them by the factor (1 + A_Z / |Zd|) at the most, which on the
    seeded cases (|Z| >= 1.5, the scene within a few units of the eye) stays far below 2^8
    (tests/test_entry_checks_cpu.py measures it)."""
    M = _np_tables(camera)[0]
    v = _np_homogeneous(surfels)
    cc = np.einsum("brc,bnc->bnr", M, v)
    A_cc = np.einsum("brc,bnc->bnr", np.abs(M), np.abs(v))
    X, Y, Z = (np.abs(cc[..., k]) for k in range(3))
    A_X, A_Y, A_Z = (A_cc[..., k] for k in range(3))
    live = cc[..., 2] != 0
    Zd = np.where(live, Z, 1.0)
    f = abs(float(camera["focal_length"]))
    (sx, sy), (hx, hy) = frame_scales(camera)
    out = "px_coord" if coords else "plane"
    plane = [f * (A_X / Zd + X * A_Z / Zd ** 2), f * (A_Y / Zd + Y * A_Z / Zd ** 2), A_Z]
    if coords:
        plane = [plane[0] * abs(sx) + abs(hx), plane[1] * abs(sy) + abs(hy), A_Z]
    vals = {out: np.stack(plane, -1)}
    g = np.abs(np.asarray(upstream[out], np.float64))
    gx, gy, gz = (g[..., 0] * abs(sx), g[..., 1] * abs(sy), g[..., 2]) if coords else (g[..., 0], g[..., 1], g[..., 2])
    d = np.stack((f * (gx / Zd + gx * A_Z / Zd ** 2), f * (gy / Zd + gy * A_Z / Zd ** 2),
                  gz + np.where(live, f * (gx * A_X + gy * A_Y) / Zd ** 2
                                + 2 * f * (gx * X + gy * Y) * A_Z / Zd ** 3, 0.0)), -1)
    cols = np.asarray(surfels).shape[-1]
    grads = {"surfels": np.einsum("bnr,brc->bnc", d, np.abs(M))[..., :cols]}
    import entry_checks
    return vals, grads, entry_checks.camera_magnitudes([(_w2c_table, np.einsum("bnr,bnc->brc", d, np.abs(v)))], camera)


def project_gradients(coords: bool, surfels, camera: Mapping, upstream, camera_wrt=CAMERA_KEYS):
    """project_surfels ({'plane'}) or with `coords` project_image_coordinates ({'px_coord', 'px_idx'})."""
    def fn(x, c):
        if not coords:
            return {"plane": project_surfels(x["surfels"], c["camera"])}
        idx, px = project_image_coordinates(x["surfels"], c["camera"])
        return {"px_coord": px, "px_idx": idx}
    vals, grads, cams = cco.autograd(fn, {"surfels": surfels}, ("surfels",), {"camera": camera}, upstream, ("surfels",),
                                     camera_wrt)
    return vals, grads, cams["camera"]
