#!/usr/bin/env python3
"""sample_mesh_batched against what a user has without it, on the GPU: forward + backward of pos.sum() + normal.sum(),
and the forward alone.

Workload: B views of the bunny (assets/data/bunny.obj, 2503 vertices, 4968 faces; every view rotated, scaled and
shifted a little), one connectivity, no camera, S uniform samples per view from RandomState(0).
Forms, in one process, alternating round by round after a warm-up so that all see the same machine state:
    fused               sample_mesh_batched with a topology made once (HIP kernels; the stable sort of the backward is
                        torch's)
    torch               the same computation composed in float32 torch on the same GPU: gathers, torch.cumsum,
                        torch.searchsorted(right=True), gathers; autograd's backward (index_add into the vertices)
    fused_forward       the fused call on vertices that do not require grad
    torch_forward       the composition under torch.no_grad()
    reference_forward   the reference's path: float64 numpy on the host, one mesh per call -- face normals and double areas,
                        np.random.choice(p=area / sum), rand(S, 2) and the barycentric combination, written out here so
                        that the tool runs without the reference checkout -- for each of the B meshes, then the upload
                        of pos and normal.  It draws its own uniforms, as the reference does.
Before the timing, fused and torch are each compared with the composition run once in float64 on the same float32
vertices (not timed): the share of samples on the same face, the points where the face agrees, and grad_v.
Sizes: --views x --size^2 samples (64 x 128^2 by default) and --small-views x --small-size^2 (8 x 48^2).
Each round times a window of at least --window seconds per form with device events (the host's numpy work of
reference_forward lies between the two events); the rounds are run --runs times (twice by default) and every run is
reported, one JSON line each.  Fails without a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_bench as pb  # noqa: E402  (puts the repository and tests/ on the path)
import mesh_sampling_cases as cases  # noqa: E402
from surf_renderer_amd import mesh_topology, sample_mesh_batched  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--small-views", type=int, default=8)
ap.add_argument("--small-size", type=int, default=48)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mesh_sampling: no GPU")
dev = torch.device("cuda:0")


def workload(B, S):
    v0, f = cases.load_obj("bunny")
    rng = np.random.RandomState(0)
    v = np.stack([cases._moved(v0 / np.abs(v0).max(), rng) for _ in range(B)]).astype(np.float32)
    return v, f, rng.random_sample((B, S, 3))


def torch_composition(v, f, u):
    """v [B, V, 3] float32, f [F, 3] int64, u [B, S, 3] float32 -> pos, normal [B, S, 3], face [B, S]"""
    tri = v[:, f]                                                     # [B, F, 3, 3]
    c = torch.linalg.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
    length = c.norm(dim=-1, keepdim=True)
    n = c / torch.where(length == 0, torch.ones_like(length), length)
    r, s = tri[:, :, 0] - tri[:, :, 2], tri[:, :, 1] - tri[:, :, 2]
    area = torch.linalg.cross(r, s).norm(dim=-1).detach()             # the face choice is not differentiated
    cdf = torch.cumsum(area, dim=-1)
    cdf = cdf / cdf[:, -1:]
    face = torch.searchsorted(cdf, u[..., 0].contiguous(), right=True).clamp_(max=f.shape[0] - 1)
    q = torch.sqrt(u[..., 1])
    bary = torch.stack((1 - q, (1 - u[..., 2]) * q, u[..., 2] * q), dim=-1)
    B, S = face.shape
    corners = f[face].reshape(B, S * 3, 1).expand(-1, -1, 3)          # [B, 3 S, 3]
    pos = (bary[..., None] * torch.gather(v, 1, corners).reshape(B, S, 3, 3)).sum(dim=2)
    normal = torch.gather(n, 1, face[..., None].expand(-1, -1, 3))
    return pos, normal, face


def reference_formulation(v, f, n_samples):
    """one mesh in float64 numpy the way the reference works: face normals and double areas for every face,
    np.random.choice(p=area / sum), then rand(S, 2) for the point inside each chosen triangle"""
    p = v[f]                                                          # [F, 3 corners, 3]
    c = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(c, axis=1)
    normal = c / np.where(length == 0, 1.0, length)[:, None]
    area = np.linalg.norm(np.cross(p[:, 0] - p[:, 2], p[:, 1] - p[:, 2]), axis=1)
    face = np.random.choice(len(f), n_samples, p=area / area.sum())
    st = np.random.rand(n_samples, 2)
    q = np.sqrt(st[:, 0])
    bary = np.stack([1 - q, (1 - st[:, 1]) * q, st[:, 1] * q], axis=1)
    return np.einsum("sc,sck->sk", bary, p[face]), normal[face]


def bench(B, size):
    S = size * size
    v_host, f_host, u_host = workload(B, S)
    v = torch.tensor(v_host, device=dev, requires_grad=True)
    v_plain = v.detach()
    f = torch.tensor(f_host, device=dev)
    u64 = torch.tensor(u_host, device=dev)
    u32 = u64.float()
    topo = mesh_topology(f, v.shape[1])
    v_host64 = v_host.astype(np.float64)

    def fused():
        v.grad = None
        r = sample_mesh_batched(v, None, u64, topology=topo)
        (r.pos.sum() + r.normal.sum()).backward()

    def composed():
        v.grad = None
        pos, normal, _ = torch_composition(v, f, u32)
        (pos.sum() + normal.sum()).backward()

    def composed_forward():
        with torch.no_grad():
            return torch_composition(v_plain, f, u32)

    def reference_forward():
        out = [reference_formulation(v_host64[b], f_host, S) for b in range(B)]
        pos = torch.tensor(np.stack([o[0] for o in out]), dtype=torch.float32).to(dev)
        normal = torch.tensor(np.stack([o[1] for o in out]), dtype=torch.float32).to(dev)
        return pos, normal

    forms = {"fused": fused, "torch": composed,
             "fused_forward": lambda: sample_mesh_batched(v_plain, None, u64, topology=topo),
             "torch_forward": composed_forward, "reference_forward": reference_forward}
    grads = {}
    for name in ("fused", "torch"):                                   # warm-up, and each form's gradient
        forms[name](); forms[name]()
        torch.cuda.synchronize()
        grads[name] = v.grad.double().clone()
    for name in ("fused_forward", "torch_forward", "reference_forward"):
        forms[name]()
    torch.cuda.synchronize()
    # both forms against the composition in float64 on the same float32 vertices (not timed)
    v64 = v_plain.double().requires_grad_(True)
    pos64, normal64, face64 = torch_composition(v64, f, u64)
    (pos64.sum() + normal64.sum()).backward()
    r = forms["fused_forward"]()
    pos32, normal32, face32 = composed_forward()
    agreement = {}
    for name, face, pos in (("fused", r.face, r.pos), ("torch", face32, pos32)):
        same = face == face64
        agreement[name] = {
            "faces_equal_share": float(f"{float(same.double().mean()):.6g}"),
            "pos_max_difference_where_equal": float(f"{float((pos.double() - pos64.detach())[same].abs().max()):.3g}"),
            "grad_v_max_difference_over_max": float(f"{float((grads[name] - v64.grad).abs().max() / v64.grad.abs().max()):.3g}")}
    del v64, pos64, normal64, face64
    for run in range(args.runs):
        calls, times, med = pb.timed(forms, args.rounds, args.window)
        out = {"workload": "bunny_pos_sum_plus_normal_sum", "run": run + 1, "views": B, "samples_per_view": S,
               "faces": int(f.shape[0]), "vertices": int(v.shape[1]), "rounds": args.rounds,
               "window_s_at_least": args.window, "calls_per_window": calls}
        out.update({name: pb.spread(ts) for name, ts in times.items()})
        out["ratio_of_medians"] = {"torch_over_fused": round(med["torch"] / med["fused"], 2),
                                   "torch_forward_over_fused_forward": round(med["torch_forward"] / med["fused_forward"], 2),
                                   "reference_forward_over_fused_forward": round(med["reference_forward"] / med["fused_forward"], 2)}
        out["fused_apart_from_every_round_of"] = {
            "torch": bool(max(times["fused"]) < min(times["torch"]) or min(times["fused"]) > max(times["torch"])),
            "torch_forward": bool(max(times["fused_forward"]) < min(times["torch_forward"])
                                  or min(times["fused_forward"]) > max(times["torch_forward"])),
            "reference_forward": bool(max(times["fused_forward"]) < min(times["reference_forward"])
                                      or min(times["fused_forward"]) > max(times["reference_forward"]))}
        if run == 0:
            out["against_the_float64_composition"] = agreement
        print(json.dumps(out), flush=True)


bench(args.views, args.size)
bench(args.small_views, args.small_size)
