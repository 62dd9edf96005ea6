"""Uniform surface samples of a triangle mesh on the GPU: the reference's uniform_sample_mesh
(diffrend/utils/sample_generator.py:157-194) under its own name, batched, and differentiable in the vertices.  The swap
is one import:

    # from diffrend.utils.sample_generator import uniform_sample_mesh
    from surf_renderer_amd import uniform_sample_mesh
    pos, normal = uniform_sample_mesh(obj, num_samples, camera=camera)      # obj = {'v': [V, 3], 'f': [F, 3]}

    topo = mesh_topology(f, V)                                              # once per connectivity
    r = sample_mesh_batched(v, f, uniforms, eye=eyes, topology=topo)        # v [B, V, 3], uniforms [B, S, 3] float64
    nearest_points(r.pos, target).dist_u.mean().backward()                  # d / d v

Per view: a face's weight is the reference's double area (triangle_double_area); with a camera a face is kept iff
n . (eye - v0) >= 0 (numpy/ops.py backface_culling); the face of a sample is the number of faces whose CDF value is
<= r0, which is numpy's choice(p=...); the point is (1 - q) v0 + (1 - t) q v1 + t q v2 with q = sqrt(s), and the normal
is the face's c / |c|.  The three uniforms (r0, s, t) of every sample are an input; uniform_sample_mesh draws them from
numpy in the reference's own order -- random_sample(S), then rand(S, 2) -- so after np.random.seed(k) it consumes the
stream as the reference does and returns the reference's samples.

The kernels (surf_renderer_amd/csrc/srh_mesh.h) compute in fp64 on the float32 values of v, with one fp32 store per
element and no atomic: values and gradients are identical from run to run, a batch equals its views and [V, 3] equals
B = 1.

Three deliberate deviations from the reference:
  - Culled faces.  The reference removes them and returns nothing that names a face.  Here a culled face gets weight 0,
    which selects the same faces, and `face` indexes the caller's f.
  - A view without a positive weight (every face culled, degenerate or not finite).  The reference raises inside
    np.random.choice.  Here that view returns face = -1 and NaN pos, normal and bary, with a zero gradient; the other
    views of the batch are unaffected.  A weight that is not finite and positive counts as 0 wherever it occurs, so one
    NaN vertex does not poison its view.
  - The gradient.  pos and normal are differentiable in v: pos is a barycentric combination of three vertices, the
    normal goes through c / |c| with gradient exactly 0 where |c| = 0.  face, bary, uniforms, eye and the face choice
    are NOT differentiable: this is the usual reparameterisation with the surface parameters held fixed -- the samples
    move with the surface, the area weights that chose their faces are not differentiated.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._layer import as_float_tensor, f32, fill_grads, gpu_device, grad_buffers, ptr, scratch, stream, upstreams
from ._projection import sorted_order

_NAME = "sample_mesh_batched"


class MeshSamples(NamedTuple):
    """pos, normal, bary [B, S, 3] float32 and face [B, S] int64 (without B for a [V, 3] mesh).  pos and normal are
    differentiable in v; face (an index into the caller's f, -1 in a view without a positive weight) and bary are not."""
    pos: torch.Tensor
    normal: torch.Tensor
    face: torch.Tensor
    bary: torch.Tensor


class MeshTopology:
    """What the calls need of a connectivity, made once by mesh_topology: f as the kernels read it (int32, [F, 3] or
    [B, F, 3], contiguous, on the GPU), checked against [0, n_vertices), and the stable ascending order of its flattened
    corners, in which the backward sums the incident corners of every vertex."""

    def __init__(self, f: torch.Tensor, corner_order: torch.Tensor, n_vertices: int):
        self.f, self.corner_order, self.n_vertices = f, corner_order, n_vertices

    @property
    def n_faces(self) -> int:
        return self.f.shape[-2]

    @property
    def n_views(self) -> Optional[int]:
        """B of a per-view connectivity, None for one shared by the views"""
        return self.f.shape[0] if self.f.dim() == 3 else None


def _check_faces(name: str, f: Any, n_vertices: int) -> torch.Tensor:
    """f as an integer tensor on its own device, its shape and range checked (on a device-resident f the range check
    costs a synchronisation: mesh_topology does it once)."""
    if f is None:
        raise ValueError(f"{name}: f is missing")
    t = f if isinstance(f, torch.Tensor) else torch.as_tensor(np.array(f))
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{name}: f has dtype {t.dtype}, expected an integer type")
    if t.dim() not in (2, 3) or t.shape[-1] != 3:
        raise ValueError(f"{name}: f is {list(t.shape)}, expected [F, 3] or [B, F, 3]")
    if not 1 <= t.shape[-2] <= _lib.MESH_MAX:
        raise ValueError(f"{name}: {t.shape[-2]} faces, expected 1..2^24")
    if t.dim() == 3 and not 1 <= t.shape[0] <= 65535:
        raise ValueError(f"{name}: f has {t.shape[0]} views, expected 1..65535")
    if not 1 <= n_vertices <= _lib.MESH_MAX:
        raise ValueError(f"{name}: {n_vertices} vertices, expected 1..2^24")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= n_vertices:
        raise ValueError(f"{name}: f has entries in [{lo}, {hi}], expected [0, {n_vertices})")
    return t


def mesh_topology(f, n_vertices: int, device=None) -> MeshTopology:
    """Check f ([F, 3] shared by the views, or [B, F, 3]; any integer dtype, numpy or torch, any device) against
    [0, n_vertices) and sort its flattened corners, once; pass the result as `topology=` to every call on this
    connectivity.  ValueError before anything reaches the GPU."""
    t = _check_faces("mesh_topology", f, int(n_vertices))
    dev = torch.device(device) if device is not None else gpu_device("mesh_topology", (t,))
    t = t.to(device=dev, dtype=torch.int32).contiguous()
    flat = t.reshape(-1, 3 * t.shape[-2])                                   # [1 or B, 3 F]
    order = sorted_order(flat).reshape(t.shape[:-2] + (3 * t.shape[-2],)).contiguous()
    return MeshTopology(t, order, int(n_vertices))


class _SampleFunction(torch.autograd.Function):
    """v [B, V, 3] fp32 contiguous -> pos, normal [B, S, 3], face [B, S] int32, bary [B, S, 3]"""

    @staticmethod
    def forward(ctx, params, topo, uniforms, eye, v):
        lib = _lib.load()
        B, S, dev = params.n_views, params.n_samples, v.device
        pos, normal, bary = (torch.empty((B, S, 3), dtype=torch.float32, device=dev) for _ in range(3))
        face = torch.empty((B, S), dtype=torch.int32, device=dev)
        n_bytes = lib.srh_mesh_sample_workspace_bytes(C.byref(params), _lib.MESH_WS_FWD)
        ws = scratch(n_bytes, dev)
        _lib.check(lib.srh_mesh_sample_fwd(C.byref(params), v.data_ptr(), topo.f.data_ptr(), ptr(eye),
                                           uniforms.data_ptr(), ws.data_ptr(), n_bytes, pos.data_ptr(),
                                           normal.data_ptr(), face.data_ptr(), bary.data_ptr(), stream(dev)))
        ctx.params, ctx.topo = params, topo
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(face, bary)
        ctx.save_for_backward(v, uniforms, face)
        return pos, normal, face, bary

    @staticmethod
    def backward(ctx, g_pos, g_normal, _g_face, _g_bary):
        v, uniforms, face = ctx.saved_tensors
        grads = grad_buffers((v,), ctx.needs_input_grad[4:5])
        ups = upstreams((g_pos, g_normal))

        def launch():
            lib, params = _lib.load(), ctx.params
            order = sorted_order(face)                      # the scatter as a gather: sorted in the backward only
            n_bytes = lib.srh_mesh_sample_workspace_bytes(C.byref(params), _lib.MESH_WS_BWD)
            ws = scratch(n_bytes, v.device)
            _lib.check(lib.srh_mesh_sample_bwd(C.byref(params), v.data_ptr(), ctx.topo.f.data_ptr(),
                                               uniforms.data_ptr(), face.data_ptr(), order.data_ptr(),
                                               ctx.topo.corner_order.data_ptr(), ptr(ups[0]), ptr(ups[1]),
                                               ws.data_ptr(), n_bytes, grads[0].data_ptr(), stream(v.device)))

        fill_grads(grads, ups, launch)
        return (None, None, None, None, grads[0])


def _validate(name: str, v, f, uniforms, eye, topology):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError)."""
    v = as_float_tensor("v", v, name)
    if v.dim() not in (2, 3) or v.shape[-1] != 3:
        raise ValueError(f"{name}: v is {list(v.shape)}, expected [V, 3] or [B, V, 3]")
    B, V = (v.shape[0] if v.dim() == 3 else 1), v.shape[-2]
    if not 1 <= B <= 65535:
        raise ValueError(f"{name}: {B} views, expected 1..65535")
    if not 1 <= V <= _lib.MESH_MAX:
        raise ValueError(f"{name}: {V} vertices per view, expected 1..2^24")
    if topology is not None:
        if not isinstance(topology, MeshTopology):
            raise ValueError(f"{name}: topology is a {type(topology).__name__}, expected what mesh_topology returns")
        if topology.n_vertices != V:
            raise ValueError(f"{name}: topology was made for {topology.n_vertices} vertices and v has {V}")
        if f is not None and tuple(np.shape(f)) != tuple(topology.f.shape):
            raise ValueError(f"{name}: f is {list(np.shape(f))} and topology was made for {list(topology.f.shape)}")
        f_shape = tuple(topology.f.shape)
    else:
        f = _check_faces(name, f, V)
        f_shape = tuple(f.shape)
    if len(f_shape) == 3 and (v.dim() != 3 or f_shape[0] != B):
        raise ValueError(f"{name}: f has {f_shape[0]} views and v is {list(v.shape)}")
    uniforms = as_float_tensor("uniforms", uniforms, name)
    if uniforms.dim() != v.dim() or uniforms.shape[-1] != 3 or (v.dim() == 3 and uniforms.shape[0] != B):
        form = "[B, S, 3] with v's B" if v.dim() == 3 else "[S, 3]"
        raise ValueError(f"{name}: uniforms is {list(uniforms.shape)}, expected {form}")
    S = uniforms.shape[-2]
    if not 1 <= S <= _lib.MESH_MAX:
        raise ValueError(f"{name}: {S} samples per view, expected 1..2^24")
    if not bool(((uniforms >= 0) & (uniforms < 1)).all()):
        raise ValueError(f"{name}: uniforms has entries outside [0, 1)")
    if eye is not None:
        eye = as_float_tensor("eye", eye, name)
        if tuple(eye.shape) not in ((3,), (B, 3)) or (eye.dim() == 2 and v.dim() != 3):
            raise ValueError(f"{name}: eye is {list(eye.shape)}, expected [3]" + (" or [B, 3]" if v.dim() == 3 else ""))
    return v, f, uniforms, eye, (B, V, f_shape[-2], S)


def _sample(name: str, v, f, uniforms, eye, topology) -> MeshSamples:
    v, f, uniforms, eye, (B, V, F, S) = _validate(name, v, f, uniforms, eye, topology)
    dev = gpu_device(name, (v,) if topology is None else (topology.f, v))
    if topology is None:
        topology = mesh_topology(f, V, device=dev)
    elif topology.f.device != dev:
        raise ValueError(f"{name}: topology is on {topology.f.device} and the call runs on {dev}")
    params = _lib.SrhMeshSampleParams(n_views=B, n_vertices=V, n_faces=F, n_samples=S,
                                      faces_per_view=int(topology.n_views is not None),
                                      eye_per_view=int(eye is not None and eye.dim() == 2))
    uniforms = uniforms.detach().to(device=dev, dtype=torch.float64).reshape(B, S, 3).contiguous()
    if eye is not None:
        eye = eye.detach().to(device=dev, dtype=torch.float64).contiguous()
    pos, normal, face, bary = _SampleFunction.apply(params, topology, uniforms, eye, f32(v, dev).reshape(B, V, 3))
    outs = [pos, normal, face.long(), bary]
    if v.dim() == 2:
        outs = [t[0] for t in outs]
    return MeshSamples(*outs)


def sample_mesh_batched(v, f, uniforms, eye=None, topology: Optional[MeshTopology] = None) -> MeshSamples:
    """S surface samples of each of B meshes in one call.  v [B, V, 3] (or [V, 3]: one mesh, results without B), any
    floating dtype and device, computed on its float32 values in fp64 on the GPU; f [F, 3], shared by the views, or
    [B, F, 3], any integer dtype (may be None with `topology`); uniforms [B, S, 3] float64 = (r0, s, t) per sample, each
    in [0, 1); eye [3] or [B, 3] (float64 as given) turns the backface cull on.  `topology`: mesh_topology(f, V), which
    saves the range check of f (a synchronisation) and the sort of its corners on every call.  1 <= B <= 65535 and V, F,
    S <= 2^24 per view.  Returns MeshSamples(pos, normal, face, bary); gradients reach v in its own dtype, layout and
    device.  What is and is not differentiable, the culled faces and the view without a positive weight: see the
    module's docstring."""
    return _sample(_NAME, v, f, uniforms, eye, topology)


def draw_uniforms(num_samples: int, rng=None) -> np.ndarray:
    """[S, 3] float64 = (r0, s, t) drawn in the reference's order: np.random.choice(p=...) takes random_sample(S), then
    uniform_sample_triangle takes rand(S, 2).  `rng`: an np.random.RandomState, else numpy's global one."""
    rng = np.random if rng is None else rng
    r0 = rng.random_sample(num_samples)
    st = rng.rand(num_samples, 2)
    return np.concatenate([r0[:, None], st], axis=1)


def uniform_sample_mesh(obj, num_samples, camera=None, *, rng=None, uniforms=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's call: obj = {'v': [V, 3], 'f': [F, 3]}, num_samples = S, camera = {'eye': ...} (only the eye is
    read, as in the reference) -> (pos [S, 3], normal [S, 3]), float32 tensors on the GPU, differentiable in obj['v']
    where that is a tensor that requires grad.  The uniforms are drawn by draw_uniforms(S, rng) unless given ([S, 3]).
    The reference's optional precomputed 'a' (areas) and 'fn' (normals) are refused, not ignored."""
    name = "uniform_sample_mesh"
    for k in ("a", "fn"):
        if k in obj:
            raise ValueError(f"{name}: obj['{k}'] (precomputed {'areas' if k == 'a' else 'normals'}) is not supported; "
                             "remove it and they are computed from v and f")
    if "v" not in obj or "f" not in obj:
        raise ValueError(f"{name}: obj needs 'v' and 'f'")
    v = as_float_tensor("obj['v']", obj["v"], name)
    if v.dim() != 2:
        raise ValueError(f"{name}: obj['v'] is {list(v.shape)}, expected [V, 3]")
    f = obj["f"] if isinstance(obj["f"], torch.Tensor) else torch.as_tensor(np.array(obj["f"]))
    if f.dim() != 2:
        raise ValueError(f"{name}: obj['f'] is {list(f.shape)}, expected [F, 3]")
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 1:
        raise ValueError(f"{name}: num_samples = {num_samples!r}, expected an integer >= 1")
    eye = None
    if camera is not None:
        if "eye" not in camera:
            raise ValueError(f"{name}: camera has no 'eye'")
        e = camera["eye"]
        e = e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else np.asarray(e)
        eye = torch.as_tensor(np.asarray(e, np.float64).reshape(-1)[:3].copy())
    if uniforms is None:
        # validate before the stream is consumed, so that a refused call leaves the generator where it was
        _validate(name, v, f, np.zeros((1, 3)), eye, None)
        uniforms = draw_uniforms(int(num_samples), rng)
    else:
        uniforms = as_float_tensor("uniforms", uniforms, name)
        if uniforms.dim() != 2 or uniforms.shape[0] != num_samples:
            raise ValueError(f"{name}: uniforms is {list(uniforms.shape)}, expected [{num_samples}, 3]")
    r = _sample(name, v, f, uniforms, eye, None)
    return r.pos, r.normal
