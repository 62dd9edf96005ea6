"""Distances between two point sets without the pair tensor: per-point nearest neighbours in both directions, and the
reference's hausdorff (diffrend/torch/ops.py:112-125) on top of them under its own name, so the swap is one import:

    # from diffrend.torch.ops import hausdorff
    from surf_renderer_amd import hausdorff
    sym, uv, vu = hausdorff(u, v)

    r = nearest_points(u, v)                       # u [B, N, D], v [B, M, D]
    chamfer = r.dist_u.mean(-1) + r.dist_v.mean(-1)

The reference forms the [N, M, D] difference tensor; the kernels (surf_renderer_amd/csrc/srh_pointsets.h) stream one set
past the other and keep O(B (N + M)) memory.  Differences, squares, their sum over D in ascending component order and the
square root are fp64 on the float32 inputs, with one fp32 store per element; no atomic, so values and gradients are
identical from run to run, a batch equals its views and [N, D] equals B = 1.

Three deliberate deviations from the reference:
  - NaN.  The running best starts at +inf with index 0 and a candidate wins only when its squared distance is strictly
    smaller, so a candidate whose squared distance is NaN or +inf never wins, and a query without a finite candidate
    gets dist = +inf, idx = 0.  The reference's torch.min lets one NaN target poison every query.
  - Ties.  Candidates are visited in ascending index: an exact tie goes to the lowest index.  torch.min leaves it open.
  - Coincident points.  The derivative of dist_u[i] is (u_i - v_j) / dist with respect to u_i and its negative with
    respect to the nearest v_j, and exactly 0 where the fp64 distance is 0 or not finite.  The reference gives NaN for
    every coincident pair, selected or not (0 / 0 in sqrt's backward).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._layer import as_float_tensor, f32, fill_grads, gpu_device, grad_buffers, ptr, stream
from ._projection import sorted_order

_NAME = "nearest_points"


class NearestPoints(NamedTuple):
    """dist_u, idx_u [B, N]: for each u_i the distance to its nearest v and that v's index; dist_v, idx_v [B, M] the
    other way round (None, None under directed=True).  dist float32, idx int64; without B for [N, D] inputs."""
    dist_u: torch.Tensor
    idx_u: torch.Tensor
    dist_v: Optional[torch.Tensor]
    idx_v: Optional[torch.Tensor]


class _NearestFunction(torch.autograd.Function):
    """(u [B, N, D], v [B, M, D]), fp32 contiguous -> dist_u [B, N], idx_u [B, N] int32 and, unless directed, dist_v,
    idx_v [B, M].  The distances are the kernel's float32 values WIDENED to float64, so that their upstream gradients
    arrive in float64: where two of them meet in one distance (hausdorff's symmetric and directed values) autograd's
    sum is then exact, and it multiplies a direction that the other set's term may cancel."""

    @staticmethod
    def forward(ctx, params, directed, u, v):
        lib = _lib.load()
        B, N, M, dev = params.n_views, params.n_u, params.n_v, u.device
        outs = [torch.empty((B, N), dtype=torch.float32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev)]
        if not directed:
            outs += [torch.empty((B, M), dtype=torch.float32, device=dev),
                     torch.empty((B, M), dtype=torch.int32, device=dev)]
        _lib.check(lib.srh_nearest_points_fwd(C.byref(params), u.data_ptr(), v.data_ptr(),
                                              *[ptr(t) for t in outs + [None] * (4 - len(outs))], stream(dev)))
        ctx.params = params
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*outs[1::2])
        ctx.save_for_backward(u, v, *outs[1::2])
        return tuple(t if k % 2 else t.double() for k, t in enumerate(outs))

    @staticmethod
    def backward(ctx, g_dist_u, _g_idx_u, g_dist_v=None, _g_idx_v=None):
        u, v, idx_u, *rest = ctx.saved_tensors
        idx_v = rest[0] if rest else None
        grads = grad_buffers((u, v), ctx.needs_input_grad[2:4])
        ups = [None if g is None else g.contiguous() for g in (g_dist_u, g_dist_v)]          # float64, as the outputs

        def launch():
            # the fan-in of a side is a gather over the other side's ordered indices: sorted only where it is summed
            order_u = sorted_order(idx_u) if ups[0] is not None and grads[1] is not None else None
            order_v = sorted_order(idx_v) if ups[1] is not None and grads[0] is not None else None
            _lib.check(_lib.load().srh_nearest_points_bwd(C.byref(ctx.params), u.data_ptr(), v.data_ptr(), ptr(idx_u),
                                                          ptr(idx_v), ptr(order_u), ptr(order_v), ptr(ups[0]),
                                                          ptr(ups[1]), ptr(grads[0]), ptr(grads[1]), stream(u.device)))

        fill_grads(grads, ups, launch)
        return (None, None, *grads)


def _validate(name: str, u, v, batched: Optional[bool] = None):
    """Everything the kernels index by, checked on the host before anything reaches the GPU (ValueError).  `batched`:
    the rank the caller insists on (hausdorff: False, hausdorff_batched: True), None for either."""
    u, v = as_float_tensor("u", u, name), as_float_tensor("v", v, name)
    ranks = (2, 3) if batched is None else ((3,) if batched else (2,))
    form = " or ".join({2: "[N, D]", 3: "[B, N, D]"}[r] for r in ranks)
    for k, t in (("u", u), ("v", v)):
        if t.dim() not in ranks:
            raise ValueError(f"{name}: {k} is {list(t.shape)}, expected {form}")
    if u.dim() != v.dim():
        raise ValueError(f"{name}: u is {list(u.shape)} and v is {list(v.shape)}: one has a batch and the other has not")
    B = u.shape[0] if u.dim() == 3 else 1
    if u.dim() == 3 and v.shape[0] != B:
        raise ValueError(f"{name}: u has {B} views and v has {v.shape[0]}")
    N, M, D = u.shape[-2], v.shape[-2], u.shape[-1]
    if v.shape[-1] != D:
        raise ValueError(f"{name}: u has {D} columns and v has {v.shape[-1]}")
    if not 1 <= D <= _lib.POINTSETS_MAX_DIMS:
        raise ValueError(f"{name}: points have {D} columns, expected 1..{_lib.POINTSETS_MAX_DIMS}")
    if not 1 <= B <= 65535:
        raise ValueError(f"{name}: {B} views, expected 1..65535")
    for k, n in (("u", N), ("v", M)):
        if not 1 <= n <= _lib.POINTSETS_MAX_POINTS:
            raise ValueError(f"{name}: {k} has {n} points per view, expected 1..2^24")
    return u, v, (B, N, M, D)


def _nearest(name: str, u, v, squared: bool, directed: bool, batched: Optional[bool], wide: bool = False) -> NearestPoints:
    """`wide`: the distances stay in _NearestFunction's float64 (hausdorff's maxima run on them); else float32."""
    u, v, (B, N, M, D) = _validate(name, u, v, batched)
    dev = gpu_device(name, (u, v))
    params = _lib.SrhPointSetParams(n_views=B, n_u=N, n_v=M, dims=D, squared=int(bool(squared)))
    outs = _NearestFunction.apply(params, bool(directed), f32(u, dev).reshape(B, N, D), f32(v, dev).reshape(B, M, D))
    outs = [t.long() if k % 2 else (t if wide else t.float()) for k, t in enumerate(outs)]
    if u.dim() == 2:
        outs = [t[0] for t in outs]
    return NearestPoints(*outs, *[None] * (4 - len(outs)))


def nearest_points(u, v, squared: bool = False, directed: bool = False) -> NearestPoints:
    """For each point of u its nearest point of v, and the other way round.  u [N, D] and v [M, D], or [B, N, D] and
    [B, M, D] with one B; D in 1..4, N and M in 1..2^24 and independent, any floating dtype and device (computed in
    float32 values, fp64 arithmetic, on the GPU).  Returns NearestPoints(dist_u, idx_u, dist_v, idx_v): dist float32,
    differentiable in u and v (gradients come back in each leaf's own dtype, layout and device), idx int64, not
    differentiable.  squared=True: squared distances, whose gradient is 2 (u - v) without a division.  directed=True:
    the u side only, at half the work -- a one-sided Chamfer term; dist_v and idx_v are None.  Ties, NaN and
    coincident points: see the module's docstring."""
    return _nearest(_NAME, u, v, squared, directed, None)


def _hausdorff(r: NearestPoints) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    # the reference's orientation: its D.min(dim=0) runs over u, so uv is the farthest v from u.  amax, not max(dim):
    # the reference's torch.max(x) over a whole tensor shares the gradient evenly among tied maxima, and so does amax
    uv, vu = r.dist_v.amax(dim=-1), r.dist_u.amax(dim=-1)
    return torch.maximum(uv, vu).float(), uv.float(), vu.float()                 # float32 values in float64: exact


def hausdorff(u, v) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The reference's call: u [N, D], v [M, D] -> (symmetric, uv, vu), three 0-d float32 tensors with
    uv = max_j min_i |u_i - v_j|, vu = max_i min_j |u_i - v_j| and symmetric = max(uv, vu).  The outer maxima are torch's
    own, so a tied maximum splits its gradient as the reference's does."""
    return _hausdorff(_nearest("hausdorff", u, v, False, False, False, wide=True))


def hausdorff_batched(u, v) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """hausdorff for u [B, N, D], v [B, M, D]: three [B] tensors, each view's values those of hausdorff(u[b], v[b])."""
    return _hausdorff(_nearest("hausdorff_batched", u, v, False, False, True, wide=True))
