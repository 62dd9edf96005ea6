"""The host scaffold the fused layer modules share (splats, regularizers and the three projection layers): device
choice, scratch, the float32-contiguous conversion and the backward pattern.  The camera helpers of the projection
layers are in _camera.py, what else those three share in _projection.py.  A layer whose wording or steps differ keeps
its own code."""
from __future__ import annotations

from typing import Any, Callable, Iterable, List, Optional, Sequence

import numpy as np
import torch


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def gpu_device(name: str, tensors: Iterable[Any]) -> torch.device:
    """Where the layer `name` runs: the device of the first CUDA tensor among `tensors`, else the current GPU."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{name}: the hip backend needs a GPU")
    return next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.device.type == "cuda"),
                torch.device("cuda"))


def scratch(n_bytes: int, device) -> torch.Tensor:
    return torch.empty((n_bytes,), dtype=torch.uint8, device=device)


def stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def f32(t: torch.Tensor, device) -> torch.Tensor:
    """float32, contiguous, on `device`; autograd carries the gradient back through these conversions to the leaf's own
    dtype, layout and device"""
    return t.to(device=device, dtype=torch.float32).contiguous()


def as_float_tensor(name: str, x: Any, caller: str) -> torch.Tensor:
    if x is None:
        raise ValueError(f"{caller}: {name} is missing")
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if not t.is_floating_point():
        raise ValueError(f"{caller}: {name} has dtype {t.dtype}, expected a floating-point type")
    return t


def grad_buffers(inputs: Sequence[Optional[torch.Tensor]], needed: Sequence[bool]) -> List[Optional[torch.Tensor]]:
    """An input that does not require grad gets no buffer, and the kernels skip the work only it would need."""
    return [torch.empty_like(t) if t is not None and need else None for t, need in zip(inputs, needed)]


def view_grad_buffers(lib, views: Sequence[torch.Tensor], needed: Sequence[bool], width: int, height: int,
                      n_bytes: Optional[Callable[[], int]] = None):
    """The extra output of a layer's backward under camera_grad: per view table float64 that requires grad a [B, 12]
    buffer (the *_bwd_view entry point writes every element), else None; and the partials workspace those entry points
    share -- None when no table requires grad, and the backward is then the plain one.  `n_bytes` gives the workspace's
    size where the layer's kernel does not run srh_view_grad_workspace_bytes' 256-lane workgroups."""
    grads = [torch.empty((v.shape[0], 12), dtype=v.dtype, device=v.device) if need else None
             for v, need in zip(views, needed)]
    if all(g is None for g in grads):
        return grads, None
    size = n_bytes() if n_bytes else lib.srh_view_grad_workspace_bytes(views[0].shape[0], width, height)
    return grads, scratch(size, views[0].device)


def view_grad_buffers_for_points(lib, views, needed, n_points: int, tables: int = 1):
    """view_grad_buffers for a layer whose lanes are N free points, not the W H pixels of a frame: `views` may hold
    None (an absent input's table, which gets no buffer), and the workspace holds `tables` sets of partials of
    ceil(N / 256) workgroups each."""
    there = [(v, need) for v, need in zip(views, needed) if v is not None]
    if not there:
        return [None] * len(views), None
    B = there[0][0].shape[0]
    got, ws = view_grad_buffers(lib, [v for v, _ in there], [need for _, need in there], n_points, 1,
                                n_bytes=lambda: tables * lib.srh_view_grad_workspace_bytes(B, n_points, 1))
    got = iter(got)
    return [None if v is None else next(got) for v in views], ws


def upstreams(grads: Iterable[Optional[torch.Tensor]]) -> List[Optional[torch.Tensor]]:
    return [None if g is None else g.to(torch.float32).contiguous() for g in grads]


def fill_grads(grads: Iterable[Optional[torch.Tensor]], ups: Iterable[Optional[torch.Tensor]],
               launch: Callable[[], None]) -> None:
    """The backward of a layer whose kernels write every element of every buffer in `grads`: nothing without a buffer,
    zeros without an upstream gradient, else `launch()`."""
    grads = [g for g in grads if g is not None]
    if not grads:
        return
    if all(u is None for u in ups):
        for g in grads:
            g.zero_()
    else:
        launch()
