"""splat_regularizers refuses what the kernels cannot index -- ValueError on the host, before anything reaches the GPU
(so these run without one)."""
import numpy as np
import pytest
import torch

from surf_renderer_amd import splat_regularizers


def _res(B=2, H=4, W=5, dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    shape = (B, H, W) if B else (H, W)
    return {"pos": torch.rand(*shape, 3, generator=g).to(dtype), "normal": torch.rand(*shape, 3, generator=g).to(dtype),
            "image": torch.rand(*shape, 3, generator=g).to(dtype), "depth": torch.rand(*shape, generator=g).to(dtype)}


@pytest.mark.parametrize("key", ["pos", "normal", "image", "depth"])
def test_a_missing_key(key):
    res = _res()
    del res[key]
    with pytest.raises(ValueError, match=key):
        splat_regularizers(res, 2.0, 4.0)
    res[key] = None
    with pytest.raises(ValueError, match=key):
        splat_regularizers(res, 2.0, 4.0)


@pytest.mark.parametrize("key,shape", [("pos", (2, 4, 5, 2)), ("pos", (2, 20, 3)), ("normal", (2, 4, 6, 3)),
                                       ("normal", (3, 4, 5, 3)), ("depth", (2, 4, 5, 1)), ("depth", (2, 5, 4)),
                                       ("image", (2, 4, 5, 4)), ("image", (4, 5, 3))])
def test_shapes_that_disagree(key, shape):
    res = _res()
    res[key] = torch.zeros(shape)
    with pytest.raises(ValueError, match="pos|normal|depth|image"):
        splat_regularizers(res, 2.0, 4.0)


@pytest.mark.parametrize("B", [2, 0])
@pytest.mark.parametrize("H,W", [(1, 5), (5, 1), (1, 1)])
def test_a_grid_reflection_cannot_pad(B, H, W):
    with pytest.raises(ValueError, match="2 x 2"):
        splat_regularizers(_res(B, H, W), 2.0, 4.0)


def test_image_must_have_three_or_four_axes():
    res = {k: v[0, 0] for k, v in _res().items()}
    with pytest.raises(ValueError, match="image"):
        splat_regularizers(res, 2.0, 4.0)
    res = _res()
    res = {k: v[None] for k, v in res.items()}
    with pytest.raises(ValueError, match="image"):
        splat_regularizers(res, 2.0, 4.0)


def test_z_min_above_z_max():
    with pytest.raises(ValueError, match="z_min"):
        splat_regularizers(_res(), 4.0, 2.0)
    with pytest.raises(ValueError, match="z_min"):
        splat_regularizers(_res(), float("nan"), 2.0)


@pytest.mark.parametrize("key", ["pos", "normal", "image", "depth"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.bool, torch.uint8])
def test_a_non_float_input(key, dtype):
    res = _res()
    res[key] = res[key].to(dtype)
    with pytest.raises(ValueError, match="floating"):
        splat_regularizers(res, 2.0, 4.0)
    res[key] = np.zeros(tuple(res[key].shape), dtype=np.int64)
    with pytest.raises(ValueError, match="floating"):
        splat_regularizers(res, 2.0, 4.0)


def test_an_empty_batch():
    with pytest.raises(ValueError, match="empty"):
        splat_regularizers({k: v[:0] for k, v in _res().items()}, 2.0, 4.0)


def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for dtype in (torch.float32, torch.float64, torch.float16):
        with pytest.raises(RuntimeError, match="GPU"):
            splat_regularizers(_res(dtype=dtype), 2.0, 4.0)
    with pytest.raises(RuntimeError, match="GPU"):
        splat_regularizers(_res(B=0), 2.0, 2.0)
