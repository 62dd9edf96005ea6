"""nearest_points, hausdorff and hausdorff_batched refuse what the kernels could not index, with ValueError and before
anything reaches the GPU (none is needed here); the names are exported."""
import numpy as np
import pytest
import torch

import surf_renderer_amd
from surf_renderer_amd import pointsets


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


BIG = torch.empty((1 << 24) + 1, 1)          # one point too many; never read


def test_the_names_are_exported():
    for name in ("nearest_points", "hausdorff", "hausdorff_batched"):
        assert name in surf_renderer_amd.__all__ and getattr(surf_renderer_amd, name) is getattr(pointsets, name)


@pytest.mark.parametrize("u,v,shown", [
    (None, z(4, 3), "u is missing"), (z(4, 3), None, "v is missing"),
    (z(4, 3, dtype=torch.int64), z(4, 3), "u has dtype"), (z(4, 3), np.zeros((4, 3), np.int32), "v has dtype"),
    (z(3), z(4, 3), r"u is \[3\]"), (z(2, 2, 4, 3), z(2, 4, 3), "u is"), (z(4, 3), z(1, 1, 4, 3), "v is"),
    (z(4, 3), z(1, 4, 3), "batch"), (z(2, 4, 3), z(3, 4, 3), "2 views and v has 3"),
    (z(4, 3), z(4, 2), "3 columns and v has 2"), (z(2, 4, 3), z(2, 5, 4), "columns"),
    (z(4, 0), z(4, 0), "0 columns"), (z(4, 5), z(4, 5), "5 columns"),
    (z(0, 3), z(4, 3), "u has 0 points"), (z(2, 4, 3), z(2, 0, 3), "v has 0 points"),
    (BIG, z(4, 1), "u has 16777217 points"), (z(1, 4, 1), BIG[None], "v has 16777217"),
    (z(65536, 2, 3), z(65536, 2, 3), "65536 views"), (z(0, 4, 3), z(0, 4, 3), "0 views"),
])
def test_nearest_points_refuses(u, v, shown):
    with pytest.raises(ValueError, match="nearest_points: .*" + shown):
        pointsets.nearest_points(u, v)


def test_the_hausdorff_calls_insist_on_their_rank_and_name_themselves():
    with pytest.raises(ValueError, match=r"hausdorff: u is \[2, 4, 3\], expected \[N, D\]"):
        pointsets.hausdorff(z(2, 4, 3), z(2, 4, 3))
    with pytest.raises(ValueError, match=r"hausdorff_batched: u is \[4, 3\], expected \[B, N, D\]"):
        pointsets.hausdorff_batched(z(4, 3), z(4, 3))
    with pytest.raises(ValueError, match="hausdorff: .*5 columns"):
        pointsets.hausdorff(z(4, 5), z(4, 5))
    with pytest.raises(ValueError, match="hausdorff_batched: .*v has 0 points"):
        pointsets.hausdorff_batched(z(1, 4, 3), z(1, 0, 3))


def test_a_valid_call_gets_as_far_as_the_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        pointsets.nearest_points(z(4, 3), np.zeros((5, 3)))
