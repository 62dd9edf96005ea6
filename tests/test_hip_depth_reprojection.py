"""GPU: depth_to_surfels chained with the projection layers (tests/depth_reprojection_cases.py).

Identity, the reference's headline property: a depth map lifted and projected back into the same camera by
projection_renderer returns the image bit for bit with a mask that is False everywhere -- every surfel lands on its own
pixel, and a mean over one value is that value.

End to end: a depth leaf -> depth_to_surfels -> projection_renderer_differentiable_fast into a second camera
(compute_new_depth) -> a weighted sum over every output; depth.grad against the two fp64 restatements chained under
autograd, with the float32 hand-over of the surfels between them that the layers have (depth_reprojection_cases.
end_to_end_expected says why), under the layers' stated tolerances (projection_checks)."""
import numpy as np
import pytest
import torch

import depth_reprojection_cases as cases
from projection_checks import compare_grads, compare_values, to_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(cases.IDENTITY))
def test_a_lifted_depth_map_projects_back_onto_its_own_pixels(name):
    from surf_renderer_amd import depth_to_surfels, projection_renderer
    c = cases.identity(name)
    rgb = torch.tensor(c["rgb"], device=DEV, requires_grad=True)
    out, mask = projection_renderer(depth_to_surfels(torch.tensor(c["depth"], device=DEV), c["camera"]), rgb, c["camera"])
    assert out.shape == mask.shape == rgb.shape
    assert not mask.any().item()
    assert torch.equal(out, rgb.detach())
    upstream = torch.rand(out.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    (out * upstream).sum().backward()
    assert torch.equal(rgb.grad, upstream)               # one surfel per pixel: the gradient comes back as it went in


def test_a_loss_on_a_reprojected_view_reaches_the_depth_map():
    from surf_renderer_amd import depth_to_surfels, projection_renderer_differentiable_fast
    c = cases.end_to_end()
    depth = torch.tensor(c["depth"], device=DEV, requires_grad=True)
    surfels = depth_to_surfels(depth, c["camera1"])
    out, proj_out = projection_renderer_differentiable_fast(surfels, torch.tensor(c["rgb"], device=DEV), c["camera2"],
                                                            blur_size=cases.BLUR_SIZE, **cases.FLAGS)
    res = dict(proj_out, out=out)
    sum((res[k] * torch.tensor(g, device=DEV)).sum() for k, g in c["upstream"].items()).backward()
    torch.cuda.synchronize()
    want, want_g = cases.end_to_end_expected()
    compare_values({k: to_np(v) for k, v in res.items()}, want, "depth -> surfels -> projection")
    assert depth.grad.shape == depth.shape
    compare_grads({"depth": to_np(depth.grad)}, {"depth": want_g}, "depth -> surfels -> projection")
    assert np.all(np.isfinite(to_np(surfels)))
