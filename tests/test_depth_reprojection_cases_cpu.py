"""The conditions on the seeded cases of tests/depth_reprojection_cases.py, which are what lets tests/
test_hip_depth_reprojection.py compare every element, and the identity property in the fp64 restatements themselves:
lifted on either grid and projected back by the hard projection, every surfel lands on its own pixel."""
import numpy as np
import pytest
import torch

import depth_reprojection_cases as cases
import hard_projection_oracle as ho
import projection_oracle as po
import surfels_oracle as so


@pytest.mark.parametrize("grid", ["numpy", "torch"])
@pytest.mark.parametrize("name", list(cases.IDENTITY))
def test_the_restatements_meet_the_identity(name, grid):
    c = cases.identity(name)
    B, H, W = c["shape"]
    assert np.all(c["depth"] >= 1.5)
    surfels = so.lift(torch.tensor(c["depth"].astype(np.float64)), c["camera"], grid=grid).float().double()
    res = ho.project(surfels, torch.tensor(c["rgb"].astype(np.float64)), c["camera"])
    assert np.array_equal(res["index"].numpy(), np.broadcast_to(np.arange(H * W), (B, H * W)))
    assert not res["mask"].any() and np.array_equal(res["out"].numpy(), c["rgb"].astype(np.float64))
    # and by a wide margin: the coordinates are within 1e-3 of the pixel centres, 0.5 from the nearest tie
    px = po.pixel_coordinates(surfels, c["camera"]).numpy()[..., :2].reshape(B, H, W, 2)
    centres = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), axis=-1)
    assert np.abs(px - centres).max() <= 1e-3


def test_the_end_to_end_draw_is_clear_of_every_kink_and_reaches_every_output():
    c = cases.end_to_end()
    assert po.decision_margin(cases.lifted(c), c["rgb"], c["camera2"], None, cases.BLUR_SIZE, **cases.FLAGS) >= 1.0
    assert set(c["upstream"]) == set(po.OUTPUTS)
    assert not np.array_equal(c["camera1"]["eye"], c["camera2"]["eye"])
    want, want_g = cases.end_to_end_expected()
    assert set(want) == set(po.OUTPUTS) and want_g.shape == c["depth"].shape
    # most pixels stay in the second camera's frame and get a gradient; those that leave it get exactly 0
    assert np.all(np.isfinite(want_g)) and 0.5 < (want_g != 0).mean() < 1.0
