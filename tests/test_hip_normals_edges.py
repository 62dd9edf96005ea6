"""GPU: the plane-fit layer on the edge inputs of tests/normals_edge_cases.py against the fp64 restatement tests/
normals_oracle.py; tests/test_normals_edge_cases_cpu.py shows that each case reaches the branch it is named for.  Then the
chain depth -> depth_to_surfels -> normals -> a weighted sum, against the two restatements chained under autograd.

Stated tolerances, those of tests/test_hip_normals.py: every element within 2^-24 |ref| + NORMALS_C64 max|ref| + 2^-149
of the restatement (entry_checks.check_plane_fit), and beside it normals rtol 2e-6 with atol 2e-7 max(|want|, 1), pos.grad
rtol 2e-6 with atol 2e-7 max|want|.  In the three cases with a special point an element is non-finite exactly where the
restatement's is -- a NaN where it is a NaN, the same infinity where it is one -- and every other element is held to the
same bounds (max|want| over the finite elements).  The chain's depth gradient is a sum of the two layers' terms through a
float32 hand-over and keeps the array-scale tolerance."""
import numpy as np
import pytest
import torch

import entry_checks as ec
import normals_edge_cases as edges
import normals_oracle as no
import surfels_oracle as so
from entry_checks import to_np
from projection_checks import ATOL_SCALE, RTOL, assert_bit_identical, compare_grads, compare_values, one_view
from test_hip_normals import DEV, _hip

pytestmark = pytest.mark.gpu

ORDINARY = [n for n in edges.NAMES if n not in edges.SPECIAL]


@pytest.mark.parametrize("name", ORDINARY)
def test_values_and_gradients_match_the_restatement_and_a_batch_equals_its_views(name):
    c = edges.case(name)
    whole = _hip(c)
    want, want_g = edges.expected(name)
    again, again_g = edges.turned(name)
    ec.check_plane_fit(whole[0]["normal"], want["normal"], again["normal"], name + " normal")
    ec.check_plane_fit(whole[1]["pos"], want_g["pos"], again_g["pos"], name + " grad pos")
    compare_values(whole[0], want, name)
    compare_grads(whole[1], want_g, name, nonzero=c["nonzero"])
    if c["shape"][0] > 1 and np.asarray(c["camera"]["eye"]).ndim == 2:
        for b in range(c["shape"][0]):
            assert_bit_identical(whole, _hip(one_view(c, b, ("pos",))), slice(b, b + 1))


def test_a_shared_camera_equals_the_same_camera_given_per_view_bit_for_bit():
    c = edges.case("world_shared_6x5")
    per_view = dict(c, camera=dict(c["camera"], **{k: np.tile(c["camera"][k], (2, 1)) for k in ("eye", "at", "up")}))
    assert_bit_identical(_hip(c), _hip(per_view))
    hom = dict(c, camera=dict(c["camera"], eye=np.append(c["camera"]["eye"], 1.0).astype(np.float32),
                              up=np.append(c["camera"]["up"], 0.0).astype(np.float32)))
    assert_bit_identical(_hip(c), _hip(hom))


def test_a_constant_patch_faces_the_camera():
    got, got_g = _hip(edges.case("constant_4x4"))
    assert np.all(got["normal"][..., :2] == 0) and np.all(got["normal"][..., 2] == np.float32(1.0 / np.sqrt(1.0 + 3e-10)))
    assert np.all(got_g["pos"] == 0)


@pytest.mark.parametrize("name", list(edges.SPECIAL))
def test_a_special_point_spoils_its_reach_and_nothing_else(name):
    c = edges.case(name)
    got, got_g = _hip(c)
    want, want_g = edges.expected(name)
    again, again_g = edges.turned(name)
    ec.check_plane_fit(got["normal"], want["normal"], again["normal"], name + " normal")
    ec.check_plane_fit(got_g["pos"], want_g["pos"], again_g["pos"], name + " grad pos")
    for tag, g, w, floor in (("normal", got["normal"], want["normal"], 1.0), ("grad pos", got_g["pos"], want_g["pos"], 0.0)):
        finite = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), finite), (name, tag, np.argwhere(np.isfinite(g) != finite))
        scale = max(np.abs(w[finite]).max(), floor)
        print(f"{name} {tag}: {finite.sum()} finite elements, max err {np.abs(g[finite] - w[finite]).max():.3g}, scale {scale:.3g}")
        np.testing.assert_allclose(g[finite], w[finite], rtol=RTOL, atol=ATOL_SCALE * scale, err_msg=f"{name} {tag}")
    # the corner's NaN upstream gradient reaches nothing that does not depend on it: without it, the other elements are
    # the same bit for bit
    clean = dict(c, upstream={"normal": np.where(np.isnan(c["upstream"]["normal"]), np.float32(0.5), c["upstream"]["normal"])})
    _, clean_g = _hip(clean)
    far = ~np.broadcast_to(edges.reach(edges.CORNER, 1)[None, :, :, None], got_g["pos"].shape)
    assert np.array_equal(got_g["pos"][far], clean_g["pos"][far], equal_nan=True)


@pytest.mark.parametrize("name", ["wide_2x300", "tall_300x2"])
def test_outputs_are_overwritten_not_accumulated(name, monkeypatch):
    """The kernels write every element: with torch.empty handing out NaN-filled buffers the results do not change."""
    c = edges.case(name)
    want = _hip(c)
    empty, empty_like = torch.empty, torch.empty_like

    def nan_filled(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(255)

    monkeypatch.setattr(torch, "empty", lambda *a, **k: nan_filled(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: nan_filled(empty_like(*a, **k)))
    got = _hip(c)
    assert np.all(np.isfinite(got[0]["normal"])) and np.all(np.isfinite(got[1]["pos"]))
    assert_bit_identical(want, got)


# ---- depth -> surfels -> normals ------------------------------------------------------------------------------------
def _chain_case():
    """B = 2 views of 12 x 16: depth = 3 + smooth + noise as in normals_cases, with a twelfth of the depths 0 or negative
    (they lift to the origin, several of them side by side); weights for the normals and the positions."""
    import normals_cases as nc
    import projection_cases as pc
    B, H, W = 2, 12, 16
    rng = np.random.RandomState(9200)
    eye, at, up = pc.draw_camera(rng, B)
    depth = nc.draw_depth(rng, B, H, W)
    for b in range(B):
        bad = rng.permutation(H * W)[:H * W // 12]
        depth[b].reshape(-1)[bad[0::2]] = 0.0
        depth[b].reshape(-1)[bad[1::2]] = -rng.uniform(0.5, 1.5, len(bad[1::2]))
    depth[0, 5, 7:9] = 0.0                                   # two dead neighbours: a zero-length difference at the origin
    return {"depth": pc.f32(depth), "shape": (B, H, W),
            "camera": {"eye": eye, "at": at, "up": up, "viewport": [0, 0, W, H], "fovy": float(pc.FOVY), "focal_length": pc.FOCAL},
            "w_normal": pc.f32(rng.uniform(-1, 1, (B, H * W, 3))), "w_pos": pc.f32(rng.uniform(-1, 1, (B, H * W, 3)))}


def _chain_expected(c, frame):
    """The two fp64 restatements chained under autograd.  The layers hand the points over as float32 -- one store per
    element -- so the chain does too, with the rounding's gradient the identity (as tests/depth_reprojection_cases.py's
    end_to_end_expected does, which says why)."""
    depth = torch.tensor(c["depth"].astype(np.float64), requires_grad=True)
    pos = so.lift(depth, c["camera"], frame="camera")
    pos = pos + (pos.float().double() - pos).detach()
    normal = no.plane_fit(pos, c["camera"], frame)
    loss = (normal * torch.tensor(c["w_normal"].astype(np.float64))).sum() + (pos * torch.tensor(c["w_pos"].astype(np.float64))).sum()
    loss.backward()
    return {"pos": pos.detach().numpy(), "normal": normal.detach().numpy()}, {"depth": depth.grad.numpy()}


@pytest.mark.parametrize("frame", ["camera", "world"])
def test_a_loss_on_normals_and_positions_reaches_the_depth_map(frame):
    from surf_renderer_amd import depth_to_surfels, estimate_surface_normals_plane_fit_batched
    c = _chain_case()
    assert (c["depth"] <= 0).sum() >= 30
    depth = torch.tensor(c["depth"], device=DEV, requires_grad=True)
    pos = depth_to_surfels(depth, c["camera"], frame="camera")
    normal = estimate_surface_normals_plane_fit_batched(pos, camera=c["camera"], frame=frame)
    assert normal.shape == pos.shape == (2, 12 * 16, 3)
    ((normal * torch.tensor(c["w_normal"], device=DEV)).sum() + (pos * torch.tensor(c["w_pos"], device=DEV)).sum()).backward()
    torch.cuda.synchronize()
    want, want_g = _chain_expected(c, frame)
    tag = f"depth -> surfels -> normals ({frame})"
    assert np.all(np.isfinite(to_np(normal))) and np.all(np.isfinite(to_np(depth.grad)))
    A_pos = so.magnitudes({"depth": c["depth"]}, c["camera"], {"pos": c["w_pos"]}, "camera")[0]["pos"]
    exact = so.lift(torch.tensor(c["depth"].astype(np.float64)), c["camera"], frame="camera").numpy()    # before the hand-over's rounding
    ec.check_all({"pos": to_np(pos)}, {"pos": exact}, {"pos": A_pos}, tag + " pos")
    again = no.turned_gradients({"pos": want["pos"]}, c["camera"], {"normal": c["w_normal"]}, frame, c["shape"])[0]
    ec.check_plane_fit(to_np(normal), want["normal"], again["normal"], tag + " normal")
    compare_values({"pos": to_np(pos), "normal": to_np(normal)}, want, tag)
    assert depth.grad.shape == depth.shape
    compare_grads({"depth": to_np(depth.grad)}, want_g, tag)
    assert np.all(to_np(depth.grad)[c["depth"] <= 0] == 0)
