"""GPU: depth_to_surfels (srh_depth_to_surfels_fwd / _bwd) against the fp64 restatement tests/surfels_oracle.py on the
same fp32 inputs and the same (numpy) pixel grid; tests/test_surfels_oracle_cpu.py ties that to the reference's own
function (tests/golden/surfels/sf1_*.npz) and bounds the difference between the two grids.

Stated tolerances: the kernels compute the restatement's fp64 arithmetic and store fp32 once, so every coordinate and
every gradient entry is held to its own bound |got - ref| <= 2^-24 |ref| + 2^-40 A + 2^-149, A the restatement's sum of
the magnitudes of the entry's terms (tests/entry_checks.py, surfels_oracle.magnitudes).  The same arithmetic in float32
does not meet that bound (tests/test_entry_checks_cpu.py).  The older array-scale comparison stays beside it: rtol 2e-6
with atol 2e-7 max(|want|, 1) for values and 2e-7 max|want| for the gradient (projection_checks).  Where depth <= 0 the
point is the eye and the gradient exactly 0."""
import numpy as np
import pytest
import torch

import entry_checks as ec
import surfels_cases as cases
from entry_checks import to_np
from projection_checks import assert_bit_identical, compare_grads, compare_values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hip(c, depth=None, wrt=True):
    """({'pos': [B, N, 3]}, {'depth': gradient or None}) of a case from the GPU."""
    from surf_renderer_amd import depth_to_surfels
    B, H, W = c["shape"]
    d = torch.tensor(c["depth"], device=DEV, requires_grad=wrt) if depth is None else depth
    pos = depth_to_surfels(d, c["camera"], frame=c["frame"])
    assert pos.shape == (B, H * W, 3) and pos.dtype == torch.float32 and pos.device.type == "cuda"
    if d.requires_grad:
        (pos * torch.tensor(c["upstream"]["pos"], device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return {"pos": to_np(pos)}, {"depth": to_np(d.grad)}


@pytest.mark.parametrize("name,variant", cases.ALL)
def test_values_and_gradients_match_the_restatement(name, variant):
    c = cases.case(name, variant)
    got, got_g = _hip(c)
    want, want_g = cases.expected(name, variant)
    A, A_g, _ = cases.magnitudes(name, variant)
    ec.check_all(got, want, A, cases.tag(name, variant) + " values")
    ec.check_all(got_g, want_g, A_g, cases.tag(name, variant) + " gradients")
    compare_values(got, want, cases.tag(name, variant))
    compare_grads(got_g, want_g, cases.tag(name, variant))
    dead = c["depth"] <= 0
    assert np.all(got_g["depth"][dead] == 0)
    if dead.any() and c["frame"] == "world":                 # the point is the eye, in the fp32 it was given in
        B, H, W = c["shape"]
        eye = np.broadcast_to(np.asarray(c["camera"]["eye"], np.float64)[:, None, :3], (B, H * W, 3))
        assert np.array_equal(got["pos"][dead.reshape(B, H * W)], eye[dead.reshape(B, H * W)])


def test_no_input_requires_grad():
    got, got_g = _hip(cases.case("17x9"), wrt=False)
    ec.check_all(got, cases.expected("17x9")[0], cases.magnitudes("17x9")[0], "17x9 forward only")
    compare_values(got, cases.expected("17x9")[0], "17x9 forward only")
    assert got_g["depth"] is None


@pytest.mark.parametrize("name", ["12x16", "36x48"])
def test_two_runs_are_bit_identical(name):
    c = cases.case(name)
    assert_bit_identical(_hip(c), _hip(c))


@pytest.mark.parametrize("name", ["12x16", "17x9"])
def test_a_batch_equals_its_views_bit_for_bit(name):
    c = cases.case(name)
    whole = _hip(c)
    for b in range(c["shape"][0]):
        one = dict(c, depth=c["depth"][b:b + 1], shape=(1, *c["shape"][1:]),
                   upstream={"pos": c["upstream"]["pos"][b:b + 1]},
                   camera=dict(c["camera"], **{k: c["camera"][k][b:b + 1] for k in ("eye", "at", "up")}))
        assert_bit_identical(whole, _hip(one), slice(b, b + 1))


def test_every_shape_of_depth_gives_the_same_surfels_and_a_gradient_of_its_own_shape():
    c = cases.case("12x16")
    B, H, W = c["shape"]
    want = None
    for shape in ((B, H * W), (B, H, W), (B, H, W, 1)):
        d = torch.tensor(c["depth"].reshape(shape), device=DEV, requires_grad=True)
        got = _hip(c, depth=d)
        assert d.grad.shape == shape
        got[1]["depth"] = got[1]["depth"].reshape(B, H * W)
        want = want or got
        assert_bit_identical(want, got)


def test_outputs_are_overwritten_not_accumulated(monkeypatch):
    """The kernels write every element: with torch.empty handing out NaN-filled buffers the results do not change."""
    c = cases.case("36x48")
    want = _hip(c)
    empty, empty_like = torch.empty, torch.empty_like

    def nan_filled(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(123)

    monkeypatch.setattr(torch, "empty", lambda *a, **k: nan_filled(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: nan_filled(empty_like(*a, **k)))
    assert_bit_identical(want, _hip(c))


def test_float64_and_cpu_inputs_are_converted_and_the_gradient_comes_back_in_the_leafs_own():
    c = cases.case("12x16")
    want, want_g = cases.expected("12x16")
    for leaf in (torch.tensor(c["depth"].astype(np.float64), device=DEV, requires_grad=True),        # fp64 GPU leaf
                 torch.tensor(c["depth"].astype(np.float64), requires_grad=True),                    # fp64 CPU leaf
                 torch.tensor(np.ascontiguousarray(c["depth"].transpose(0, 2, 1, 3)), device=DEV,
                              requires_grad=True)):                                                  # not contiguous
        d = leaf.permute(0, 2, 1, 3) if leaf.dtype == torch.float32 else leaf
        camera = dict(c["camera"], eye=torch.tensor(c["camera"]["eye"], dtype=torch.float64),
                      at=torch.tensor(c["camera"]["at"], device=DEV))
        from surf_renderer_amd import depth_to_surfels
        pos = depth_to_surfels(d, camera)
        (pos * torch.tensor(c["upstream"]["pos"], device=DEV)).sum().backward()
        assert pos.device.type == "cuda" and pos.dtype == torch.float32
        assert leaf.grad.dtype == leaf.dtype and leaf.grad.device == leaf.device and leaf.grad.shape == leaf.shape
        grad = leaf.grad.permute(0, 2, 1, 3) if leaf.dtype == torch.float32 else leaf.grad
        A, A_g, _ = cases.magnitudes("12x16")
        ec.check_all({"pos": to_np(pos)}, want, A, "12x16 converted values")
        ec.check_all({"depth": ec.narrowed(to_np(grad))}, want_g, A_g, "12x16 converted gradients")
        compare_values({"pos": to_np(pos)}, want, "12x16 converted")
        compare_grads({"depth": to_np(grad)}, want_g, "12x16 converted")


def test_the_camera_frame_places_the_points_where_render_splats_along_ray_does():
    """frame='camera' against the `pos` output of render_splats_along_ray for the same z, K = 1 and given normals: both
    use the same grid, so the two agree within the stated tolerance."""
    from surf_renderer_amd import depth_to_surfels, render_splats_along_ray
    c = cases.case("12x16", "camera")
    B, H, W = c["shape"]
    depth = torch.tensor(c["depth"], device=DEV)
    pos = depth_to_surfels(depth, c["camera"], frame="camera")
    for b in range(B):
        z = -depth[b].reshape(H * W)
        normal = torch.zeros(H * W, 3, device=DEV)
        normal[:, 2] = 1.0
        cam = {"eye": c["camera"]["eye"][b], "at": c["camera"]["at"][b], "up": c["camera"]["up"][b],
               "viewport": c["camera"]["viewport"], "fovy": c["camera"]["fovy"],
               "focal_length": c["camera"]["focal_length"], "proj_type": "perspective"}
        scene = {"camera": cam, "lights": {"pos": torch.tensor([[0.0, 0.0, 4.0, 1.0]], device=DEV),
                                            "color_idx": torch.tensor([0]), "attenuation": torch.tensor([[1.0, 0.0, 0.0]]),
                                            "ambient": torch.tensor([0.1, 0.1, 0.1])},
                 "colors": torch.tensor([[1.0, 1.0, 1.0]]),
                 "materials": {"albedo": torch.tensor([[0.5, 0.5, 0.5]]), "coeffs": torch.tensor([[1.0, 0.0, 0.0]])},
                 "objects": {"disk": {"pos": z, "normal": normal,
                                      "material_idx": torch.zeros(H * W, dtype=torch.long)}}}
        res = render_splats_along_ray(scene, samples=1)
        want = {"pos": to_np(res["pos"]).reshape(1, H * W, 3)}
        compare_values({"pos": to_np(pos[b:b + 1])}, want, f"12x16 view {b} against the splat renderer")
