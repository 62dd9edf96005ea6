"""CPU: tests/camera_chain_oracle.py, the restatement with camera leaves that the GPU tests of camera_grad=True compare
with.  With the camera detached it must give EXACTLY what surfels_oracle, projection_oracle and
reverse_projection_oracle give, values and gradients, on every seeded case: it restates only the camera path, in their
order of operations.  With camera leaves the values and the other gradients do not move either, a leaf the loss cannot
reach gets exactly zero, and the camera gradient agrees with a central difference of the same fp64 function."""
import numpy as np
import pytest
import torch

import camera_chain_oracle as co
import projection_cases as pc
import projection_oracle as po
import reverse_projection_cases as rc
import surfels_cases as sc


def _same(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        assert np.array_equal(a[k], b[k]), (tag, k)


def _lift(c, camera_wrt):
    return co.lift_gradients({"depth": c["depth"]}, c["camera"], c["upstream"], c["frame"], camera_wrt=camera_wrt)


def _project(c, camera_wrt):
    return co.project_gradients(pc.inputs(c), c["camera"], c["upstream"], c["blur_size"], camera_wrt=camera_wrt,
                                **c["flags"])


def _reverse(c, camera_wrt):
    ups = c["upstream"] if c["only"] is None else {c["only"]: c["upstream"][c["only"]]}
    return co.reverse_gradients(rc.inputs(c), c["camera1"], c["camera2"], ups, wrt=c["wrt"], camera_wrt=camera_wrt,
                                **c["flags"])


LAYERS = {"lift": (sc, _lift), "projection": (pc, _project), "reverse": (rc, _reverse)}
EVERY = [(layer, n, v) for layer, (m, _) in LAYERS.items() for n, v in m.ALL]


@pytest.mark.parametrize("layer,name,variant", EVERY)
def test_detached_it_is_the_existing_oracle_exactly_and_camera_leaves_move_nothing_else(layer, name, variant):
    cases, run = LAYERS[layer]
    c = cases.case(name, variant)
    want, want_g = cases.expected(name, variant)
    tag = f"{layer} {cases.tag(name, variant)}"
    got, got_g, cam_g = run(c, ())
    _same(got, want, tag)
    _same(got_g, want_g, tag)
    assert all(g == {} for g in cam_g.values())
    got, got_g, cam_g = run(c, co.CAMERA_KEYS)
    _same(got, want, tag + " with camera leaves")
    _same(got_g, want_g, tag + " with camera leaves")
    for label, g in cam_g.items():
        for k in co.CAMERA_KEYS:
            assert g[k].shape == np.asarray(c[label][k]).shape and np.all(np.isfinite(g[k])), (tag, label, k)
            if g[k].shape[1] == 4:                       # w is dropped before lookat
                assert np.all(g[k][:, 3] == 0), (tag, label, k)


def test_what_a_camera_cannot_reach_gets_exactly_zero():
    c = sc.case("12x16", "camera")                        # the camera frame does not read eye / at / up
    assert all(np.all(g == 0) for g in _lift(c, co.CAMERA_KEYS)[2]["camera"].values())
    c = rc.case("12x16", "no_depth")                      # camera2 enters through the values of the new depth alone
    g = _reverse(c, co.CAMERA_KEYS)[2]
    assert all(np.all(v == 0) for v in g["camera2"].values())
    assert all(np.abs(v).max() > 0 for v in g["camera1"].values())


@pytest.mark.parametrize("layer,name", [("lift", "3x5"), ("projection", "3x5"), ("reverse", "3x5")])
def test_the_camera_gradient_is_the_derivative_of_the_function(layer, name):
    """Central differences of the fp64 loss in every camera component, step 1e-6: the cases stay clear of every kink by
    1e-4 pixels, and the truncation and rounding errors of the quotient are far below the 1e-5 relative bound.  The scale
    is the camera's, not the entry's: camera2['up'] of the reverse layer cannot reach the loss (row 2 of the matrix is
    unit(eye - at)), so its gradient is rounding noise in both."""
    cases, run = LAYERS[layer]
    c = cases.case(name)
    ups = c["upstream"]

    def loss(case):
        values = run(case, ())[0]
        return sum(float(np.sum(values[k] * np.asarray(ups[k], np.float64).reshape(values[k].shape))) for k in ups)

    cam_g = run(c, co.CAMERA_KEYS)[2]
    h = 1e-6
    for label, g in cam_g.items():
        scale = max(np.abs(v).max() for v in g.values())
        assert scale > 0, (layer, label)
        for k in co.CAMERA_KEYS:
            num = np.zeros_like(g[k])
            for idx in np.ndindex(*g[k].shape):
                vals = []
                for s in (h, -h):
                    v = np.asarray(c[label][k], np.float64).copy()
                    v[idx] += s
                    vals.append(loss(dict(c, **{label: dict(c[label], **{k: v})})))
                num[idx] = (vals[0] - vals[1]) / (2 * h)
            assert np.abs(num - g[k]).max() <= 1e-5 * scale, (layer, label, k, num, g[k])


def test_the_chain_composes_the_two():
    """chain_gradients is project(lift(.)): against the two oracles composed by hand."""
    cl, cp = sc.case("12x16"), pc.case("12x16")
    depth = cl["depth"]
    values, g, cam_g = co.chain_gradients(depth, cp["rgb"], cl["camera"], cp["camera"], cp["upstream"]["out"],
                                          cp["blur_size"], round_pos=False)
    d = torch.tensor(np.asarray(depth, np.float64), requires_grad=True)
    out = po.project(co.lift(d, cl["camera"]), torch.as_tensor(np.asarray(cp["rgb"], np.float64)), cp["camera"], None,
                     cp["blur_size"])["out"]
    (out * torch.as_tensor(np.asarray(cp["upstream"]["out"], np.float64))).sum().backward()
    assert np.array_equal(values["out"], out.detach().numpy()) and np.array_equal(g["depth"], d.grad.numpy())
    assert all(np.abs(v).max() > 0 for cam in cam_g.values() for v in cam.values())


def _matrices(camera):
    """(the restatement's world-to-camera and camera-to-world matrices [B, 3, 4], the layers' own) in fp64."""
    from surf_renderer_amd import _camera
    vec = [torch.as_tensor(np.ascontiguousarray(np.asarray(camera[k], np.float64)[:, :3])) for k in co.CAMERA_KEYS]
    R, eye = co.camera_to_world(camera, torch.float64)
    return ((co.world_to_camera(camera, torch.float64)[:, :3, :], torch.cat((R, eye[..., None]), dim=-1)),
            (_camera.view_matrices(*vec), _camera.inverse_view_matrices(*vec)))


def test_the_restatements_matrices_are_the_layers_own_and_fp64_sees_the_epsilon(monkeypatch):
    """The matrices camera_grad=True differentiates through (_camera.view_matrices / inverse_view_matrices, the
    reference's lookat with its 1e-10 under normalize's root) against the restatement's, bit for bit in fp64, for every
    camera of every seeded case.  This is what guards the 1e-10 in the restatement: the float32 fixtures cannot
    (tests/test_camera_warp_golden_cpu.py), fp64 can -- without it the matrices differ."""
    cameras = [m.case(n)[label] for m, labels in ((sc, ("camera",)), (pc, ("camera",)), (rc, ("camera1", "camera2")))
               for n in m.NAMES for label in labels]
    for camera in cameras:
        got, want = _matrices(camera)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    monkeypatch.setattr(po, "_normalize",
                        lambda u: po.nonzero_divide(u, torch.sqrt(torch.sum(u * u, dim=-1, keepdim=True))))
    for camera in cameras:
        got, want = _matrices(camera)
        assert not torch.equal(got[0], want[0]) and not torch.equal(got[1], want[1])
