"""CPU: tests/dense_camera_oracle.py tied down.

  - with the camera detached it gives exactly (bit for bit) what dense_projection_oracle and normals_oracle give, values
    and gradients, on every seeded case of dense_projection_cases and normals_cases;
  - its camera gradients are those of central differences in fp64;
  - for the normals g_eye = -g_at to fp64 rounding: z depends on eye - at only, and the rotation on nothing else of them.

Central differences: step h = 1e-6 on entries of order 1 gives a truncation error of order h^2 = 1e-12 and a rounding
error of order 1e-16 / h = 1e-10 relative to the loss; the gradients are compared at 1e-6 of the camera's largest
gradient entry, four orders above both."""
import numpy as np
import pytest
import torch

import dense_camera_oracle as dco
import dense_projection_cases as dc
import dense_projection_oracle as do
import normals_cases as nc
import normals_oracle as no

H_STEP, FD_TOL = 1e-6, 1e-6
FD_DENSE = [("2x2", "grid", False), ("3x5", "flat", True), ("12x16", "grid", True), ("17x9", "grid", False)]
FD_NORMALS = ["2x2", "3x5", "17x9"]


def _same(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        assert np.array_equal(a[k], b[k]), (tag, k)


@pytest.mark.parametrize("frame,layout,rotated", dc.ALL)
def test_detached_the_dense_restatement_is_the_layers_own_oracle(frame, layout, rotated):
    c = dc.case(frame, layout, rotated)
    want, want_g = dc.expected(frame, layout, rotated)
    got, got_g, _ = dco.project_gradients(dc.inputs(c), c["camera"], c["upstream"], c["blur_size"], camera_wrt=())
    _same(got, want, dc.tag(frame, layout, rotated))
    _same(got_g, want_g, dc.tag(frame, layout, rotated))


def test_the_separable_form_takes_camera_leaves_too():
    c = dc.case("12x16", "grid", True)
    a = dco.project_gradients(dc.inputs(c), c["camera"], c["upstream"], c["blur_size"])
    b = dco.project_gradients(dc.inputs(c), c["camera"], c["upstream"], c["blur_size"], fn=do.project_separable)
    for k, g in a[2]["camera"].items():
        np.testing.assert_allclose(b[2]["camera"][k], g, rtol=1e-9, atol=1e-12 * np.abs(g).max())


@pytest.mark.parametrize("name,variant", nc.ALL)
@pytest.mark.parametrize("frame", ["camera", "world"])
def test_detached_the_normals_restatement_is_the_layers_own_oracle(name, variant, frame):
    c = nc.case(name, variant)
    want, want_g = no.gradients({"pos": c["pos"]}, c["camera"], c["upstream"], frame)
    got, got_g, _ = dco.normals_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], frame, camera_wrt=())
    _same(got, want, (name, variant, frame))
    _same(got_g, want_g, (name, variant, frame))


def _central_differences(loss, camera):
    """{entry: d loss / d entry} by central differences over every element of eye, at and up."""
    out = {}
    for k in dco.CAMERA_KEYS:
        base = np.asarray(camera[k], dtype=np.float64)
        g = np.zeros_like(base)
        for idx in np.ndindex(*base.shape):
            lo, hi = base.copy(), base.copy()
            lo[idx] -= H_STEP
            hi[idx] += H_STEP
            g[idx] = (loss(dict(camera, **{k: hi})) - loss(dict(camera, **{k: lo}))) / (2 * H_STEP)
        out[k] = g
    return out


def _compare_with_differences(got, fd, tag):
    top = max(np.abs(g).max() for g in got.values())
    assert top > 0, tag
    for k in dco.CAMERA_KEYS:
        err = np.abs(got[k] - fd[k]).max() / top
        print(f"{tag} {k}: {err:.3g}")
        assert err <= FD_TOL, (tag, k, err)


@pytest.mark.parametrize("frame,layout,rotated", FD_DENSE)
def test_the_dense_camera_gradients_are_those_of_central_differences(frame, layout, rotated):
    c = dc.case(frame, layout, rotated)
    x = {k: (None if c[k] is None else torch.as_tensor(c[k].astype(np.float64))) for k in do.INPUTS}
    ups = {k: torch.as_tensor(u.astype(np.float64)) for k, u in c["upstream"].items()}

    def loss(camera):
        res = dco.project(x["surfels"], x["rgb"], camera, x["rotated_image"], c["blur_size"])
        return float(sum((res[k] * ups[k]).sum() for k in ups))

    got = dco.project_gradients(dc.inputs(c), c["camera"], c["upstream"], c["blur_size"])[2]["camera"]
    _compare_with_differences(got, _central_differences(loss, c["camera"]), dc.tag(frame, layout, rotated))


@pytest.mark.parametrize("name", FD_NORMALS)
@pytest.mark.parametrize("shared", [False, True])
def test_the_normals_camera_gradients_are_those_of_central_differences(name, shared):
    c = nc.case(name)
    camera = dict(c["camera"], **{k: c["camera"][k][0] for k in dco.CAMERA_KEYS}) if shared else c["camera"]
    pos, up = torch.as_tensor(c["pos"].astype(np.float64)), torch.as_tensor(c["upstream"]["normal"].astype(np.float64))

    def loss(cam):
        return float((dco.plane_fit(pos, cam, "world") * up).sum())

    got = dco.normals_gradients({"pos": c["pos"]}, camera, c["upstream"], "world")[2]["camera"]
    for k in dco.CAMERA_KEYS:
        assert got[k].shape == np.asarray(camera[k]).shape
    _compare_with_differences(got, _central_differences(loss, camera), f"normals {name} shared={shared}")


@pytest.mark.parametrize("name,variant", nc.ALL)
def test_the_normals_eye_gradient_is_minus_the_at_gradient(name, variant):
    c = nc.case(name, variant)
    cam = dco.normals_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], "world")[2]["camera"]
    top = np.abs(cam["eye"]).max()
    assert top > 0
    assert np.abs(cam["eye"] + cam["at"]).max() <= 1e-14 * top, np.abs(cam["eye"] + cam["at"]).max() / top


def test_the_camera_frame_gives_the_camera_nothing():
    c = nc.case("12x16")
    cam = dco.normals_gradients({"pos": c["pos"]}, c["camera"], c["upstream"], "camera")[2]["camera"]
    assert all(not np.any(g) for g in cam.values())
