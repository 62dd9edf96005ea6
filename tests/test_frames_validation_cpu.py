"""Every refusal of world_to_cam[_batched], cam_to_world[_batched], project_surfels and project_image_coordinates: a
ValueError on the host, before the library is loaded (projection_validation.no_library makes it unreachable) and before
anything reaches the GPU, so these run without one."""
import numpy as np
import pytest
import torch

import surf_renderer_amd as sra
from projection_validation import camera, no_library  # noqa: F401  (autouse fixture)

BATCHED = (sra.world_to_cam_batched, sra.cam_to_world_batched)
UNBATCHED = (sra.world_to_cam, sra.cam_to_world)
PROJECTIONS = (sra.project_surfels, sra.project_image_coordinates)
each_batched = pytest.mark.parametrize("fn", BATCHED, ids=lambda f: f.__name__)
each_unbatched = pytest.mark.parametrize("fn", UNBATCHED, ids=lambda f: f.__name__)
each_projection = pytest.mark.parametrize("fn", PROJECTIONS, ids=lambda f: f.__name__)


def views(B=2, hom=False):
    return {k: v for k, v in camera(B, 4, 5, hom=hom).items() if k in ("eye", "at", "up")}


def one_view(hom=False):
    return {k: v[0] for k, v in views(1, hom).items()}


def test_the_six_functions_are_exported():
    for name in ("world_to_cam", "world_to_cam_batched", "cam_to_world", "cam_to_world_batched", "project_surfels",
                 "project_image_coordinates"):
        assert name in sra.__all__ and callable(getattr(sra, name))


@each_batched
@pytest.mark.parametrize("what", ["pos", "normal"])
@pytest.mark.parametrize("shape", [(7, 3), (2, 7), (2, 7, 2), (2, 7, 5), (2, 1, 7, 3)])
def test_points_of_another_rank_or_column_count(fn, what, shape):
    args = {"pos": torch.zeros(2, 7, 3), "normal": torch.zeros(2, 7, 3), what: torch.zeros(shape)}
    with pytest.raises(ValueError, match=what):
        fn(args["pos"], args["normal"], views())


@each_batched
def test_both_inputs_missing(fn):
    with pytest.raises(ValueError, match="both None"):
        fn(None, None, views())


@each_batched
def test_a_batch_mismatch(fn):
    with pytest.raises(ValueError, match="views"):
        fn(torch.zeros(2, 7, 3), torch.zeros(3, 7, 3), views())
    with pytest.raises(ValueError, match="eye"):
        fn(torch.zeros(3, 7, 3), None, views(2))
    with pytest.raises(ValueError, match="eye"):
        fn(None, torch.zeros(1, 7, 4), views(2))


@each_batched
@pytest.mark.parametrize("what", ["pos", "normal"])
def test_an_empty_or_oversized_batch_or_point_count(fn, what):
    for shape, match in (((2, 0, 3), "points"), ((0, 7, 3), "views"), ((65536, 1, 3), "views"),
                         ((1, (1 << 24) + 1, 3), "points")):
        t = torch.zeros(1).expand(shape)                # no memory behind it
        with pytest.raises(ValueError, match=what + ".*" + match):
            fn(*((t, None) if what == "pos" else (None, t)), views(min(max(shape[0], 1), 2)))


@each_batched
def test_a_non_float_input(fn):
    with pytest.raises(ValueError, match="floating"):
        fn(torch.zeros(2, 7, 3, dtype=torch.int64), None, views())
    with pytest.raises(ValueError, match="floating"):
        fn(None, np.zeros((2, 7, 3), dtype=np.int32), views())


@each_batched
@pytest.mark.parametrize("camera_grad", [None, 1, "yes", 0.0])
def test_a_camera_grad_that_is_not_a_bool(fn, camera_grad):
    with pytest.raises(ValueError, match="camera_grad"):
        fn(torch.zeros(2, 7, 3), None, views(), camera_grad=camera_grad)


@each_batched
@pytest.mark.parametrize("key", ["eye", "at", "up"])
def test_the_camera_checks(fn, key):
    pos = torch.zeros(2, 7, 3)
    c = views()
    del c[key]
    with pytest.raises(ValueError, match=key + ".*missing"):
        fn(pos, None, c)
    for shape in ((3,), (2, 2), (2, 5), (1, 3), (2, 1, 3)):
        with pytest.raises(ValueError, match=key):
            fn(pos, None, dict(views(), **{key: torch.ones(shape)}))
    with pytest.raises(ValueError, match="requires grad.*camera_grad=True"):
        fn(pos, None, dict(views(), **{key: views()[key].clone().requires_grad_(True)}))


@each_batched
def test_the_w_conventions_and_degenerate_cameras(fn):
    pos = torch.zeros(2, 7, 3)
    for key, w in (("up", 1.0), ("eye", 0.0), ("at", 0.0)):
        c = views(hom=True)
        c[key] = c[key].clone()
        c[key][1, 3] = w
        with pytest.raises(ValueError, match=key + ".*w"):
            fn(pos, None, c)
    c = views()
    with pytest.raises(ValueError, match="eye.*at"):
        fn(pos, None, dict(c, at=c["eye"].clone()))
    with pytest.raises(ValueError, match="up"):
        fn(pos, None, dict(c, up=torch.zeros(2, 3)))
    with pytest.raises(ValueError, match="eye"):
        fn(pos, None, dict(c, eye=torch.full((2, 3), float("nan"))))


@each_batched
def test_the_transforms_do_not_ask_for_a_pinhole_but_refuse_one_that_wants_a_gradient(fn, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):                       # eye / at / up are enough
        fn(torch.zeros(2, 7, 4, dtype=torch.float64), np.zeros((2, 9, 3), np.float32), views(hom=True))
    c = dict(views(), focal_length=torch.tensor(0.5, requires_grad=True))
    for camera_grad in (False, True):
        with pytest.raises(ValueError, match="focal_length.*requires grad"):
            fn(torch.zeros(2, 7, 3), None, c, camera_grad=camera_grad)


@each_unbatched
def test_the_unbatched_forms_take_one_view(fn, monkeypatch):
    with pytest.raises(ValueError, match="pos"):
        fn(torch.zeros(1, 7, 3), None, one_view())
    with pytest.raises(ValueError, match="normal"):
        fn(None, torch.zeros(3), one_view())
    with pytest.raises(ValueError, match="pos"):
        fn(torch.zeros(7, 5), None, one_view())
    with pytest.raises(ValueError, match="eye"):
        fn(torch.zeros(7, 3), None, views(1))
    with pytest.raises(ValueError, match="both None"):
        fn(None, None, one_view())
    with pytest.raises(ValueError, match="camera_grad"):
        fn(torch.zeros(7, 3), None, one_view(), camera_grad=1)
    with pytest.raises(ValueError, match="requires grad"):
        fn(torch.zeros(7, 3), None, dict(one_view(), up=one_view()["up"].clone().requires_grad_(True)))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for hom in (False, True):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(torch.zeros(7, 4), np.zeros((5, 3)), one_view(hom))


def full(B=2, hom=False, **change):
    return dict(camera(B, 4, 5, hom=hom), **change)


@each_projection
@pytest.mark.parametrize("shape", [(7, 3), (2, 7), (2, 7, 2), (2, 7, 5), (2, 1, 7, 3), (2, 0, 3), (0, 7, 3)])
def test_surfels_of_another_shape(fn, shape):
    with pytest.raises(ValueError, match="surfels"):
        fn(torch.zeros(shape), full())


@each_projection
def test_surfels_missing_out_of_range_or_not_float(fn):
    with pytest.raises(ValueError, match="surfels"):
        fn(None, full())
    with pytest.raises(ValueError, match="surfels.*points"):
        fn(torch.zeros(1).expand(1, (1 << 24) + 1, 3), full(1))
    with pytest.raises(ValueError, match="surfels.*views"):
        fn(torch.zeros(1).expand(65536, 1, 3), full(1))
    with pytest.raises(ValueError, match="floating"):
        fn(torch.zeros(2, 7, 3, dtype=torch.int32), full())
    with pytest.raises(ValueError, match="eye"):
        fn(torch.zeros(3, 7, 3), full(2))


@each_projection
@pytest.mark.parametrize("key", ["eye", "at", "up", "viewport", "fovy", "focal_length"])
def test_a_missing_camera_entry(fn, key):
    c = full()
    del c[key]
    with pytest.raises(ValueError, match=key + ".*missing"):
        fn(torch.zeros(2, 7, 3), c)


@each_projection
def test_the_pinhole_checks(fn):
    s = torch.zeros(2, 7, 3)
    for viewport in ([0, 0, 0, 4], [0, 0, 5, 0], [3, 0, 2, 4], [0, 0, 5], [0, 0, 4097, 4096]):
        with pytest.raises(ValueError, match="viewport"):
            fn(s, full(viewport=viewport))
    for key, value in (("fovy", 0.0), ("fovy", 3.2), ("fovy", float("nan")), ("focal_length", 0.0),
                       ("focal_length", -1.0), ("focal_length", float("inf"))):
        with pytest.raises(ValueError, match=key):
            fn(s, full(**{key: value}))
    with pytest.raises(ValueError, match="eye.*at"):
        fn(s, full(at=full()["eye"].clone()))


@each_projection
def test_camera_gradients_need_the_keyword_and_only_eye_at_up_have_one(fn):
    s = torch.zeros(2, 7, 3)
    for key in ("eye", "at", "up"):
        with pytest.raises(ValueError, match=key + ".*requires grad.*camera_grad=True"):
            fn(s, full(**{key: full()[key].clone().requires_grad_(True)}))
    for key in ("fovy", "focal_length"):
        for camera_grad in (False, True):
            with pytest.raises(ValueError, match=key + ".*requires grad"):
                fn(s, full(**{key: torch.tensor(0.5, requires_grad=True)}), camera_grad=camera_grad)
    with pytest.raises(ValueError, match="viewport.*requires grad"):
        fn(s, full(viewport=torch.tensor([0.0, 0.0, 5.0, 4.0], requires_grad=True)), camera_grad=True)
    for camera_grad in (None, 1, "yes"):
        with pytest.raises(ValueError, match="camera_grad"):
            fn(s, full(), camera_grad=camera_grad)


@each_projection
def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(fn, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for hom in (False, True):
        for cols in (3, 4):
            with pytest.raises(RuntimeError, match="GPU"):
                fn(torch.zeros(2, 7, cols, dtype=torch.float16), full(hom=hom))
