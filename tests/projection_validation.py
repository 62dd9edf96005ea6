"""The argument checks the three re-projection layers have in common, written once: each function here returns test
functions for one layer, and the layer's test module (tests/test_projection_validation_cpu.py, test_dense_... and
test_reverse_...) takes them into its namespace beside the tests only it has.  `project` is the layer, `args(B, H, W, D,
hom)` its valid arguments by name.  Every refusal is a ValueError on the host, before the library is loaded and before
anything reaches the GPU, so these run without one."""
import numpy as np
import pytest
import torch

from surf_renderer_amd import _lib


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.fixture
def cam():
    """The camera argument of a layer with one; a layer with two parametrises `cam` instead."""
    return "camera"


def camera(B, H, W, fovy=0.7, focal=0.5, hom=False):
    c = {"eye": torch.tensor([[0.0, 0.5, 4.0]] * B), "at": torch.zeros(B, 3), "up": torch.tensor([[0.0, 1.0, 0.0]] * B),
         "viewport": [0, 0, W, H], "fovy": fovy, "focal_length": focal}
    if hom:
        c["eye"] = torch.cat((c["eye"], torch.ones(B, 1)), -1)
        c["at"] = torch.cat((c["at"], torch.ones(B, 1)), -1)
        c["up"] = torch.cat((c["up"], torch.zeros(B, 1)), -1)
    return c


def refused(project, args, match, hom=False, **change):
    a = args(hom=hom)
    a.update(change)
    with pytest.raises(ValueError, match=match):
        project(**a)


def _tests(*functions):
    return {f.__name__: f for f in functions}


def surfel_tests(project, args):
    """The layers that take (surfels, rgb, camera, rotated_image, blur_size)."""
    @pytest.mark.parametrize("shape", [(2, 20), (2, 20, 4), (20, 3), (2, 4, 5, 3)])
    def test_surfels_of_another_shape(shape):
        refused(project, args, "surfels", surfels=torch.zeros(shape))

    @pytest.mark.parametrize("n", [19, 21, 25])
    def test_a_surfel_count_that_is_not_the_frame(n):
        refused(project, args, "W x H", surfels=torch.zeros(2, n, 3))

    @pytest.mark.parametrize("shape", [(2, 20), (3, 20, 3), (2, 5, 4, 3), (2, 21, 3), (20, 3), (2, 4, 5)])
    def test_rgb_of_another_shape(shape):
        refused(project, args, "rgb", rgb=torch.zeros(shape))

    def test_an_empty_batch():
        c = dict(args()["camera"], eye=torch.zeros(0, 3), at=torch.zeros(0, 3), up=torch.zeros(0, 3))
        with pytest.raises(ValueError, match="empty"):
            project(torch.zeros(0, 20, 3), torch.zeros(0, 20, 3), c)

    @pytest.mark.parametrize("viewport", [[0, 0, 0, 4], [0, 0, 5, 0], [3, 0, 2, 4], [0, 0, 5]])
    def test_an_empty_or_malformed_viewport(viewport):
        refused(project, args, "viewport", camera=dict(args()["camera"], viewport=viewport))

    @pytest.mark.parametrize("blur_size", [0.0, -0.15, float("nan"), float("inf")])
    def test_a_blur_size_that_is_not_positive_and_finite(blur_size):
        refused(project, args, "blur_size", blur_size=blur_size)

    def test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback(monkeypatch):
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
        for hom in (False, True):
            for dtype in (torch.float32, torch.float64, torch.float16):
                a = args(hom=hom)
                with pytest.raises(RuntimeError, match="GPU"):
                    project(a["surfels"].to(dtype), a["rgb"].to(dtype).reshape(2, 20, 3), a["camera"],
                            rotated_image=a["rgb"].reshape(2, 20, 3))
        with pytest.raises(RuntimeError, match="GPU"):
            project(**args(B=1, H=1, W=1, D=1))

    return _tests(test_surfels_of_another_shape, test_a_surfel_count_that_is_not_the_frame, test_rgb_of_another_shape,
                  test_an_empty_batch, test_an_empty_or_malformed_viewport, test_a_blur_size_that_is_not_positive_and_finite,
                  test_a_valid_call_without_a_gpu_is_an_error_not_a_fallback)


def image_tests(project, args, inputs, rgb_shape, rotated_shapes):
    """rgb's channels, the rotated image and the dtypes: `inputs` are the layer's tensor arguments, `rgb_shape(D)` an rgb
    that is valid but for its D channels, `rotated_shapes` what a rotated image beside the valid rgb must not be."""
    @pytest.mark.parametrize("D", [0, 5, 8])
    def test_a_channel_count_outside_one_to_four(D):
        refused(project, args, "channels", rgb=torch.zeros(rgb_shape(D)))

    @pytest.mark.parametrize("shape", rotated_shapes)
    def test_a_rotated_image_unlike_rgb(shape):
        refused(project, args, "rotated_image", rotated_image=torch.zeros(shape))

    @pytest.mark.parametrize("key", inputs)
    @pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.bool])
    def test_a_non_float_input(key, dtype):
        a = args()
        a["rotated_image"] = a["rgb"].clone()
        a[key] = a[key].to(dtype)
        with pytest.raises(ValueError, match="floating"):
            project(**a)
        a[key] = np.zeros(tuple(a[key].shape), dtype=np.int64)
        with pytest.raises(ValueError, match="floating"):
            project(**a)

    return _tests(test_a_channel_count_outside_one_to_four, test_a_rotated_image_unlike_rgb, test_a_non_float_input)


def camera_tests(project, args, cams=None):
    """Every check of a camera dict, against the argument `cam`: the fixture above, or each of `cams`."""
    each_camera = pytest.mark.parametrize("cam", cams) if cams else (lambda f: f)

    def bad(match, cam, hom=False, **entries):
        """refused, with the valid camera's `entries` replaced; an entry that is a function gets the valid camera"""
        c = args(hom=hom)[cam]
        changed = dict(c, **{k: (v(c) if callable(v) else v) for k, v in entries.items()})
        refused(project, args, cam + ".*" + match, hom=hom, **{cam: changed})

    @each_camera
    @pytest.mark.parametrize("key", ["eye", "at", "up", "viewport", "fovy", "focal_length"])
    def test_a_missing_camera_entry(cam, key):
        c = dict(args()[cam])
        del c[key]
        refused(project, args, cam + ".*" + key, **{cam: c})

    @each_camera
    @pytest.mark.parametrize("key", ["eye", "at", "up"])
    @pytest.mark.parametrize("shape", [(3,), (2, 2), (2, 5), (1, 3), (2, 1, 3)])
    def test_camera_vectors_of_another_shape(cam, key, shape):
        bad(key, cam, **{key: torch.ones(shape)})

    @each_camera
    def test_the_w_conventions_of_the_reference(cam):
        def second_w(key, w):
            def change(c):
                v = c[key].clone()
                v[1, 3] = w
                return v
            return change
        for key, w in (("up", 1.0), ("eye", 0.0), ("at", 0.0)):
            bad(key + ".*w", cam, hom=True, **{key: second_w(key, w)})

    @each_camera
    def test_a_degenerate_camera(cam):
        bad("eye.*at", cam, at=lambda c: c["eye"].clone())
        bad("up", cam, up=torch.zeros(2, 3))
        bad("up", cam, up=lambda c: c["eye"] - c["at"])
        bad("eye", cam, eye=torch.full((2, 3), float("nan")))

    @each_camera
    @pytest.mark.parametrize("key,value", [("fovy", 0.0), ("fovy", 3.2), ("fovy", float("nan")), ("focal_length", 0.0),
                                           ("focal_length", -1.0), ("focal_length", float("inf"))])
    def test_projection_scalars_out_of_range(cam, key, value):
        bad(key, cam, **{key: value})

    @each_camera
    @pytest.mark.parametrize("key", ["eye", "at", "up"])
    def test_a_camera_that_requires_grad(cam, key):
        bad("requires grad", cam, **{key: lambda c: c[key].clone().requires_grad_(True)})

    return _tests(test_a_missing_camera_entry, test_camera_vectors_of_another_shape, test_the_w_conventions_of_the_reference,
                  test_a_degenerate_camera, test_projection_scalars_out_of_range, test_a_camera_that_requires_grad)
