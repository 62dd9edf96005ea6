"""The Python host layer's shared helpers, on CPU tensors and without the render library: where a gradient buffer is bound
in SrhGrads, which scene references a batch of views hands the library, how upstream gradients are prepared, the
keyword signatures of the low-level views calls and the names ``surf_renderer_amd.renderer`` keeps importable."""
import ctypes as C
import inspect
import itertools

import pytest
import torch

from surf_renderer_amd import _lib, renderer
from surf_renderer_amd.scene import PRIM_CODE
from surf_renderer_amd.frame import _bind_grad, _like, _upstream
from surf_renderer_amd.views import ViewScenes, _scene_refs

N_DISK, N_TRI = 5, 2


def _buffers() -> renderer.SceneBuffers:
    """Two segments, disk x 5 and triangle x 2, two lights, three colours, two materials: built by hand from CPU tensors."""
    f32, i32 = torch.float32, torch.int32
    t = {"disk.pos": torch.zeros(N_DISK, 4, dtype=f32), "disk.normal": torch.zeros(N_DISK, 4, dtype=f32),
         "disk.radius": torch.ones(N_DISK, dtype=f32), "disk.material_idx": torch.zeros(N_DISK, dtype=i32),
         "triangle.face": torch.zeros(N_TRI, 3, 4, dtype=f32), "triangle.normal": torch.zeros(N_TRI, 4, dtype=f32),
         "triangle.material_idx": torch.zeros(N_TRI, dtype=i32),
         "lights.pos": torch.zeros(2, 4, dtype=f32), "lights.color_idx": torch.zeros(2, dtype=i32),
         "colors": torch.zeros(3, 3, dtype=f32), "materials.albedo": torch.zeros(2, 3, dtype=f32),
         "materials.coeffs": torch.zeros(2, 3, dtype=f32)}
    ob = _lib.SrhObjects(n_segments=2)
    ob.seg[0].type, ob.seg[0].count = PRIM_CODE["disk"], N_DISK
    ob.seg[1].type, ob.seg[1].count = PRIM_CODE["triangle"], N_TRI
    for s, kind in enumerate(("disk", "triangle")):
        for key, x in t.items():
            if key.startswith(kind + "."):
                setattr(ob.seg[s], key.split(".")[1], x.data_ptr())
    ls = _lib.SrhLights(n_lights=2, n_colors=3, pos=t["lights.pos"].data_ptr(), color_idx=t["lights.color_idx"].data_ptr(),
                        colors=t["colors"].data_ptr())
    ms = _lib.SrhMaterials(n_materials=2, albedo=t["materials.albedo"].data_ptr(), coeffs=t["materials.coeffs"].data_ptr())
    return renderer.SceneBuffers(device=torch.device("cpu"), kinds=["disk", "triangle"], counts=[N_DISK, N_TRI], tensors=t,
                                 objects=ob, lights=ls, materials=ms, gamma=None, total=N_DISK + N_TRI)


def _grad_fields(sg: _lib.SrhGrads) -> dict:
    """Every non-NULL pointer of ``sg`` as {(field, segment or None): address}."""
    out = {}
    for name, ctype in _lib.SrhGrads._fields_:
        val = getattr(sg, name)
        if ctype is C.c_void_p:
            if val:
                out[(name, None)] = val
        else:
            out.update({(name, s): val[s] for s in range(len(val)) if val[s]})
    return out


# where each differentiable input's gradient buffer belongs in SrhGrads: (field, segment); spelt out, not derived
_EXPECTED_FIELD = {
    "disk.pos": ("pos", 0), "disk.normal": ("normal", 0), "disk.radius": None,
    "triangle.face": ("face", 1), "triangle.normal": ("normal", 1),
    "lights.pos": ("lights_pos", None), "colors": ("colors", None),
    "materials.albedo": ("albedo", None), "materials.coeffs": ("coeffs", None),
}


def test_float_keys_of_the_hand_built_scene():
    buf = _buffers()
    assert renderer._float_keys(buf, "torch") == list(_EXPECTED_FIELD)
    assert renderer._float_keys(buf, "numpy") == [k for k in _EXPECTED_FIELD if k != "materials.coeffs"]


@pytest.mark.parametrize("key", list(_EXPECTED_FIELD))
def test_bind_grad_sets_exactly_the_keys_field(key):
    buf = _buffers()
    g = torch.zeros_like(buf.tensors[key])
    sg = _lib.SrhGrads()
    _bind_grad(sg, buf, key, g)
    want = _EXPECTED_FIELD[key]
    assert _grad_fields(sg) == ({} if want is None else {want: g.data_ptr()})


def test_bind_grad_keeps_every_key_apart():
    buf = _buffers()
    keys = renderer._float_keys(buf, "torch")
    grads = {k: torch.zeros_like(buf.tensors[k]) for k in keys}
    assert len({g.data_ptr() for g in grads.values()}) == len(keys)
    sg = _lib.SrhGrads()
    for k in keys:
        _bind_grad(sg, buf, k, grads[k])
    assert _grad_fields(sg) == {_EXPECTED_FIELD[k]: grads[k].data_ptr() for k in keys if _EXPECTED_FIELD[k] is not None}
    assert sg.face[0] is None and sg.face[1] == grads["triangle.face"].data_ptr()      # segment 1, not 0


def _struct_bytes(ref) -> bytes:
    return bytes(ref._obj)


def test_view_scenes_refs():
    buf = _buffers()
    disk_pos = torch.ones(N_DISK, 4)
    lights_pos, albedo = torch.ones(2, 4), torch.ones(2, 3)
    scenes = ViewScenes(buf, [{}, {"disk.pos": disk_pos}, {"lights.pos": lights_pos, "materials.albedo": albedo}])
    ob, ls, ms, mask = scenes.refs(buf, 0, 3)
    assert mask == _lib.VIEWS_OBJECTS | _lib.VIEWS_LIGHTS | _lib.VIEWS_MATERIALS
    assert _struct_bytes(ob) == bytes(buf.objects)                  # view 0 overrides nothing
    assert _struct_bytes(ls) == bytes(buf.lights)
    assert _struct_bytes(ms) == bytes(buf.materials)
    assert C.addressof(ob._obj) == C.addressof(scenes.objects[0])   # and is the head of the per-view arrays
    ob1, ls1, ms1, _ = scenes.refs(buf, 1, 2)
    assert ob1._obj.seg[0].pos == scenes.keys[1]["disk.pos"].data_ptr() == disk_pos.data_ptr()
    assert ob1._obj.seg[0].normal == buf.tensors["disk.normal"].data_ptr()
    assert _struct_bytes(ls1) == bytes(buf.lights)
    assert scenes.lights[2].pos == lights_pos.data_ptr() and scenes.materials[2].albedo == albedo.data_ptr()
    assert _scene_refs(buf, scenes, 1, 2)[3] == mask
    for first, n in ((1, 3), (3, 1), (-1, 2)):
        with pytest.raises(ValueError, match=f"3 per-view scenes for {n} cameras from view {first}"):
            scenes.refs(buf, first, n)
        with pytest.raises(ValueError):
            _scene_refs(buf, scenes, first, n)


def test_view_scenes_refs_only_what_is_overridden():
    buf = _buffers()
    scenes = ViewScenes(buf, [{}, {"lights.pos": torch.ones(2, 4)}])
    ob, ls, ms, mask = scenes.refs(buf, 1, 1)
    assert mask == _lib.VIEWS_LIGHTS
    assert C.addressof(ob._obj) == C.addressof(buf.objects) and C.addressof(ms._obj) == C.addressof(buf.materials)
    assert C.addressof(ls._obj) == C.addressof(scenes.lights[1])


def test_scene_refs_without_view_scenes():
    buf = _buffers()
    ob, ls, ms, mask = _scene_refs(buf, None, 0, 7)
    assert mask == 0
    assert C.addressof(ob._obj) == C.addressof(buf.objects)
    assert C.addressof(ls._obj) == C.addressof(buf.lights)
    assert C.addressof(ms._obj) == C.addressof(buf.materials)


_SHAPE = (2, 3, 4, 3)


@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("present", list(itertools.product([False, True], repeat=4)))
def test_upstream_zero_fill_rule(present, camera):
    has_image, has_depth, has_normal, has_pos = present
    given = [torch.full(_SHAPE if i != 1 else _SHAPE[:-1], float(i + 1)) if has else None for i, has in enumerate(present)]
    g_image, g_depth, g_normal, g_pos = _upstream(*given, camera, _SHAPE, torch.device("cpu"))
    # a missing image gradient becomes zeros unless an aux upstream gradient is given, or camera gradients are wanted
    # and a depth gradient is given
    stays_none = has_normal or has_pos or (camera and has_depth)
    if has_image:
        assert torch.equal(g_image, given[0])
    elif stays_none:
        assert g_image is None
    else:
        assert g_image.shape == _SHAPE and g_image.dtype == torch.float32 and not g_image.any()
    for got, src in ((g_depth, given[1]), (g_normal, given[2]), (g_pos, given[3])):
        assert (got is None) if src is None else torch.equal(got, src)


def test_upstream_makes_dense_float32():
    base = torch.arange(2 * 3 * 8 * 3, dtype=torch.float64).reshape(2, 3, 8, 3)
    g_image = base[:, :, ::2]                                       # float64, not contiguous
    g_depth = torch.arange(2 * 4 * 3, dtype=torch.float64).reshape(2, 4, 3).transpose(1, 2)
    assert not g_image.is_contiguous() and not g_depth.is_contiguous()
    out = _upstream(g_image, g_depth, g_image + 1, None, True, _SHAPE, torch.device("cpu"))
    for got, src in zip(out[:3], (g_image, g_depth, g_image + 1)):
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == src.shape
        assert torch.equal(got.double(), src)                       # small integers: exact in float32
    assert out[3] is None


def test_like_hands_a_camera_gradient_back_in_the_leafs_form():
    g = torch.tensor([1.0, 2.0, 3.0, 0.0])
    up3 = _like(g, (3,), torch.float64, torch.device("cpu"))
    assert up3.dtype == torch.float64 and up3.tolist() == [1.0, 2.0, 3.0]
    assert _like(g, (1, 4), torch.float32, torch.device("cpu")).tolist() == [[1.0, 2.0, 3.0, 0.0]]


def test_low_level_views_calls_refuse_unknown_keywords():
    fwd = inspect.signature(renderer.render_views_buffers)
    bwd = inspect.signature(renderer.render_views_bwd_buffers)
    fwd.bind(None, [], None, None, shading="torch", double_sided=True, use_quartic=True, waves_per_tile=4)
    bwd.bind(None, [], None, None, None, None, None, shading="torch", double_sided=True, use_quartic=True)
    with pytest.raises(TypeError):
        fwd.bind(None, [], None, None, shadng="torch")
    with pytest.raises(TypeError):
        bwd.bind(None, [], None, None, None, None, None, shadng="torch")
    with pytest.raises(TypeError):
        bwd.bind(None, [], None, None, None, None, None, waves_per_tile=4)
    for sig, defaults in ((fwd, {"shading": "numpy", "double_sided": False, "use_quartic": False, "waves_per_tile": 0}),
                          (bwd, {"shading": "numpy", "double_sided": False, "use_quartic": False})):
        assert {k: sig.parameters[k].default for k in defaults} == defaults


_REEXPORTED = (
    # the package's public names (__init__.py)
    "render", "render_views", "ResidentScene", "CapturedStep", "ViewScenes", "flatten_scene", "render_buffers",
    "camera_struct", "generate_rays",
    # what pipeline.py, bench.py, the tools and the tests use
    "render_views_buffers", "render_views_bwd_buffers", "shadow_pass", "bin_statistics", "SceneBuffers", "frame_size",
    "RenderResult", "_ws_state", "_ws_note", "_layout_key", "_float_keys", "_RenderFunction", "_Shade",
)


@pytest.mark.parametrize("name", _REEXPORTED)
def test_renderer_keeps_the_name_importable(name):
    assert getattr(renderer, name) is not None


def test_package_names_come_from_renderer():
    import surf_renderer_amd
    for name in surf_renderer_amd._RENDERER:
        assert getattr(surf_renderer_amd, name) is getattr(renderer, name)
