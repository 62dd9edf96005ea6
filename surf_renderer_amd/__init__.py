"""surf_renderer_amd -- MI355X-native `hip` backend for DiffRend's render(scene) hot path.

    from surf_renderer_amd import render
    res = render(scene)            # same scene dict as diffrend.numpy.renderer.render
    res['image'], res['depth'], res['nearest']

The names below are imported on first use (PEP 562): `surf_renderer_amd.frame_writer`'s writer process is spawned, imports
this package on the way to its own module and needs numpy only -- not torch and the render library.
"""
import importlib

_RENDERER = ("render", "render_views", "ResidentScene", "CapturedStep", "ViewScenes", "flatten_scene", "render_buffers", "camera_struct",
             "generate_rays")
_SCENE = ("load_scene", "load_model", "load_obj", "load_splat", "obj_to_triangle_spec")
_SPLATS = ("render_splats_along_ray", "render_splats_along_ray_batch")
_SPLATS_NDC = ("render_splats_NDC", "render_splats_NDC_batch")
_REGULARIZERS = ("splat_regularizers", "REGULARIZER_TERMS")
_PROJECTION = ("projection_renderer_differentiable_fast",)
_REVERSE_PROJECTION = ("projection_reverse_renderer",)
_DENSE_PROJECTION = ("projection_renderer_differentiable", "projection_renderer_differentiable_camera")
_SURFELS = ("depth_to_surfels",)
_HARD_PROJECTION = ("projection_renderer",)
_NORMALS = ("estimate_surface_normals_plane_fit_batched", "estimate_surface_normals_plane_fit", "estimate_surface_normals")
_FRAMES = ("world_to_cam", "world_to_cam_batched", "cam_to_world", "cam_to_world_batched", "project_surfels",
           "project_image_coordinates")
_POINTSETS = ("nearest_points", "hausdorff", "hausdorff_batched", "NearestPoints")
_MESH_SAMPLING = ("uniform_sample_mesh", "sample_mesh_batched", "mesh_topology", "draw_uniforms", "MeshSamples",
                  "MeshTopology")
_SH_LIGHTING = ("radiance_SH9", "radiance_SH9_batched", "RealSH9_ZonalMatrix", "irradiance", "irradiance_batched",
                "irradiance_polar", "irrad_Z", "reconstruct_SH9", "RealSH9_cart", "RealSH9_polar", "load_lightprobe")

__all__ = [*_RENDERER, *_SCENE, *_SPLATS, *_SPLATS_NDC, *_REGULARIZERS, *_PROJECTION, *_REVERSE_PROJECTION, *_DENSE_PROJECTION,
           *_SURFELS, *_HARD_PROJECTION, *_NORMALS, *_FRAMES, *_POINTSETS, *_MESH_SAMPLING, *_SH_LIGHTING]


def __getattr__(name):
    if name in _RENDERER:
        return getattr(importlib.import_module(".renderer", __name__), name)
    if name in _SCENE:
        return getattr(importlib.import_module(".scene", __name__), name)
    if name in _SPLATS:
        return getattr(importlib.import_module(".splats", __name__), name)
    if name in _SPLATS_NDC:
        return getattr(importlib.import_module(".splats_ndc", __name__), name)
    if name in _REGULARIZERS:
        return getattr(importlib.import_module(".regularizers", __name__), name)
    if name in _PROJECTION:
        return getattr(importlib.import_module(".projection", __name__), name)
    if name in _REVERSE_PROJECTION:
        return getattr(importlib.import_module(".reverse_projection", __name__), name)
    if name in _DENSE_PROJECTION:
        return getattr(importlib.import_module(".dense_projection", __name__), name)
    if name in _SURFELS:
        return getattr(importlib.import_module(".surfels", __name__), name)
    if name in _HARD_PROJECTION:
        return getattr(importlib.import_module(".hard_projection", __name__), name)
    if name in _NORMALS:
        return getattr(importlib.import_module(".normals", __name__), name)
    if name in _FRAMES:
        return getattr(importlib.import_module(".frames", __name__), name)
    if name in _POINTSETS:
        return getattr(importlib.import_module(".pointsets", __name__), name)
    if name in _MESH_SAMPLING:
        return getattr(importlib.import_module(".mesh_sampling", __name__), name)
    if name in _SH_LIGHTING:
        return getattr(importlib.import_module(".sh_lighting", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted([*globals(), *__all__])
