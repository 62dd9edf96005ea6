"""ctypes binding of libsrh.so (the C ABI in include/srh.h).  Fails loudly when the library is
missing or was built for a different ABI: there is no CPU fallback behind the hip backend."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import build as _build

ABI_VERSION = 12
MAX_SEGMENTS = 4
MAX_LIGHTS = 64

MODE_AUTO, MODE_EXACT, MODE_FAST, MODE_BINNED = 0, 1, 2, 3
MODES = {"auto": MODE_AUTO, "exact": MODE_EXACT, "fast": MODE_FAST, "binned": MODE_BINNED}
SHADING = {"numpy": 0, "torch": 1}

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)


class SrhCamera(C.Structure):
    _fields_ = [("eye", C.c_double * 4), ("at", C.c_double * 4), ("up", C.c_double * 4),
                ("fovy", C.c_double), ("focal_length", C.c_double),
                ("near_clip", C.c_double), ("far_clip", C.c_double),
                ("viewport", C.c_int32 * 4), ("ortho", C.c_int32), ("up_is_unit", C.c_int32)]


class SrhSegment(C.Structure):
    _fields_ = [("type", C.c_int32), ("count", C.c_int32),
                ("pos", C.c_void_p), ("normal", C.c_void_p), ("radius", C.c_void_p),
                ("face", C.c_void_p), ("material_idx", C.c_void_p)]


class SrhObjects(C.Structure):
    _fields_ = [("n_segments", C.c_int32), ("seg", SrhSegment * MAX_SEGMENTS)]


class SrhLights(C.Structure):
    _fields_ = [("n_lights", C.c_int32), ("n_colors", C.c_int32),
                ("pos", C.c_void_p), ("color_idx", C.c_void_p), ("colors", C.c_void_p),
                ("attenuation", C.c_void_p), ("ambient", C.c_void_p)]


class SrhMaterials(C.Structure):
    _fields_ = [("n_materials", C.c_int32), ("albedo", C.c_void_p), ("coeffs", C.c_void_p)]


class SrhParams(C.Structure):
    _fields_ = [("row0", C.c_int32), ("row1", C.c_int32), ("mode", C.c_int32),
                ("tonemap_gamma", C.c_int32), ("gamma", C.c_double),
                ("shading", C.c_int32), ("double_sided", C.c_int32), ("use_quartic", C.c_int32), ("waves_per_tile", C.c_int32),
                ("normal_out", C.c_void_p), ("pos_out", C.c_void_p),
                ("image_row_stride", C.c_int64), ("depth_row_stride", C.c_int64),
                ("nearest_row_stride", C.c_int64),
                ("ev_start", C.c_void_p), ("ev_stop", C.c_void_p), ("visibility", C.c_void_p),
                ("view_row0", C.c_void_p), ("stages", C.c_int32), ("counters_clean", C.c_int32),
                ("per_view", C.c_int32), ("reserved1", C.c_int32)]

STAGE_BIN, STAGE_RENDER, STAGE_KEEP_BINS = 1, 2, 4
E_NOT_APPLICABLE = -6
VIEWS_OBJECTS, VIEWS_LIGHTS, VIEWS_MATERIALS = 1, 2, 4


class SrhGrads(C.Structure):
    _fields_ = [("pos", C.c_void_p * MAX_SEGMENTS), ("normal", C.c_void_p * MAX_SEGMENTS),
                ("radius", C.c_void_p * MAX_SEGMENTS), ("face", C.c_void_p * MAX_SEGMENTS),
                ("lights_pos", C.c_void_p), ("colors", C.c_void_p), ("albedo", C.c_void_p),
                ("coeffs", C.c_void_p), ("attenuation", C.c_void_p), ("ambient", C.c_void_p)]


class SrhCameraGrads(C.Structure):
    _fields_ = [("eye", C.c_void_p), ("at", C.c_void_p), ("up", C.c_void_p)]


class SrhSplatParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32),
                ("pos_cols", C.c_int32), ("use_quartic", C.c_int32), ("shade", C.c_int32), ("reserved", C.c_int32),
                ("fovy", C.c_double), ("focal_length", C.c_double), ("at", C.c_double * 3), ("up", C.c_double * 3)]


class SrhSplatInputs(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("pos_view_stride", C.c_int64), ("normal", C.c_void_p),
                ("normal_view_stride", C.c_int64), ("light_vis", C.c_void_p), ("light_vis_view_stride", C.c_int64),
                ("eye", C.c_void_p), ("eye_view_stride", C.c_int64), ("lights_pos_view_stride", C.c_int64),
                ("material_idx", C.c_void_p)]


class SrhSplatGrads(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pos", "normal", "light_vis", "lights_pos", "colors", "attenuation",
                                          "ambient", "albedo", "coeffs")]


class SrhSplatNdcParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("pos_cols", C.c_int32),
                ("use_quartic", C.c_int32), ("double_sided", C.c_int32), ("shade", C.c_int32), ("reserved", C.c_int32),
                ("fovy", C.c_double), ("near_clip", C.c_double), ("far_clip", C.c_double), ("at", C.c_double * 3),
                ("up", C.c_double * 3)]


class SrhSplatNdcInputs(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("pos_view_stride", C.c_int64), ("normal", C.c_void_p),
                ("normal_view_stride", C.c_int64), ("eye", C.c_void_p), ("eye_view_stride", C.c_int64),
                ("lights_pos_view_stride", C.c_int64), ("material_idx", C.c_void_p)]


class SrhSplatNdcGrads(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pos", "normal", "lights_pos", "colors", "attenuation", "ambient", "albedo",
                                          "coeffs")]


class SrhRegularizerParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32),
                ("z_min", C.c_double), ("z_max", C.c_double), ("z_scale", C.c_double),
                ("unit_normal_scale", C.c_double)]


REG_TERMS, REG_STATS = 7, 4

PROJ_MAX_CHANNELS, PROJ_MAX_BLUR_HALF = 4, 64
(PROJ_USE_DEPTH, PROJ_USE_CENTER_DIST, PROJ_BLUR_ROTATED, PROJ_DETACH_MASK, PROJ_DETACH_MASK2,
 PROJ_DETACH_DEPTH_MERGE) = 1, 2, 4, 8, 16, 32
PROJ_WS_FWD, PROJ_WS_SAVED, PROJ_WS_BWD = 0, 1, 2


class SrhProjectionParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("flags", C.c_int32), ("blur_half", C.c_int32), ("fovy", C.c_double), ("focal_length", C.c_double),
                ("taps", C.c_double * (PROJ_MAX_BLUR_HALF + 1))]


RPROJ_WS_FWD, RPROJ_WS_BWD = 0, 1


class SrhReverseProjectionParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("fovy1", C.c_double), ("focal_length1", C.c_double), ("fovy2", C.c_double),
                ("focal_length2", C.c_double), ("depth_epsilon", C.c_double)]


DPROJ_WS_FWD, DPROJ_WS_SAVED, DPROJ_WS_BWD, DPROJ_WS_VIEW = 0, 1, 2, 4


class SrhDenseProjectionParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("has_rotated", C.c_int32), ("reserved", C.c_int32), ("sigma", C.c_double), ("fovy", C.c_double),
                ("focal_length", C.c_double)]


SURFELS_FRAME = {"camera": 0, "world": 1}


class SrhSurfelsParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("frame", C.c_int32),
                ("fovy", C.c_double), ("focal_length", C.c_double)]


class SrhHardProjectionParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("fovy", C.c_double), ("focal_length", C.c_double)]


class SrhFrameParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_pos", C.c_int32), ("n_normal", C.c_int32), ("pos_cols", C.c_int32),
                ("normal_cols", C.c_int32)]


class SrhProjectCoordsParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_points", C.c_int32), ("cols", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("fovy", C.c_double), ("focal_length", C.c_double)]


class SrhPointSetParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_u", C.c_int32), ("n_v", C.c_int32), ("dims", C.c_int32),
                ("squared", C.c_int32)]


POINTSETS_MAX_DIMS, POINTSETS_MAX_POINTS = 4, 1 << 24


class SrhMeshSampleParams(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_vertices", C.c_int32), ("n_faces", C.c_int32), ("n_samples", C.c_int32),
                ("faces_per_view", C.c_int32), ("eye_per_view", C.c_int32)]


MESH_MAX = 1 << 24                      # vertices, faces and samples per view
MESH_WS_FWD, MESH_WS_BWD = 0, 1


class SrhSh9Params(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("n_points", C.c_int32),
                ("channels", C.c_int32), ("m_per_view", C.c_int32)]


SH9_MAX_CHANNELS, SH9_MAX = 4, 1 << 24  # channels; pixels of a probe and normals per view (MESH_MAX's value)
SH9_WS_PROJECT, SH9_WS_IRRADIANCE_BWD = 0, 1


def _p(struct):
    return C.POINTER(struct)


_V, _I, _Z = C.c_void_p, C.c_int32, C.c_size_t
# what the single-frame entry points start with, and the batched ones after their n_views
_FRAME = [_p(SrhCamera), _p(SrhObjects), _p(SrhLights), _p(SrhMaterials), _p(SrhParams), _V, _Z]
_SPLAT = [_p(SrhSplatParams), _p(SrhSplatInputs), _p(SrhLights), _p(SrhMaterials)]
_SPLAT_NDC = [_p(SrhSplatNdcParams), _p(SrhSplatNdcInputs), _p(SrhLights), _p(SrhMaterials)]

# name -> (restype, argtypes): every entry point of include/srh.h, in its order (tests/test_abi.py compares the two)
SIGNATURES = {
    "srh_abi_version": (C.c_int, []),
    "srh_last_error": (C.c_char_p, []),
    "srh_workspace_bytes": (_Z, [_p(SrhObjects), _I, _I]),
    "srh_generate_rays": (C.c_int, [_p(SrhCamera), _I, _I, _V, _V]),
    "srh_render_fwd": (C.c_int, _FRAME + [_V] * 4),
    "srh_render_bwd": (C.c_int, _FRAME + [_V] * 4 + [_p(SrhGrads), _V]),
    "srh_render_bwd_aux": (C.c_int, _FRAME + [_V] * 6 + [_p(SrhGrads), _V]),
    "srh_camera_grad_scratch_bytes": (_Z, [_I, _I]),
    "srh_render_bwd_camera": (C.c_int, _FRAME + [_V] * 6 + [_p(SrhGrads), _p(SrhCameraGrads), _V, _Z, _V]),
    "srh_workspace_bytes_views": (_Z, [_p(SrhObjects), _I, _I, _I]),
    "srh_render_views": (C.c_int, [_I] + _FRAME + [_V] * 4),
    "srh_render_views_aux": (C.c_int, [_I] + _FRAME + [_V] * 6),
    "srh_render_views_bwd": (C.c_int, [_I] + _FRAME + [_V] * 4 + [_p(SrhGrads), _V]),
    "srh_camera_grad_scratch_bytes_views": (_Z, [_I, _I, _I]),
    "srh_render_views_bwd_camera": (C.c_int, [_I] + _FRAME + [_V] * 6 + [_p(SrhGrads), _p(SrhCameraGrads), _V, _Z, _V]),
    "srh_shadow_workspace_bytes": (_Z, [_p(SrhObjects), _I, _I, _I]),
    "srh_shadow_shade": (C.c_int, _FRAME + [_V] * 5),
    "srh_bin_counters": (C.c_int, [_p(SrhObjects), _I, _I, _I, _I, _p(_Z), _p(_I), _p(_I), _p(_I), _p(_I)]),
    "srh_camera_ray_flags": (C.c_int, [_p(SrhCamera), _I, _p(_I)]),
    "srh_event_create": (C.c_int, [_p(_V)]),
    "srh_event_destroy": (C.c_int, [_V]),
    "srh_event_elapsed_ms": (C.c_int, [_V, _V, _p(C.c_float)]),
    "srh_splat_workspace_bytes": (_Z, _SPLAT[:2]),
    "srh_splat_fwd": (C.c_int, _SPLAT + [_V] * 5),
    "srh_splat_bwd": (C.c_int, _SPLAT + [_V, _Z] + [_V] * 4 + [_p(SrhSplatGrads), _V]),
    "srh_splat_ndc_fwd": (C.c_int, _SPLAT_NDC + [_V] * 4),
    "srh_splat_ndc_bwd": (C.c_int, _SPLAT_NDC + [_V] * 3 + [_p(SrhSplatNdcGrads), _V]),
    "srh_regularizers_workspace_bytes": (_Z, [_I, _I, _I]),
    "srh_regularizers_fwd": (C.c_int, [_p(SrhRegularizerParams)] + [_V] * 5 + [_Z] + [_V] * 3),
    "srh_regularizers_bwd": (C.c_int, [_p(SrhRegularizerParams)] + [_V] * 11),
    "srh_projection_workspace_bytes": (_Z, [_p(SrhProjectionParams), _I]),
    "srh_projection_keys": (C.c_int, [_p(SrhProjectionParams), _V, _V, _V, _Z, _V, _V]),
    "srh_projection_fwd": (C.c_int, [_p(SrhProjectionParams)] + [_V] * 5 + [_Z, _V, _Z] + [_V] * 5),
    "srh_projection_bwd": (C.c_int, [_p(SrhProjectionParams)] + [_V] * 5 + [_Z, _V, _Z] + [_V] * 8),
    "srh_view_grad_workspace_bytes": (_Z, [_I, _I, _I]),
    "srh_projection_bwd_view": (C.c_int, [_p(SrhProjectionParams)] + [_V] * 5 + [_Z, _V, _Z] + [_V] * 9 + [_Z, _V]),
    "srh_reverse_projection_workspace_bytes": (_Z, [_p(SrhReverseProjectionParams), _I]),
    "srh_reverse_projection_fwd": (C.c_int, [_p(SrhReverseProjectionParams)] + [_V] * 8 + [_Z] + [_V] * 5),
    "srh_reverse_projection_keys": (C.c_int, [_p(SrhReverseProjectionParams), _V, _V, _V, _Z, _V, _V]),
    "srh_reverse_projection_bwd": (C.c_int, [_p(SrhReverseProjectionParams)] + [_V] * 9 + [_Z] + [_V] * 8),
    "srh_reverse_projection_bwd_view": (C.c_int, [_p(SrhReverseProjectionParams)] + [_V] * 9 + [_Z] + [_V] * 10
                                        + [_Z, _V]),
    "srh_dense_projection_workspace_bytes": (_Z, [_p(SrhDenseProjectionParams), _I]),
    "srh_dense_projection_fwd": (C.c_int, [_p(SrhDenseProjectionParams)] + [_V] * 5 + [_Z, _V, _Z] + [_V] * 3),
    "srh_dense_projection_bwd": (C.c_int, [_p(SrhDenseProjectionParams)] + [_V] * 5 + [_Z, _V, _Z] + [_V] * 6),
    "srh_dense_projection_bwd_view": (C.c_int, [_p(SrhDenseProjectionParams)] + [_V] * 5 + [_Z, _V, _Z] + [_V] * 7
                                      + [_Z, _V]),
    "srh_depth_to_surfels_fwd": (C.c_int, [_p(SrhSurfelsParams)] + [_V] * 4),
    "srh_depth_to_surfels_bwd": (C.c_int, [_p(SrhSurfelsParams)] + [_V] * 5),
    "srh_depth_to_surfels_bwd_view": (C.c_int, [_p(SrhSurfelsParams)] + [_V] * 6 + [_Z, _V]),
    "srh_hard_projection_keys": (C.c_int, [_p(SrhHardProjectionParams)] + [_V] * 4),
    "srh_hard_projection_fwd": (C.c_int, [_p(SrhHardProjectionParams)] + [_V] * 7),
    "srh_hard_projection_bwd": (C.c_int, [_p(SrhHardProjectionParams)] + [_V] * 5),
    "srh_normals_workspace_bytes": (_Z, [_I, _I, _I]),
    "srh_normals_fwd": (C.c_int, [_I, _I, _I] + [_V] * 4),
    "srh_normals_bwd": (C.c_int, [_I, _I, _I] + [_V] * 4 + [_Z, _V, _V]),
    "srh_normals_bwd_view": (C.c_int, [_I, _I, _I] + [_V] * 4 + [_Z, _V, _V, _V, _Z, _V]),
    "srh_splat_bwd_view": (C.c_int, _SPLAT + [_V, _Z] + [_V] * 4 + [_p(SrhSplatGrads), _V, _V, _Z, _V]),
    "srh_splat_ndc_bwd_view": (C.c_int, _SPLAT_NDC + [_V] * 3 + [_p(SrhSplatNdcGrads), _V, _V, _Z, _V]),
    "srh_frame_transform_fwd": (C.c_int, [_p(SrhFrameParams)] + [_V] * 7),
    "srh_frame_transform_bwd": (C.c_int, [_p(SrhFrameParams)] + [_V] * 7),
    "srh_frame_transform_bwd_view": (C.c_int, [_p(SrhFrameParams)] + [_V] * 11 + [_Z, _V]),
    "srh_project_coordinates_fwd": (C.c_int, [_p(SrhProjectCoordsParams)] + [_V] * 6),
    "srh_project_coordinates_bwd": (C.c_int, [_p(SrhProjectCoordsParams)] + [_V] * 6),
    "srh_project_coordinates_bwd_view": (C.c_int, [_p(SrhProjectCoordsParams)] + [_V] * 7 + [_Z, _V]),
    "srh_nearest_points_fwd": (C.c_int, [_p(SrhPointSetParams)] + [_V] * 7),
    "srh_nearest_points_bwd": (C.c_int, [_p(SrhPointSetParams)] + [_V] * 11),
    "srh_mesh_sample_workspace_bytes": (_Z, [_p(SrhMeshSampleParams), _I]),
    "srh_mesh_sample_fwd": (C.c_int, [_p(SrhMeshSampleParams)] + [_V] * 5 + [_Z] + [_V] * 5),
    "srh_mesh_sample_bwd": (C.c_int, [_p(SrhMeshSampleParams)] + [_V] * 9 + [_Z] + [_V] * 2),
    "srh_sh9_workspace_bytes": (_Z, [_p(SrhSh9Params), _I]),
    "srh_sh9_project_fwd": (C.c_int, [_p(SrhSh9Params), _V, _V, _Z, _V, _V]),
    "srh_sh9_project_bwd": (C.c_int, [_p(SrhSh9Params)] + [_V] * 3),
    "srh_sh9_irradiance_fwd": (C.c_int, [_p(SrhSh9Params)] + [_V] * 4),
    "srh_sh9_irradiance_bwd": (C.c_int, [_p(SrhSh9Params)] + [_V] * 6 + [_Z, _V]),
}
EXPORTS = tuple(SIGNATURES)

_lib: Optional[C.CDLL] = None


class SrhError(RuntimeError):
    """A libsrh entry point returned non-zero."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libsrh error {code}: {message}")
        self.code = code


def lib_path() -> str:
    """In-tree libsrh.so; SRH_LIB points experiments (kernel A/B builds) at another build of the same ABI."""
    return os.environ.get("SRH_LIB") or _build.LIB_PATH


def load(build_if_missing: bool = True) -> C.CDLL:
    """dlopen libsrh.so (building it with hipcc first if it is absent and a toolchain exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise RuntimeError(f"{path} is missing; run `python -m surf_renderer_amd.build`")
        _build.build_lib()
    # torch first: the device buffers this library is handed come from torch's HIP runtime, and the process must hold
    # ONE runtime -- dlopening libsrh.so before torch pulls in the system's libamdhip64, torch then brings its own, and
    # every launch ends in "no ROCm-capable device is detected" (seen with build() followed by smoke() in one process)
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        if not hasattr(lib, name):
            raise RuntimeError(f"{path} does not export {name}")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    got = lib.srh_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {got}, this package expects {ABI_VERSION}; rebuild it")
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != 0:
        raise SrhError(code, load().srh_last_error().decode("utf-8", "replace"))


class EventPair:
    """Two timing-enabled HIP events recorded by libsrh around a frame's dominant kernel."""

    def __init__(self):
        lib = load()
        self.start, self.stop = C.c_void_p(), C.c_void_p()
        check(lib.srh_event_create(C.byref(self.start)))
        check(lib.srh_event_create(C.byref(self.stop)))

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        check(load().srh_event_elapsed_ms(self.start, self.stop, C.byref(ms)))
        return float(ms.value)

    def close(self) -> None:
        lib = load()
        for ev in (self.start, self.stop):
            if ev:
                lib.srh_event_destroy(ev)
        self.start = self.stop = C.c_void_p()
