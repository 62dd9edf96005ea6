// libsrh.so -- MI355X (gfx950) render(scene) backend: the host layer and the C ABI declared in include/srh.h.  The
// kernels live in the headers: srh_prep.h (per-frame records and binning), srh_allpairs.h (rays, exact, ortho, fast),
// srh_binned.h (the tile-binned render kernel), srh_backward.h, srh_shadow.h, srh_splat.h, srh_regularizers.h, srh_projection.h,
// srh_reverse_projection.h, srh_dense_projection.h, srh_splat_ndc.h, srh_surfels.h, srh_hard_projection.h, srh_normals.h,
// srh_frames.h, srh_pointsets.h, srh_mesh.h.
//
// Launch structure of one frame (all on the caller's stream, no host sync):
//   k_prep        one thread per primitive: per-frame records (unit normal, plane offset, eye-relative
//                 centre, ...) in fp64, plus the fp32 reject records of the FAST mode
//   k_render_*    the frame's pixels, in the mode the caller asked for
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <mutex>
#include <type_traits>

#include "srh.h"
#include "srh_device.h"
#include "srh_reject.h"
#include "srh_binned.h"
#include "srh_prep.h"
#include "srh_allpairs.h"
#include "srh_backward.h"
#include "srh_shadow.h"
#include "srh_splat.h"
#include "srh_splat_ndc.h"
#include "srh_regularizers.h"
#include "srh_projection.h"
#include "srh_reverse_projection.h"
#include "srh_dense_projection.h"
#include "srh_surfels.h"
#include "srh_hard_projection.h"
#include "srh_normals.h"
#include "srh_frames.h"
#include "srh_pointsets.h"
#include "srh_mesh.h"
#include "srh_sh9.h"

using namespace srh;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

// what every entry point returns after its launches
int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SRH_OK : hip_fail(e, what);
}

constexpr size_t kAlign = 256;
size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// ------------------------------------------------------------------------------------------------
// argument checks and camera arithmetic the entry points share (no HIP call)
// ------------------------------------------------------------------------------------------------
// the first NULL among a list of named pointers, in the order given
struct NamedPtr {
  const char* name;
  const void* ptr;
};
int check_not_null(std::initializer_list<NamedPtr> ptrs) {
  for (const NamedPtr& a : ptrs)
    if (!a.ptr) return fail(SRH_E_NULL, "%s is NULL", a.name);
  return SRH_OK;
}

// A fused layer's batch of frames: n_views in 1..65535 (grid dimension y), sides of at least 1, W H <= 1 << 24.  `what`
// names the frame in the message.  In two halves, for a layer with a test of its own between them (reg_check_grid).
int check_n_views(int32_t n_views) {
  if (n_views < 1 || n_views > 65535) return fail(SRH_E_RANGE, "n_views = %d, expected 1..65535", n_views);
  return SRH_OK;
}
int check_grid_size(int32_t width, int32_t height, const char* what) {
  if (width < 1 || height < 1 || (int64_t)width * height > (1 << 24))
    return fail(SRH_E_RANGE, "%s %d x %d out of range", what, width, height);
  return SRH_OK;
}
int check_batch_grid(int32_t n_views, int32_t width, int32_t height, const char* what) {
  if (int rc = check_n_views(n_views)) return rc;
  return check_grid_size(width, height, what);
}

// a device scratch buffer of fp64 records: `name` for the message
int check_scratch(const char* name, const void* ws, size_t bytes, size_t need) {
  if (!ws || bytes < need || ((uintptr_t)ws % sizeof(double)))
    return fail(SRH_E_WORKSPACE, "%s: need %zu bytes, 8-byte aligned (got %zu at %p)", name, need, bytes, ws);
  return SRH_OK;
}

// The pinhole frame at the focal distance: h = 2 f tan(fovy / 2), w = h W / H, in the reference's order of operations
// (numpy/renderer.py:145-163, torch/renderer.py, project_image_coordinates).  Every entry point that needs the frame
// size takes it from here.
struct FrameSize {
  double w, h;
};
FrameSize frame_size(double fovy, double focal_length, int W, int H) {
  const double h = tan(fovy / 2) * 2 * focal_length;
  return {h * ((double)W / (double)H), h};
}

// project_image_coordinates: pixel = x (-(W - 1) / w) + W / 2 with x = f X / Z (y likewise, not mirrored), less the half
// pixel: u = fsx X / Z + cx0, v = fsy Y / Z + cy0
struct PixelScales {
  double fsx, fsy, cx0, cy0;
};
PixelScales pixel_scales(double fovy, double focal_length, int W, int H) {
  const FrameSize fs = frame_size(fovy, focal_length, W, H);
  return {focal_length * (-(double)(W - 1) / fs.w), focal_length * ((double)(H - 1) / fs.h), W / 2.0 - 0.5, H / 2.0 - 0.5};
}

// the projection layers' camera: `suffix` completes the parameter names in the messages ("", "1", "2")
int check_pinhole(const char* suffix, double fovy, double focal_length) {
  if (!(fovy > 0.0 && fovy < 3.14159265358979323846))
    return fail(SRH_E_CAMERA, "fovy%s = %g, expected 0 < fovy < pi", suffix, fovy);
  if (!(focal_length > 0.0 && std::isfinite(focal_length)))
    return fail(SRH_E_CAMERA, "focal_length%s = %g, expected positive and finite", suffix, focal_length);
  return SRH_OK;
}

// ------------------------------------------------------------------------------------------------
// launch shapes and typed launches
// ------------------------------------------------------------------------------------------------
// The per-pixel kernels' launch: one 64 x 4-thread workgroup per 64 * P x 4 pixels (P columns per lane: k_render_fast).
// The camera-gradient scratch holds one set of partial sums per workgroup of this grid.
struct PixelGrid {
  dim3 block, grid;
  size_t groups() const { return (size_t)grid.x * grid.y; }
};
PixelGrid pixel_grid(int32_t width, int32_t rows, int P = 1) {
  return {dim3(64, 4), dim3((width + 64 * P - 1) / (64 * P), (rows + 3) / 4)};
}
PixelGrid pixel_grid(const FrameDev& F, int P = 1) { return pixel_grid(F.W, F.row1 - F.row0, P); }

// f(std::integral_constant<int, T>) for the primitive type T = `type` (validated by check_objects)
template <class Fn>
void with_prim_type(int type, Fn f) {
  switch (type) {
    case SRH_PRIM_DISK: f(std::integral_constant<int, SRH_PRIM_DISK>{}); break;
    case SRH_PRIM_PLANE: f(std::integral_constant<int, SRH_PRIM_PLANE>{}); break;
    case SRH_PRIM_SPHERE: f(std::integral_constant<int, SRH_PRIM_SPHERE>{}); break;
    default: f(std::integral_constant<int, SRH_PRIM_TRIANGLE>{}); break;
  }
}

// k_prep of batch s: the instantiation for the batch's type
void launch_prep(const FrameDev& F, int s, hipStream_t st) {
  const SegDev& S = F.seg[s];
  const dim3 grid((S.count + kBinBlock - 1) / kBinBlock), block(kBinBlock);
  with_prim_type(S.type, [&](auto type) {
    hipLaunchKernelGGL(k_prep<decltype(type)::value>, grid, block, 0, st, F, s, (double*)S.rec64, (float*)S.rec32);
  });
}
void launch_prep_views(const FrameDev& F0, const FrameDev* Fs, int s, int V, hipStream_t st) {
  const dim3 grid((F0.seg[s].count + kBinBlock - 1) / kBinBlock, V), block(kBinBlock);
  with_prim_type(F0.seg[s].type, [&](auto type) {
    hipLaunchKernelGGL(k_prep_views<decltype(type)::value>, grid, block, 0, st, Fs, s);
  });
}

// The two families of the binned render kernel, as launch_binned takes them
struct BinnedMem {
  template <bool TCH, int WPT, int BATCH>
  static constexpr auto kernel = &k_render_binned_mem<TCH, WPT, BATCH>;
};
struct BinnedViews {
  template <bool TCH, int WPT, int BATCH>
  static constexpr auto kernel = &k_render_binned_views<TCH, WPT, BATCH>;
};

// The binned render kernel of frame F (of grid_y views shaped like F) with the kernel's own arguments `args`.
// One wave per tile while that still gives every SIMD several waves, four waves per tile for small frames / slabs:
// SrhParams.waves_per_tile (1 or 4) decides, else the caller's `auto_split`.
template <class Family, class... Args>
void launch_binned(const FrameDev& F, int waves_per_tile, bool auto_split, unsigned grid_y, hipStream_t st, Args... args) {
  const bool split = (waves_per_tile == 1 || waves_per_tile == 4) ? waves_per_tile == 4 : auto_split;
  // whole regions of tiles, a multiple of 8 of them (see binned_grid)
  const dim3 grid(binned_grid(F) * 4, grid_y), block(split ? 256 : 64);
  // one object batch of a known type: the instantiation without per-batch generality and without the other types' code
  const int batch = F.nseg == 1 ? F.seg[0].type : -1;
  auto typed = [&](auto b) {
    auto launch = [&](auto tch, auto wpt) {
      hipLaunchKernelGGL((Family::template kernel<decltype(tch)::value, decltype(wpt)::value, decltype(b)::value>), grid,
                         block, 0, st, args...);
    };
    using One = std::integral_constant<int, 1>;
    using Four = std::integral_constant<int, 4>;
    if (F.shading) { if (split) launch(std::true_type{}, Four{}); else launch(std::true_type{}, One{}); }
    else { if (split) launch(std::false_type{}, Four{}); else launch(std::false_type{}, One{}); }
  };
  if (batch < 0) typed(std::integral_constant<int, -1>{});
  else with_prim_type(batch, typed);
}

template <int P>
void launch_fast(const FrameDev& F, hipStream_t st, float* image, float* depth, int32_t* nearest) {
  const PixelGrid pg = pixel_grid(F, P);
  hipLaunchKernelGGL(k_render_fast<P>, pg.grid, pg.block, 0, st, F, image, depth, nearest);
}

// ------------------------------------------------------------------------------------------------
// workspace layout, camera set-up and argument validation
// ------------------------------------------------------------------------------------------------
struct WsLayout {
  size_t off64[SRH_MAX_SEGMENTS];
  size_t off32[SRH_MAX_SEGMENTS];
  size_t lights64, frame, tilerange, neardist, counters, large, entries, entries_words;
  size_t counters_bytes;
  int tiles_x, tiles_y_max;
  size_t total;
};

int check_objects(const SrhObjects* ob) {
  if (!ob) return fail(SRH_E_NULL, "objects is NULL");
  if (ob->n_segments < 1 || ob->n_segments > SRH_MAX_SEGMENTS)
    return fail(SRH_E_RANGE, "n_segments = %d, expected 1..%d", ob->n_segments, SRH_MAX_SEGMENTS);
  long long total = 0;
  for (int s = 0; s < ob->n_segments; ++s) {
    const SrhSegment& g = ob->seg[s];
    if (g.type < 0 || g.type > 3) return fail(SRH_E_TYPE, "segment %d: unknown primitive type %d", s, g.type);
    if (g.count < 1) return fail(SRH_E_RANGE, "segment %d: count = %d (empty batches are not allowed)", s, g.count);
    if (!g.material_idx) return fail(SRH_E_NULL, "segment %d: material_idx is NULL", s);
    const bool need_pos = g.type != SRH_PRIM_TRIANGLE, need_nrm = g.type != SRH_PRIM_SPHERE;
    const bool need_rad = g.type == SRH_PRIM_DISK || g.type == SRH_PRIM_SPHERE;
    if (need_pos && !g.pos) return fail(SRH_E_NULL, "segment %d: pos is NULL", s);
    if (need_nrm && !g.normal) return fail(SRH_E_NULL, "segment %d: normal is NULL", s);
    if (need_rad && !g.radius) return fail(SRH_E_NULL, "segment %d: radius is NULL", s);
    if (g.type == SRH_PRIM_TRIANGLE && !g.face) return fail(SRH_E_NULL, "segment %d: face is NULL", s);
    total += g.count;
  }
  // tile-list offsets are 32-bit and every primitive may own up to kMaxTilesPerPrim list entries
  if (total > 0xffffffffLL / kMaxTilesPerPrim)
    return fail(SRH_E_RANGE, "too many primitives (%lld): at most %lld per scene", total, 0xffffffffLL / kMaxTilesPerPrim);
  return SRH_OK;
}

// The layout depends on the primitive counts and on the full frame size only (never on the row slab), so
// one workspace serves every slab of a frame.
WsLayout layout_for(const SrhObjects* ob, int width, int height) {
  WsLayout L;
  size_t off = 0, total = 0;
  L.lights64 = off;
  off = align_up(off + (size_t)SRH_MAX_LIGHTS * 6 * sizeof(double));
  L.frame = off;                                  // the frame's own constants, for the render kernel (FrameDev::self)
  off = align_up(off + sizeof(FrameDev));
  for (int s = 0; s < ob->n_segments; ++s) {
    const SrhSegment& g = ob->seg[s];
    L.off64[s] = off;
    off = align_up(off + (size_t)g.count * kRec64Stride[g.type] * sizeof(double));
    L.off32[s] = off;
    off = align_up(off + (size_t)g.count * kRec32Stride[g.type] * sizeof(float));
    total += (size_t)g.count;
  }
  L.tiles_x = (width + kTile - 1) / kTile;
  L.tiles_y_max = (height + kTile - 1) / kTile;
  const size_t ntiles = ((size_t)L.tiles_x * L.tiles_y_max + 3) / 4 * 4;
  L.tilerange = off;
  off = align_up(off + total * 4 * sizeof(uint16_t));
  L.counters = off;
  L.counters_bytes = (kCounterPad + SRH_MAX_SEGMENTS * ntiles) * sizeof(uint32_t);
  off = align_up(off + L.counters_bytes);
  L.large = off;
  off = align_up(off + total * sizeof(uint32_t));
  L.entries = off;
  // one-pass binning: every bin owns entries_words / nbins slots (at least kMinBinCap of them)
  L.entries_words = std::max(total * kMaxTilesPerPrim, (size_t)SRH_MAX_SEGMENTS * ntiles * kMinBinCap);
  off = align_up(off + L.entries_words * sizeof(uint32_t));
  L.neardist = off;                                // light views only (FrameDev::neardist); last, so that the regions a
  off = align_up(off + total * sizeof(float));     // primary frame touches keep their places
  L.total = off;
  return L;
}

// numpy/renderer.py:145-163 + numpy/ops.py:88-115 on the host, in fp64, same operation order.
int camera_to_frame(const SrhCamera* cam, FrameDev* F, bool orthonormal = false) {
  if (!cam) return fail(SRH_E_NULL, "camera is NULL");
  const int W = cam->viewport[2] - cam->viewport[0], H = cam->viewport[3] - cam->viewport[1];
  if (W < 1 || H < 1) return fail(SRH_E_RANGE, "empty viewport %d x %d", W, H);
  if (cam->eye[3] != 1.0) return fail(SRH_E_CAMERA, "camera.eye must have w == 1");
  if (cam->up[3] != 0.0) return fail(SRH_E_CAMERA, "camera.up must have w == 0");
  double z[4], zl = 0;
  for (int i = 0; i < 4; ++i) { z[i] = cam->eye[i] - cam->at[i]; zl += z[i] * z[i]; }
  zl = sqrt(zl);
  double ul = sqrt(cam->up[0] * cam->up[0] + cam->up[1] * cam->up[1] + cam->up[2] * cam->up[2]);
  if (!(zl > 0) || !(ul > 0)) return fail(SRH_E_CAMERA, "degenerate camera: eye == at or up == 0");
  double y[3];
  for (int i = 0; i < 3; ++i) { z[i] /= zl; y[i] = cam->up_is_unit ? cam->up[i] : cam->up[i] / ul; }
  double x[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
  if (orthonormal) {
    // torch backend (torch/utils.py:402-427): z = unit(eye - at), x = unit(cross(unit(up), z)), y = cross(z, x), where
    // unit is that backend's normalize (:135-139): v / sqrt(sum(v_i^2 + 1e-10)).  The eps leaves x and y 1.5e-10 short of
    // unit length: nothing an fp32 output shows, but a reflected ray that grazes the edge of a specular lobe
    // (rdotc = 3e-8) moves by 2 % of itself, and the gradient of rdotc ** 0.5 with it
    // (tests/test_hip_pow_paths.py::test_specular_lobe_backward).
    if (!(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] > 0))
      return fail(SRH_E_CAMERA, "degenerate camera: up is parallel to the view direction");
    auto unit_eps = [](double* v) {
      const double l = eps_len(v);
      for (int i = 0; i < 3; ++i) v[i] /= l;
    };
    double u[3];
    for (int i = 0; i < 3; ++i) { z[i] = cam->eye[i] - cam->at[i]; u[i] = cam->up[i]; }
    unit_eps(z);
    unit_eps(u);
    x[0] = u[1] * z[2] - u[2] * z[1];
    x[1] = u[2] * z[0] - u[0] * z[2];
    x[2] = u[0] * z[1] - u[1] * z[0];
    unit_eps(x);
    y[0] = z[1] * x[2] - z[2] * x[1];
    y[1] = z[2] * x[0] - z[0] * x[2];
    y[2] = z[0] * x[1] - z[1] * x[0];
  }
  const FrameSize fs = frame_size(cam->fovy, cam->focal_length, W, H);
  for (int i = 0; i < 3; ++i) { F->o[i] = cam->eye[i]; F->bx[i] = x[i]; F->by[i] = y[i]; F->bz[i] = z[i]; }
  F->half_w = fs.w / 2;
  F->half_h = fs.h / 2;
  F->focal = cam->focal_length;
  F->step_x = W > 1 ? 2.0 / (W - 1) : 0.0;
  F->step_y = H > 1 ? -2.0 / (H - 1) : 0.0;
  F->near_clip = cam->near_clip;
  F->far_clip = cam->far_clip;
  F->W = W;
  F->H = H;
  // pixel_ray's shared-reciprocal division is the IEEE division bit for bit as long as no operand needs rescaling:
  // true for ray components that are 0 or at least ~2^-150 in magnitude and lengths within 2^+-150, which camera
  // parameters of ordinary size guarantee (a cancelled component is 0 or >= 2^-53 of its terms)
  auto ordinary = [](double v) { const double a = std::fabs(v); return a == 0.0 || (a >= 1e-15 && a <= 1e15); };
  bool ok = ordinary(F->half_w) && F->half_w != 0.0 && ordinary(F->half_h) && F->half_h != 0.0 &&
            ordinary(F->focal) && F->focal != 0.0;
  for (int i = 0; i < 3; ++i) ok = ok && ordinary(F->bx[i]) && ordinary(F->by[i]) && ordinary(F->bz[i]);
  // Bit 1: |D|^2 is bounded over the whole frame, so the finish rounds' square root needs none of its range guards
  // (sqrt_bounded).  D = bx X + by Y - bz focal with |X| <= half_w, |Y| <= half_h.  Above: the triangle inequality.
  // Below: w = z - (z.y / y.y) y is orthogonal to y and (x being a cross product with z and y or their span) to x, so
  // D.w = -focal |w|^2 and |D| >= focal |w|, less what x.w and y.w are in fp64 instead of 0.  Admitted: 1e-100 <= |D| <=
  // 1e100 -- normal, finite, non-zero, |D|^2 far above 2^-767 -- and a lower bound no more than 1e6 below the upper
  // one, so that the rounding of this reckoning itself (1e-15 of the upper bound) cannot matter.
  bool bounded = ok;
  if (bounded) {
    auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const double *bx = F->bx, *by = F->by, *bz = F->bz;
    const double hw = std::fabs(F->half_w), hh = std::fabs(F->half_h), fl = std::fabs(F->focal);
    const double yy = dot(by, by), zy = dot(bz, by);
    double w[3];
    for (int i = 0; i < 3; ++i) w[i] = bz[i] - (yy > 0 ? zy / yy : 0.0) * by[i];
    const double wl = std::sqrt(dot(w, w));
    const double hi = hw * std::sqrt(dot(bx, bx)) + hh * std::sqrt(yy) + fl * std::sqrt(dot(bz, bz));
    const double lo = wl > 0 ? fl * wl - (hw * std::fabs(dot(bx, w)) + hh * std::fabs(dot(by, w))) / wl : 0.0;
    bounded = lo >= 1e-100 && hi <= 1e100 && lo >= 1e-6 * hi;        // false for a NaN anywhere
  }
  if (bounded && getenv("SRH_ROOT_GUARDS")) bounded = false;     // tests: the guarded root on a camera that needs none
  F->div_shared = ok ? (bounded ? 1 | kRootBounded : 1) : 0;
  F->ortho = cam->ortho ? 1 : 0;
  return SRH_OK;
}

int check_rows(const FrameDev& F, int row0, int row1) {
  if (row0 < 0 || row1 > F.H || row0 >= row1)
    return fail(SRH_E_RANGE, "row range [%d,%d) outside the %d image rows", row0, row1, F.H);
  return SRH_OK;
}

// what a shaded frame needs of its (non-NULL) lights and materials
int check_lights_materials(const SrhLights* lights, const SrhMaterials* materials) {
  if (lights->n_lights < 0 || lights->n_lights > SRH_MAX_LIGHTS)
    return fail(SRH_E_RANGE, "n_lights = %d, expected 0..%d", lights->n_lights, SRH_MAX_LIGHTS);
  if (lights->n_lights > 0 && (!lights->pos || !lights->color_idx || !lights->colors || lights->n_colors < 1))
    return fail(SRH_E_NULL, "lights arrays missing");
  if (materials->n_materials < 1 || !materials->albedo) return fail(SRH_E_NULL, "materials.albedo missing");
  return SRH_OK;
}

// Validation and per-frame constants shared by the forward and the backward entry points.
int setup_frame(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                FrameDev* Fp, WsLayout* Lp) {
  FrameDev& F = *Fp;
  memset(&F, 0, sizeof(F));
  if (!params) return fail(SRH_E_NULL, "params is NULL");
  if (params->shading != SRH_SHADING_NUMPY && params->shading != SRH_SHADING_TORCH)
    return fail(SRH_E_TYPE, "unknown shading model %d", params->shading);
  int rc = camera_to_frame(camera, &F, params->shading == SRH_SHADING_TORCH);
  if (rc) return rc;
  if ((rc = check_objects(objects))) return rc;
  if (!lights || !materials) return fail(SRH_E_NULL, "lights / materials is NULL");
  if ((rc = check_rows(F, params->row0, params->row1))) return rc;
  if ((rc = check_lights_materials(lights, materials))) return rc;
  if (params->mode < SRH_MODE_AUTO || params->mode > SRH_MODE_BINNED) return fail(SRH_E_TYPE, "unknown mode %d", params->mode);
  const WsLayout L = layout_for(objects, F.W, F.H);
  *Lp = L;
  if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace % kAlign) != 0)
    return fail(SRH_E_WORKSPACE, "workspace: need %zu bytes, 256-byte aligned (got %zu at %p)", L.total,
                workspace_bytes, workspace);
  F.row0 = params->row0;
  F.row1 = params->row1;
  F.gamma = params->gamma;
  F.tonemap = params->tonemap_gamma ? 1 : 0;
  F.img_stride = params->image_row_stride ? params->image_row_stride : 3 * (int64_t)F.W;
  F.depth_stride = params->depth_row_stride ? params->depth_row_stride : (int64_t)F.W;
  F.near_stride = params->nearest_row_stride ? params->nearest_row_stride : (int64_t)F.W;
  if (F.img_stride < 3 * (int64_t)F.W || F.depth_stride < F.W || F.near_stride < F.W)
    return fail(SRH_E_RANGE, "output row strides shorter than a row");
  F.nseg = objects->n_segments;
  F.nlights = lights->n_lights;
  F.ncolors = lights->n_colors;
  F.nmat = materials->n_materials;
  F.lpos = lights->pos;
  F.lcidx = lights->color_idx;
  F.colors = lights->colors;
  F.albedo = materials->albedo;
  F.shading = params->shading;
  F.double_sided = params->double_sided ? 1 : 0;
  F.use_quartic = params->use_quartic ? 1 : 0;
  F.latt = lights->attenuation;
  F.ambient = lights->ambient;
  F.coeffs = materials->coeffs;
  F.normal_out = params->normal_out;
  F.pos_out = params->pos_out;
  F.lights64 = (const double*)((char*)workspace + L.lights64);
  int first = 0;
  for (int s = 0; s < F.nseg; ++s) {
    const SrhSegment& g = objects->seg[s];
    SegDev& S = F.seg[s];
    S.type = g.type;
    S.count = g.count;
    S.first = first;
    S.rec64 = (const double*)((char*)workspace + L.off64[s]);
    S.rec32 = (const float*)((char*)workspace + L.off32[s]);
    S.pos = g.pos;
    S.normal = g.normal;
    S.radius = g.radius;
    S.face = g.face;
    S.mat = g.material_idx;
    first += g.count;
  }
  F.total = first;
  return SRH_OK;
}

// Tile-binning fields of a frame whose primitive records live in `workspace` (layout L).
// Fails the call where the counter region is not 8-byte aligned: bin_place claims two adjacent bin counters with one
// 64-bit atomic (srh_binned.h).
int setup_binning(FrameDev& F, const WsLayout& L, void* workspace) {
  if (((uintptr_t)workspace + L.counters) % 8 != 0)
    return fail(SRH_E_WORKSPACE, "workspace: the bin counters at %p + %zu are not 8-byte aligned", workspace, L.counters);
  F.tiles_x = L.tiles_x;
  F.tiles_y = (F.row1 - F.row0 + kTile - 1) / kTile;
  F.ntiles = F.tiles_x * F.tiles_y;
  F.ntiles_pad = (F.ntiles + 3) / 4 * 4;                         // a multiple of 4: every batch's counters start on 16 bytes
  F.nbins = F.nseg * F.ntiles_pad;
  F.bin_cap = (int32_t)std::min<size_t>(L.entries_words / (size_t)F.nbins, 1u << 20);
  char* ws = (char*)workspace;
  F.tilerange = (uint16_t*)(ws + L.tilerange);
  F.neardist = (float*)(ws + L.neardist);
  F.counters = (uint32_t*)(ws + L.counters);
  F.large = (uint32_t*)(ws + L.large);
  F.entries = (uint32_t*)(ws + L.entries);
  F.slab_cull = 0;
  if (F.row0 > 0 || F.row1 < F.H) {
    // rows of [D0 Dc Dr]^-1 via the adjugate (cross products)
    const PixelBasis B = pixel_basis(F);
    const double* p0 = B.D0; const double* pc = B.Dc; const double* pr = B.Dr;
    const double cx[3] = {pc[1] * pr[2] - pc[2] * pr[1], pc[2] * pr[0] - pc[0] * pr[2], pc[0] * pr[1] - pc[1] * pr[0]};
    const double cg[3] = {p0[1] * pc[2] - p0[2] * pc[1], p0[2] * pc[0] - p0[0] * pc[2], p0[0] * pc[1] - p0[1] * pc[0]};
    const double det = p0[0] * cx[0] + p0[1] * cx[1] + p0[2] * cx[2];
    if (std::isfinite(det) && std::fabs(det) > 0.0) {
      for (int k = 0; k < 3; ++k) { F.slab_ma[k] = cx[k] / det; F.slab_mg[k] = cg[k] / det; }
      F.slab_na = std::sqrt(F.slab_ma[0] * F.slab_ma[0] + F.slab_ma[1] * F.slab_ma[1] + F.slab_ma[2] * F.slab_ma[2]) * 1.000001;
      F.slab_ng = std::sqrt(F.slab_mg[0] * F.slab_mg[0] + F.slab_mg[1] * F.slab_mg[1] + F.slab_mg[2] * F.slab_mg[2]) * 1.000001;
      F.slab_cull = std::isfinite(F.slab_na) && std::isfinite(F.slab_ng) ? 1 : 0;
    }
  }
  return SRH_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int srh_abi_version(void) { return SRH_ABI_VERSION; }

const char* srh_last_error(void) { return g_err; }

size_t srh_workspace_bytes(const SrhObjects* objects, int32_t width, int32_t height) {
  if (check_objects(objects) != SRH_OK) return 0;
  const int64_t tiles_x = ((int64_t)width + kTile - 1) / kTile, tiles_y = ((int64_t)height + kTile - 1) / kTile;
  if (width < 1 || height < 1 || tiles_x * tiles_y > 65535LL * 65535LL || tiles_x > 65535 || tiles_y > 65535) {
    fail(SRH_E_RANGE, "frame size %d x %d out of range", width, height);
    return 0;
  }
  const WsLayout L = layout_for(objects, width, height);
  return L.total;
}

int srh_generate_rays(const SrhCamera* camera, int32_t row0, int32_t row1, float* ray_dir, void* stream) {
  FrameDev F;
  memset(&F, 0, sizeof(F));
  int rc = camera_to_frame(camera, &F);
  if (rc == SRH_OK && F.ortho) rc = fail(SRH_E_CAMERA, "srh_generate_rays: perspective cameras only");
  if (rc) return rc;
  if ((rc = check_rows(F, row0, row1))) return rc;
  if (!ray_dir) return fail(SRH_E_NULL, "ray_dir is NULL");
  F.row0 = row0;
  F.row1 = row1;
  const PixelGrid pg = pixel_grid(F);
  hipLaunchKernelGGL(k_rays, pg.grid, pg.block, 0, (hipStream_t)stream, F, ray_dir);
  return launch_status("k_rays launch");
}

int srh_render_fwd(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                   const SrhMaterials* materials, const SrhParams* params, void* workspace,
                   size_t workspace_bytes, float* image, float* depth, int32_t* nearest, void* stream) {
  FrameDev F;
  WsLayout L;
  int rc = setup_frame(camera, objects, lights, materials, params, workspace, workspace_bytes, &F, &L);
  if (rc) return rc;
  if (!image || !depth) return fail(SRH_E_NULL, "image / depth is NULL");
  if (F.ortho && params->shading != SRH_SHADING_TORCH)
    return fail(SRH_E_CAMERA, "orthographic projection exists only under SRH_SHADING_TORCH");
  // orthographic frames take the all-pairs fp64 kernel of their own, whatever mode is asked for
  const int mode = F.ortho ? SRH_MODE_EXACT : (params->mode == SRH_MODE_AUTO ? SRH_MODE_BINNED : params->mode);
  hipStream_t st = (hipStream_t)stream;
  // SrhParams.stages splits the frame for callers that pipeline it over two streams: SRH_STAGE_BIN = per-frame records
  // and tile bins into the workspace, SRH_STAGE_RENDER = the render kernel from bins a previous SRH_STAGE_BIN call with
  // the same arguments left there.  0 = both.
  const int stages = params->stages == 0 ? (SRH_STAGE_BIN | SRH_STAGE_RENDER) : params->stages;
  if (stages & ~(SRH_STAGE_BIN | SRH_STAGE_RENDER | SRH_STAGE_KEEP_BINS)) return fail(SRH_E_TYPE, "unknown stages mask %d", params->stages);
  if ((stages & (SRH_STAGE_BIN | SRH_STAGE_RENDER)) != (SRH_STAGE_BIN | SRH_STAGE_RENDER) && mode != SRH_MODE_BINNED)
    return fail(SRH_E_TYPE, "SrhParams.stages splits binned frames only");
  const bool run_binning = (stages & SRH_STAGE_BIN) != 0, run_render = (stages & SRH_STAGE_RENDER) != 0;
  if (mode == SRH_MODE_BINNED && (rc = setup_binning(F, L, workspace))) return rc;
  F.keep_bins = (stages & SRH_STAGE_KEEP_BINS) ? 1 : 0;
  if (mode == SRH_MODE_BINNED) F.self = (FrameDev*)((char*)workspace + L.frame);
  const bool counters_clean = params->counters_clean != 0;
  if (mode == SRH_MODE_BINNED && run_binning && !counters_clean) {
    // The bin counters start every frame at zero.  The render kernel leaves them that way (render_binned_body), so
    // a workspace that goes from frame to frame needs this launch only the first time (SrhParams.counters_clean).
    // A kernel, not hipMemsetAsync: captured into a hipGraph and replayed beside a live RCCL process group a memset
    // NODE did not take effect.
    const size_t ncount = (size_t)kCounterPad + (size_t)F.nbins;
    hipLaunchKernelGGL(k_zero_counters, dim3((unsigned)((ncount + 1023) / 1024)), dim3(256), 0, st, F.counters, (uint32_t)ncount);
  }

  for (int s = 0; s < F.nseg && run_binning; ++s) {
    launch_prep(F, s, st);
  }
  if (params->ev_start) (void)hipEventRecord((hipEvent_t)params->ev_start, st);
  if (mode == SRH_MODE_BINNED) {                 // the one mode that can come without its render stage
    // the render kernel reads the frame's constants from the workspace: k_prep of batch 0 put them there, unless this
    // call renders from bins an earlier call made
    if (run_render && !run_binning) hipLaunchKernelGGL(k_put_frame, dim3(1), dim3(64), 0, st, F);
    if (run_render)
      launch_binned<BinnedMem>(F, params->waves_per_tile, binned_waves_per_tile(F) == 4, 1, st, (FrameConstPtr)F.self,
                               image, depth, nearest);
  } else if (mode == SRH_MODE_EXACT) {
    const PixelGrid pg = pixel_grid(F);
    hipLaunchKernelGGL(F.ortho ? k_render_ortho : k_render_exact, pg.grid, pg.block, 0, st, F, image, depth, nearest);
  } else if (F.W >= 2048) {
    launch_fast<8>(F, st, image, depth, nearest);
  } else if (F.W >= 512) {
    launch_fast<4>(F, st, image, depth, nearest);
  } else {
    launch_fast<1>(F, st, image, depth, nearest);
  }
  if (params->ev_stop) (void)hipEventRecord((hipEvent_t)params->ev_stop, st);
  return launch_status("render launch");
}

// ---- many views of one scene per call ---------------------------------------------------------------------------
namespace {
// head of a views workspace: the views' FrameDev array and, for srh_render_views_bwd, their GradsDev array behind it
size_t views_header_bytes(int n_views) { return align_up((size_t)n_views * (sizeof(FrameDev) + sizeof(GradsDev))); }
// Frame descriptors of the batches in flight, PER DEVICE: a ring of kViewRing slots, each a pinned host staging area, a
// range of that device's constant-memory array g_view_frames (read by the render kernel) and an event that says "the
// batch that used this slot has finished".  The other kernels read the copy at the head of the caller's workspace.
// This is the one piece of state the library owns (include/srh.h, Conventions); it is created on first use of a
// device, lives until the process ends, and one mutex per device serialises claim + submit.
constexpr int kMaxDevices = 64;
struct ViewRing {
  std::mutex mu;
  FrameDev* stage[kViewRing] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t done[kViewRing] = {nullptr, nullptr, nullptr, nullptr};
  unsigned next = 0;
};
ViewRing g_rings[kMaxDevices];

// the device a call works on: the stream's own device when HIP can tell, else the calling thread's current device
int device_of(hipStream_t st, int* dev) {
  if (st && hipStreamGetDevice(st, dev) == hipSuccess) return SRH_OK;
  const hipError_t e = hipGetDevice(dev);
  return e == hipSuccess ? SRH_OK : hip_fail(e, "hipGetDevice");
}

// What srh_render_views and srh_render_views_bwd check about the stream before they stage descriptors: the device's
// ring, the device being current, and no capture in progress.
int views_ring(hipStream_t st, const char* who, const char* instead, ViewRing** ring) {
  int dev = 0;
  if (int rc = device_of(st, &dev)) return rc;
  if (dev < 0 || dev >= kMaxDevices) return fail(SRH_E_RANGE, "device %d: %s supports devices 0..%d", dev, who, kMaxDevices - 1);
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != dev)
    return fail(SRH_E_RANGE, "%s: the stream belongs to device %d but device %d is current", who, dev, cur);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (st && hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return fail(SRH_E_TYPE, "%s cannot be stream-captured (it waits on an event and stages through library-owned pinned "
                            "memory); capture %s calls instead", who, instead);
  *ring = &g_rings[dev];
  return SRH_OK;
}

// Claim the ring's next slot (ring.mu held): its previous batch must have finished -- a host wait only when kViewRing
// batches are behind.  A slot stages kMaxViewsPerCall FrameDev, behind them as many GradsDev (packed behind the FrameDev
// of the call's own n_views: one copy takes both), and behind room for kMaxViewsPerCall of each as many CamFinish.
constexpr size_t kStageFinish = (size_t)kMaxViewsPerCall * (sizeof(FrameDev) + sizeof(GradsDev));
constexpr size_t kStageBytes = kStageFinish + (size_t)kMaxViewsPerCall * sizeof(CamFinish);
static_assert(kStageFinish % alignof(CamFinish) == 0, "the CamFinish staging is aligned");
int claim_slot(ViewRing& ring, unsigned* slot_out) {
  const unsigned slot = ring.next % kViewRing;
  if (!ring.stage[slot]) {
    // staging first, then the event: a slot is usable only when it has both
    FrameDev* mem = nullptr;
    const hipError_t em = hipHostMalloc((void**)&mem, kStageBytes, hipHostMallocDefault);
    if (em != hipSuccess) return hip_fail(em, "hipHostMalloc(frames)");
    hipEvent_t ev = nullptr;
    const hipError_t ee = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (ee != hipSuccess) { (void)hipHostFree(mem); return hip_fail(ee, "hipEventCreate"); }
    ring.stage[slot] = mem;
    ring.done[slot] = ev;
  } else {
    const hipError_t es = hipEventSynchronize(ring.done[slot]);
    if (es != hipSuccess) return hip_fail(es, "hipEventSynchronize(slot)");
  }
  *slot_out = slot;
  return SRH_OK;
}

// The slot is consumed only after its launches: a call that failed validation leaves the ring as it was.
int release_slot(ViewRing& ring, unsigned slot, hipStream_t st) {
  const hipError_t er = hipEventRecord(ring.done[slot], st);
  ring.next++;
  if (er != hipSuccess) {
    // without the event nothing says when the staging may be reused: wait here, once, rather than race later
    (void)hipStreamSynchronize(st);
    return hip_fail(er, "hipEventRecord(slot)");
  }
  return SRH_OK;
}

// The arguments srh_render_views and srh_render_views_bwd share, and the checks both make of them before any HIP call.
struct ViewsCall {
  int32_t n_views;
  const SrhCamera* cameras;
  const SrhObjects* objects;
  const SrhLights* lights;
  const SrhMaterials* materials;
  const SrhParams* params;
  char* ws;
  size_t workspace_bytes;
  int W = 0, H = 0;
  size_t one = 0, head = 0;          // bytes of one view's workspace slice and of the header in front of the slices

  // view v's scene: the shared structs, or element v of the arrays SrhParams.per_view names
  const SrhObjects* objects_of(int v) const { return (params->per_view & SRH_VIEWS_OBJECTS) ? objects + v : objects; }
  const SrhLights* lights_of(int v) const { return (params->per_view & SRH_VIEWS_LIGHTS) ? lights + v : lights; }
  const SrhMaterials* materials_of(int v) const { return (params->per_view & SRH_VIEWS_MATERIALS) ? materials + v : materials; }
  char* slice(int v) const { return ws + head + (size_t)v * one; }

  // cameras, params and ws are not NULL
  int check(const char* who) {
    if (n_views < 1 || n_views > kMaxViewsPerCall)
      return fail(SRH_E_RANGE, "n_views = %d, expected 1..%d per call", n_views, kMaxViewsPerCall);
    if (params->normal_out || params->pos_out || params->ev_start || params->ev_stop)
      return fail(SRH_E_TYPE, "%s: normal / pos outputs and event hooks are per-frame features", who);
    W = cameras[0].viewport[2] - cameras[0].viewport[0];
    H = cameras[0].viewport[3] - cameras[0].viewport[1];
    if (!srh_workspace_bytes(objects, W, H)) return SRH_E_RANGE;   // validates, leaves the message
    one = layout_for(objects, W, H).total;
    if (params->per_view & ~(SRH_VIEWS_OBJECTS | SRH_VIEWS_LIGHTS | SRH_VIEWS_MATERIALS))
      return fail(SRH_E_TYPE, "unknown per_view mask %d", params->per_view);
    if (!lights || !materials) return fail(SRH_E_NULL, "lights / materials is NULL");
    if (params->per_view & SRH_VIEWS_OBJECTS)
      for (int v = 1; v < n_views; ++v) {     // one workspace layout, one kernel instantiation and one grid for the whole batch
        if (objects[v].n_segments != objects[0].n_segments)
          return fail(SRH_E_RANGE, "view %d has %d object batches, view 0 has %d", v, objects[v].n_segments, objects[0].n_segments);
        for (int s = 0; s < objects[0].n_segments; ++s)
          if (objects[v].seg[s].type != objects[0].seg[s].type || objects[v].seg[s].count != objects[0].seg[s].count)
            return fail(SRH_E_RANGE, "view %d, batch %d: type %d x %d, view 0 has type %d x %d", v, s, objects[v].seg[s].type,
                        objects[v].seg[s].count, objects[0].seg[s].type, objects[0].seg[s].count);
      }
    if (params->per_view & SRH_VIEWS_LIGHTS)
      for (int v = 1; v < n_views; ++v)
        if (lights[v].n_lights != lights[0].n_lights)
          return fail(SRH_E_RANGE, "view %d has %d lights, view 0 has %d", v, lights[v].n_lights, lights[0].n_lights);
    head = views_header_bytes(n_views);
    if (workspace_bytes < head + (size_t)n_views * one)
      return fail(SRH_E_RANGE, "workspace holds %zu bytes, %d views need %zu", workspace_bytes, n_views,
                  head + (size_t)n_views * one);
    if (cameras[0].ortho && params->shading != SRH_SHADING_TORCH)
      return fail(SRH_E_CAMERA, "orthographic projection exists only under SRH_SHADING_TORCH");
    return SRH_OK;
  }

  // view v's frame: its own rows (same count for every view) of a viewport like view 0's, records in its own workspace
  // slice, the projection of view 0
  int build_view(int v, FrameDev* F, WsLayout* L) const {
    const int w = cameras[v].viewport[2] - cameras[v].viewport[0], h = cameras[v].viewport[3] - cameras[v].viewport[1];
    if (w != W || h != H) return fail(SRH_E_RANGE, "view %d is %d x %d, view 0 is %d x %d", v, w, h, W, H);
    SrhParams pv = *params;
    if (params->view_row0) {
      pv.row0 = params->view_row0[v];
      pv.row1 = pv.row0 + (params->row1 - params->row0);
    }
    const int rc = setup_frame(&cameras[v], objects_of(v), lights_of(v), materials_of(v), &pv, slice(v), one, F, L);
    if (rc) return rc;
    const char* const kind[2] = {"perspective", "orthographic"};
    if (F->ortho != (cameras[0].ortho ? 1 : 0))
      return fail(SRH_E_CAMERA, "view %d is %s, view 0 %s: one projection per call", v, kind[F->ortho], kind[!F->ortho]);
    return SRH_OK;
  }
};
}  // namespace

size_t srh_workspace_bytes_views(const SrhObjects* objects, int32_t width, int32_t height, int32_t n_views) {
  if (!srh_workspace_bytes(objects, width, height)) return 0;        // validates, leaves the message
  const size_t one = layout_for(objects, width, height).total;
  if (n_views < 1 || n_views > kMaxViewsPerCall) {
    fail(SRH_E_RANGE, "n_views = %d, expected 1..%d per call", n_views, kMaxViewsPerCall);
    return 0;
  }
  return views_header_bytes(n_views) + (size_t)n_views * one;
}

// srh_render_views (normals = poses = NULL) and srh_render_views_aux: view v's normal / pos outputs are its slice of the
// stacked dense arrays, set in its frame descriptor as SrhParams.normal_out / pos_out set a single frame's
static int render_views(const char* who, int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects,
                        const SrhLights* lights, const SrhMaterials* materials, const SrhParams* params, void* workspace,
                        size_t workspace_bytes, float* images, float* depths, int32_t* nearests, float* normals,
                        float* poses, void* stream) {
  if (!cameras || !params || !workspace) return fail(SRH_E_NULL, "cameras / params / workspace is NULL");
  if (!images || !depths) return fail(SRH_E_NULL, "images / depths is NULL");
  if ((normals || poses) && params->shading != SRH_SHADING_TORCH)
    return fail(SRH_E_TYPE, "%s: normal / pos outputs exist only under SRH_SHADING_TORCH: normals / poses must be NULL", who);
  if (params->mode != SRH_MODE_AUTO && params->mode != SRH_MODE_BINNED)
    return fail(SRH_E_TYPE, "%s renders in the binned mode only", who);
  ViewsCall call{n_views, cameras, objects, lights, materials, params, (char*)workspace, workspace_bytes};
  if (int rc = call.check(who)) return rc;
  auto set_aux = [&](int v, FrameDev& F) {
    const size_t off = (size_t)v * (size_t)(F.row1 - F.row0) * (size_t)F.W * 3;
    F.normal_out = normals ? normals + off : nullptr;
    F.pos_out = poses ? poses + off : nullptr;
  };
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (cameras[0].ortho) {
    // Orthographic views (torch semantics): each view is the all-pairs fp64 frame of k_render_ortho -- its frame
    // constants travel as kernel arguments, so this branch needs no staging, no ring and no lock.
    const size_t rows = (size_t)(params->row1 - params->row0);
    for (int v = 0; v < n_views; ++v) {
      FrameDev F;
      WsLayout Lo;
      if (int rc = call.build_view(v, &F, &Lo)) return rc;
      set_aux(v, F);
      for (int s = 0; s < F.nseg; ++s) {
        launch_prep(F, s, st);
      }
      const PixelGrid pg = pixel_grid(F);
      hipLaunchKernelGGL(k_render_ortho, pg.grid, pg.block, 0, st, F, images + (size_t)v * rows * F.img_stride,
                         depths + (size_t)v * rows * F.depth_stride,
                         nearests ? nearests + (size_t)v * rows * F.near_stride : nullptr);
    }
    return launch_status("ortho views launch");
  }
  ViewRing* ringp = nullptr;
  if (int rc = views_ring(st, who, "srh_render_fwd", &ringp)) return rc;
  ViewRing& ring = *ringp;
  std::lock_guard<std::mutex> lock(ring.mu);
  unsigned slot = 0;
  if (int rc = claim_slot(ring, &slot)) return rc;
  FrameDev* stage = ring.stage[slot];
  WsLayout L;
  for (int v = 0; v < n_views; ++v) {
    if (int rc = call.build_view(v, &stage[v], &L)) return rc;
    set_aux(v, stage[v]);
    if (int rc = setup_binning(stage[v], L, call.slice(v))) return rc;
  }
  const FrameDev* Fs = (const FrameDev*)ws;
  hipError_t e = hipMemcpyAsync(ws, stage, (size_t)n_views * sizeof(FrameDev), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(frames)");
  const int base = (int)slot * kMaxViewsPerCall;
  e = hipMemcpyToSymbolAsync(HIP_SYMBOL(g_view_frames), stage, (size_t)n_views * sizeof(FrameDev),
                             (size_t)base * sizeof(FrameDev), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpyToSymbolAsync(frames)");
  const FrameDev& F0 = stage[0];
  const unsigned V = (unsigned)n_views;
  const size_t ncount = (size_t)kCounterPad + (size_t)F0.nbins;
  if (!params->counters_clean)               // as in srh_render_fwd: every view's render kernel leaves its counters at zero
    hipLaunchKernelGGL(k_views_zero, dim3((unsigned)((ncount + 255) / 256), V), dim3(256), 0, st, Fs);
  for (int s = 0; s < F0.nseg; ++s)
    launch_prep_views(F0, Fs, s, V, st);
  // all views share the GPU, so the batch as a whole decides the launch shape
  launch_binned<BinnedViews>(F0, params->waves_per_tile, (size_t)F0.ntiles * V < (size_t)kSplitTiles, V, st, base, images,
                             depths, nearests);
  if (int rc = release_slot(ring, slot, st)) return rc;
  return launch_status("views launch");
}

int srh_render_views(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects, const SrhLights* lights,
                     const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                     float* images, float* depths, int32_t* nearests, void* stream) {
  return render_views("srh_render_views", n_views, cameras, objects, lights, materials, params, workspace,
                      workspace_bytes, images, depths, nearests, nullptr, nullptr, stream);
}

int srh_render_views_aux(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects, const SrhLights* lights,
                         const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                         float* images, float* depths, int32_t* nearests, float* normals, float* poses, void* stream) {
  return render_views("srh_render_views_aux", n_views, cameras, objects, lights, materials, params, workspace,
                      workspace_bytes, images, depths, nearests, normals, poses, stream);
}

namespace {
// Workspace of the accelerated shadow pass: the primary frame's layout first (so a workspace sized by
// srh_workspace_bytes still serves the all-pairs fallback), then the light views' frame descriptors, the scene bounds,
// and one kShadowRes^2 binning slice per light.
struct ShadowLayout {
  WsLayout primary, slice;
  size_t frames, bounds, slices, total;
};
ShadowLayout shadow_layout_for(const SrhObjects* ob, int width, int height, int n_lights) {
  ShadowLayout S;
  S.primary = layout_for(ob, width, height);
  S.slice = layout_for(ob, kShadowRes, kShadowRes);
  size_t off = S.primary.total;
  S.frames = off;
  off = align_up(off + (size_t)SRH_MAX_LIGHTS * sizeof(FrameDev));
  S.bounds = off;
  off = align_up(off + 64 * sizeof(int));
  S.slices = off;
  S.total = off + (size_t)(n_lights > 0 ? n_lights : 0) * S.slice.total;
  return S;
}
}  // namespace

size_t srh_shadow_workspace_bytes(const SrhObjects* objects, int32_t width, int32_t height, int32_t n_lights) {
  if (!srh_workspace_bytes(objects, width, height)) return 0;        // validates, leaves the message
  if (n_lights < 0 || n_lights > SRH_MAX_LIGHTS) { fail(SRH_E_RANGE, "n_lights = %d, expected 0..%d", n_lights, SRH_MAX_LIGHTS); return 0; }
  // (never smaller than srh_workspace_bytes, whose per-tile table lies behind the primary layout: the forward pass may
  // render in this workspace)
  return std::max(shadow_layout_for(objects, width, height, n_lights).total, srh_workspace_bytes(objects, width, height));
}

int srh_shadow_shade(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                     const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                     const int32_t* nearest, const float* depth, float* image, uint64_t* visibility, void* stream) {
  FrameDev F;
  WsLayout L;
  int rc = setup_frame(camera, objects, lights, materials, params, workspace, workspace_bytes, &F, &L);
  if (rc) return rc;
  if (!nearest || !depth || !image) return fail(SRH_E_NULL, "nearest / depth / image is NULL");
  if (params->shading != SRH_SHADING_TORCH)
    return fail(SRH_E_TYPE, "shadow rays belong to SRH_SHADING_TORCH (the numpy backend has none)");
  hipStream_t st = (hipStream_t)stream;
  // the workspace may have served other frames since the forward pass: rebuild the fp64 records (no binning)
  for (int s = 0; s < F.nseg; ++s) {
    launch_prep(F, s, st);
  }
  const PixelGrid pg = pixel_grid(F);
  const ShadowLayout SL = shadow_layout_for(objects, F.W, F.H, F.nlights);
  const bool accelerated = params->mode != SRH_MODE_EXACT && F.nlights > 0 && workspace_bytes >= SL.total;
  if (!accelerated) {
    // all pairs (mode = SRH_MODE_EXACT asks for it; a workspace sized by srh_workspace_bytes has no room for the views)
    hipLaunchKernelGGL(k_shadow_shade, pg.grid, pg.block, 0, st, F, image, depth, nearest, visibility);
    return launch_status("shadow launch");
  }
  char* ws = (char*)workspace;
  FrameDev* frames = (FrameDev*)(ws + SL.frames);
  int* bounds = (int*)(ws + SL.bounds);
  // template of a light view: the primary frame's inputs and shading, a kShadowRes^2 viewport, slice 0's pointers
  FrameDev T = F;
  {
    SrhCamera dummy;
    memset(&dummy, 0, sizeof(dummy));
    dummy.eye[2] = 1.0; dummy.eye[3] = 1.0; dummy.at[3] = 1.0; dummy.up[1] = 1.0;
    dummy.fovy = 1.5707963267948966; dummy.focal_length = 1.0; dummy.near_clip = 1.0e-300; dummy.far_clip = 1.0e300;
    dummy.viewport[2] = kShadowRes; dummy.viewport[3] = kShadowRes;
    if ((rc = camera_to_frame(&dummy, &T, true))) return rc;
  }
  T.row0 = 0;
  T.row1 = kShadowRes;
  T.normal_out = nullptr;
  T.pos_out = nullptr;
  char* slice0 = ws + SL.slices;
  T.lights64 = (const double*)(slice0 + SL.slice.lights64);
  for (int s = 0; s < T.nseg; ++s) {
    T.seg[s].rec64 = (const double*)(slice0 + SL.slice.off64[s]);
    T.seg[s].rec32 = (const float*)(slice0 + SL.slice.off32[s]);
  }
  // (light l's slice starts l * SL.slice.total further on: a multiple of 256, so its counters keep the alignment)
  if ((rc = setup_binning(T, SL.slice, slice0))) return rc;
  T.bin_pad = 1.0;              // shadow rays cross the image plane between pixel centres
  T.near_ball = 0.1001;         // occluders up to 0.1 behind the light count (torch/renderer.py:299-306)
  const unsigned V = (unsigned)F.nlights;
  hipLaunchKernelGGL(k_bounds_init, dim3(1), dim3(64), 0, st, bounds);
  for (int s = 0; s < F.nseg; ++s)
    hipLaunchKernelGGL(k_scene_bounds, dim3((unsigned)std::min(kBoundsBlocks, (F.seg[s].count + 255) / 256)), dim3(256), 0, st, F, s, bounds);
  hipLaunchKernelGGL(k_light_frames, dim3((V + 63) / 64), dim3(64), 0, st, T, F.lpos, F.nlights, bounds, frames, SL.slice.total);
  const size_t ncount = (size_t)kCounterPad + (size_t)T.nbins;
  hipLaunchKernelGGL(k_views_zero, dim3((unsigned)((ncount + 255) / 256), V), dim3(256), 0, st, frames);
  for (int s = 0; s < T.nseg; ++s)
    launch_prep_views(T, frames, s, V, st);
  hipLaunchKernelGGL(k_shadow_shade_binned, pg.grid, pg.block, 0, st, F, frames, image, depth, nearest, visibility);
  return launch_status("shadow launch");
}

// workgroups of a backward launch over width x rows pixels (64 x 4 pixels each), and the bytes of their camera partials
static size_t camera_groups(int32_t width, int32_t rows) { return pixel_grid(width, rows).groups(); }
static size_t camera_scratch_bytes(int32_t width, int32_t rows) {
  return camera_groups(width, rows) * kCamSums * sizeof(double);
}

// where a backward adds its gradients, as the kernels take it (the torch shading's extra inputs only under `tch`)
static GradsDev grads_dev(const SrhGrads& g, bool tch) {
  GradsDev G;
  for (int s = 0; s < SRH_MAX_SEGMENTS; ++s) {
    G.pos[s] = g.pos[s]; G.normal[s] = g.normal[s]; G.radius[s] = g.radius[s]; G.face[s] = g.face[s];
  }
  G.lights_pos = g.lights_pos;
  G.colors = g.colors;
  G.albedo = g.albedo;
  G.coeffs = tch ? g.coeffs : nullptr;
  G.attenuation = tch ? g.attenuation : nullptr;
  G.ambient = tch ? g.ambient : nullptr;
  return G;
}

// srh_render_bwd (grad_normal = grad_pos = NULL), srh_render_bwd_aux and srh_render_bwd_camera (cam_part != NULL: the
// camera variant of the torch kernel, then k_camera_finish); the callers have checked which upstream gradients may be
// NULL, and the camera scratch
static int render_bwd(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                      const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                      const float* grad_image, const float* grad_depth, const float* grad_normal, const float* grad_pos,
                      const int32_t* nearest, const float* depth, const SrhGrads* grads, void* stream,
                      const SrhCameraGrads* camera_grads = nullptr, double* cam_part = nullptr) {
  FrameDev F;
  WsLayout L;
  int rc = setup_frame(camera, objects, lights, materials, params, workspace, workspace_bytes, &F, &L);
  if (rc) return rc;
  if (!nearest || !depth || !grads)
    return fail(SRH_E_NULL, "nearest / depth / grads is NULL");
  if (F.ortho && params->shading != SRH_SHADING_TORCH)
    return fail(SRH_E_CAMERA, "orthographic projection exists only under SRH_SHADING_TORCH");
  const bool tch = params->shading == SRH_SHADING_TORCH;
  const GradsDev G = grads_dev(*grads, tch);
  hipStream_t st = (hipStream_t)stream;
  // the workspace may have served other frames since the forward pass: rebuild the fp64 records (no binning)
  for (int s = 0; s < F.nseg; ++s) {
    launch_prep(F, s, st);
  }
  const PixelGrid pg = pixel_grid(F);
  if (params->ev_start) (void)hipEventRecord((hipEvent_t)params->ev_start, st);
  const uint64_t* vis = (const uint64_t*)params->visibility;
  const bool aux = grad_normal || grad_pos;
  if (!tch) {
    hipLaunchKernelGGL(k_render_bwd, pg.grid, pg.block, 0, st, F, G, grad_image, grad_depth, nearest, depth);
  } else {
    // <kAux, kImage, kCam>: the camera variants carry the aux gradients; without an image gradient the geometry-only
    // kernel runs (a depth-only call too, with both aux pointers NULL)
    const auto kernel = cam_part      ? (grad_image ? k_render_bwd_tch<true, true, true> : k_render_bwd_tch<true, false, true>)
                        : !grad_image ? k_render_bwd_tch<true, false>
                        : aux         ? k_render_bwd_tch<true, true>
                                      : k_render_bwd_tch<false, true>;
    hipLaunchKernelGGL(kernel, pg.grid, pg.block, 0, st, F, G, grad_image, grad_depth, nearest, depth, vis, grad_normal,
                       grad_pos, cam_part);
  }
  if (params->ev_stop) (void)hipEventRecord((hipEvent_t)params->ev_stop, st);
  if (cam_part) {
    CamFinish P;
    for (int k = 0; k < 3; ++k) { P.eye[k] = camera->eye[k]; P.at[k] = camera->at[k]; P.up[k] = camera->up[k]; }
    P.focal = F.focal;
    P.ortho = F.ortho;
    P.ngroups = (int32_t)camera_groups(F.W, F.row1 - F.row0);
    P.g_eye = camera_grads->eye; P.g_at = camera_grads->at; P.g_up = camera_grads->up;
    hipLaunchKernelGGL(k_camera_finish, dim3(1), dim3(1024), 0, st, P, cam_part);
  }
  return launch_status("backward launch");
}

int srh_render_bwd(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                   const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                   const float* grad_image, const float* grad_depth, const int32_t* nearest, const float* depth,
                   const SrhGrads* grads, void* stream) {
  if (!grad_image) return fail(SRH_E_NULL, "grad_image / nearest / depth / grads is NULL");
  return render_bwd(camera, objects, lights, materials, params, workspace, workspace_bytes, grad_image, grad_depth,
                    nullptr, nullptr, nearest, depth, grads, stream);
}

int srh_render_bwd_aux(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                       const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                       const float* grad_image, const float* grad_depth, const float* grad_normal,
                       const float* grad_pos, const int32_t* nearest, const float* depth, const SrhGrads* grads,
                       void* stream) {
  if (!grad_image && !grad_depth && !grad_normal && !grad_pos)
    return fail(SRH_E_NULL, "grad_image, grad_depth, grad_normal and grad_pos are all NULL");
  if (params && params->shading != SRH_SHADING_TORCH) {
    if (grad_normal || grad_pos)
      return fail(SRH_E_TYPE, "normal / pos outputs exist only under SRH_SHADING_TORCH: grad_normal / grad_pos must be NULL");
    if (!grad_image) return fail(SRH_E_NULL, "SRH_SHADING_NUMPY needs grad_image");
  }
  return render_bwd(camera, objects, lights, materials, params, workspace, workspace_bytes, grad_image, grad_depth,
                    grad_normal, grad_pos, nearest, depth, grads, stream);
}

size_t srh_camera_grad_scratch_bytes(int32_t width, int32_t rows) {
  if (width < 1 || rows < 1) { fail(SRH_E_RANGE, "camera gradient scratch for %d x %d pixels", width, rows); return 0; }
  return camera_scratch_bytes(width, rows);
}

int srh_render_bwd_camera(const SrhCamera* camera, const SrhObjects* objects, const SrhLights* lights,
                          const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                          const float* grad_image, const float* grad_depth, const float* grad_normal,
                          const float* grad_pos, const int32_t* nearest, const float* depth, const SrhGrads* grads,
                          const SrhCameraGrads* camera_grads, void* camera_scratch, size_t camera_scratch_size,
                          void* stream) {
  if (!grad_image && !grad_depth && !grad_normal && !grad_pos)
    return fail(SRH_E_NULL, "grad_image, grad_depth, grad_normal and grad_pos are all NULL");
  if (!params || !camera) return fail(SRH_E_NULL, "camera / params is NULL");
  if (params->shading != SRH_SHADING_TORCH)
    return fail(SRH_E_TYPE, "camera gradients exist only under SRH_SHADING_TORCH");
  if (!camera_grads) return fail(SRH_E_NULL, "camera_grads is NULL");
  if (!camera_grads->eye && !camera_grads->at && !camera_grads->up)         // nothing wanted: srh_render_bwd_aux
    return render_bwd(camera, objects, lights, materials, params, workspace, workspace_bytes, grad_image, grad_depth,
                      grad_normal, grad_pos, nearest, depth, grads, stream);
  const int32_t width = camera->viewport[2] - camera->viewport[0], rows = params->row1 - params->row0;
  if (width < 1 || rows < 1) return fail(SRH_E_RANGE, "empty frame %d x %d", width, rows);
  const size_t need = camera_scratch_bytes(width, rows);
  if (!camera_scratch || camera_scratch_size < need || ((uintptr_t)camera_scratch % sizeof(double)) != 0)
    return fail(SRH_E_WORKSPACE, "camera scratch: need %zu bytes, 8-byte aligned (got %zu at %p)", need,
                camera_scratch_size, camera_scratch);
  return render_bwd(camera, objects, lights, materials, params, workspace, workspace_bytes, grad_image, grad_depth,
                    grad_normal, grad_pos, nearest, depth, grads, stream, camera_grads, (double*)camera_scratch);
}

// head of a batch's camera scratch: the views' CamFinish array, in front of their slices of partial sums
static size_t camera_head_bytes(int n_views) { return align_up((size_t)n_views * sizeof(CamFinish)); }

size_t srh_camera_grad_scratch_bytes_views(int32_t width, int32_t rows, int32_t n_views) {
  if (width < 1 || rows < 1) { fail(SRH_E_RANGE, "camera gradient scratch for %d x %d pixels", width, rows); return 0; }
  if (n_views < 1 || n_views > kMaxViewsPerCall) {
    fail(SRH_E_RANGE, "n_views = %d, expected 1..%d per call", n_views, kMaxViewsPerCall);
    return 0;
  }
  return camera_head_bytes(n_views) + (size_t)n_views * camera_scratch_bytes(width, rows);
}

// srh_render_views_bwd (grad_normals = grad_poses = NULL, no camera) and srh_render_views_bwd_camera (camera_scratch !=
// NULL: the camera variant of the torch kernel for the whole batch, then k_camera_finish_views); the callers have checked
// the NULLs, which upstream gradients may be missing, and the camera scratch
static int render_views_bwd(const char* who, int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects,
                            const SrhLights* lights, const SrhMaterials* materials, const SrhParams* params,
                            void* workspace, size_t workspace_bytes, const float* grad_images, const float* grad_depths,
                            const float* grad_normals, const float* grad_poses, const int32_t* nearests,
                            const float* depths, const SrhGrads* grads, const SrhCameraGrads* camera_grads,
                            void* camera_scratch, void* stream) {
  ViewsCall call{n_views, cameras, objects, lights, materials, params, (char*)workspace, workspace_bytes};
  if (int rc = call.check(who)) return rc;
  const bool tch = params->shading == SRH_SHADING_TORCH;
  hipStream_t st = (hipStream_t)stream;
  ViewRing* ringp = nullptr;
  if (int rc = views_ring(st, who, "srh_render_bwd", &ringp)) return rc;
  ViewRing& ring = *ringp;
  std::lock_guard<std::mutex> lock(ring.mu);
  unsigned slot = 0;
  if (int rc = claim_slot(ring, &slot)) return rc;
  // the views' frames and, straight behind them, their gradient destinations: one copy to the head of the workspace
  FrameDev* stage = ring.stage[slot];
  GradsDev* gstage = (GradsDev*)(stage + n_views);
  CamFinish* cstage = (CamFinish*)((char*)stage + kStageFinish);
  SrhParams pv = *params;
  pv.mode = SRH_MODE_AUTO;                     // a backward bins nothing: whatever the forward ran in is accepted
  call.params = &pv;
  WsLayout L;
  for (int v = 0; v < n_views; ++v) {
    // records only (no setup_binning): k_prep_views then leaves the bin counters, the lists and F.self alone
    if (int rc = call.build_view(v, &stage[v], &L)) return rc;
    gstage[v] = grads_dev(grads[v], tch);
  }
  char* ws = (char*)workspace;
  hipError_t e = hipMemcpyAsync(ws, stage, (size_t)n_views * (sizeof(FrameDev) + sizeof(GradsDev)),
                                hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(frames, grads)");
  const FrameDev* Fs = (const FrameDev*)ws;
  const GradsDev* Gs = (const GradsDev*)(Fs + n_views);
  const FrameDev& F0 = stage[0];
  const unsigned V = (unsigned)n_views;
  const PixelGrid pg = pixel_grid(F0);
  double* cam_part = nullptr;
  if (camera_scratch) {
    // the finish descriptors travel in the head of the camera scratch, the partial sums of view v in slice v behind it
    for (int v = 0; v < n_views; ++v) {
      CamFinish& P = cstage[v];
      for (int k = 0; k < 3; ++k) { P.eye[k] = cameras[v].eye[k]; P.at[k] = cameras[v].at[k]; P.up[k] = cameras[v].up[k]; }
      P.focal = stage[v].focal;
      P.ortho = stage[v].ortho;
      P.ngroups = (int32_t)pg.groups();
      P.g_eye = camera_grads[v].eye; P.g_at = camera_grads[v].at; P.g_up = camera_grads[v].up;
    }
    e = hipMemcpyAsync(camera_scratch, cstage, (size_t)n_views * sizeof(CamFinish), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(camera finish)");
    cam_part = (double*)((char*)camera_scratch + camera_head_bytes(n_views));
  }
  for (int s = 0; s < F0.nseg; ++s)
    launch_prep_views(F0, Fs, s, V, st);
  const dim3 grid(pg.grid.x, pg.grid.y, V);
  if (!tch) {
    hipLaunchKernelGGL(k_render_bwd_views, grid, pg.block, 0, st, Fs, Gs, grad_images, grad_depths, nearests, depths,
                       (const uint64_t*)nullptr);
  } else {
    // <kAux, kImage, kCam>, chosen as render_bwd chooses the single frame's
    const bool aux = grad_normals || grad_poses;
    const auto kernel = cam_part      ? (grad_images ? k_render_bwd_tch_views<true, true, true> : k_render_bwd_tch_views<true, false, true>)
                        : !grad_images ? k_render_bwd_tch_views<true, false, false>
                        : aux          ? k_render_bwd_tch_views<true, true, false>
                                       : k_render_bwd_tch_views<false, true, false>;
    hipLaunchKernelGGL(kernel, grid, pg.block, 0, st, Fs, Gs, grad_images, grad_depths, nearests, depths,
                       (const uint64_t*)params->visibility, grad_normals, grad_poses, cam_part);
  }
  if (cam_part)
    hipLaunchKernelGGL(k_camera_finish_views, dim3(V), dim3(1024), 0, st, (const CamFinish*)camera_scratch,
                       (const double*)cam_part);
  if (int rc = release_slot(ring, slot, st)) return rc;
  return launch_status("views backward launch");
}

int srh_render_views_bwd(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects, const SrhLights* lights,
                         const SrhMaterials* materials, const SrhParams* params, void* workspace, size_t workspace_bytes,
                         const float* grad_images, const float* grad_depths, const int32_t* nearests, const float* depths,
                         const SrhGrads* grads, void* stream) {
  if (!cameras || !params || !workspace) return fail(SRH_E_NULL, "cameras / params / workspace is NULL");
  if (!grad_images || !nearests || !depths || !grads) return fail(SRH_E_NULL, "grad_images / nearests / depths / grads is NULL");
  return render_views_bwd("srh_render_views_bwd", n_views, cameras, objects, lights, materials, params, workspace,
                          workspace_bytes, grad_images, grad_depths, nullptr, nullptr, nearests, depths, grads, nullptr,
                          nullptr, stream);
}

int srh_render_views_bwd_camera(int32_t n_views, const SrhCamera* cameras, const SrhObjects* objects,
                                const SrhLights* lights, const SrhMaterials* materials, const SrhParams* params,
                                void* workspace, size_t workspace_bytes, const float* grad_images,
                                const float* grad_depths, const float* grad_normals, const float* grad_poses,
                                const int32_t* nearests, const float* depths, const SrhGrads* grads,
                                const SrhCameraGrads* camera_grads, void* camera_scratch, size_t camera_scratch_size,
                                void* stream) {
  if (!cameras || !params || !workspace) return fail(SRH_E_NULL, "cameras / params / workspace is NULL");
  if (!nearests || !depths || !grads) return fail(SRH_E_NULL, "nearests / depths / grads is NULL");
  if (!grad_images && !grad_depths && !grad_normals && !grad_poses)
    return fail(SRH_E_NULL, "grad_images, grad_depths, grad_normals and grad_poses are all NULL");
  if (n_views < 1 || n_views > kMaxViewsPerCall)
    return fail(SRH_E_RANGE, "n_views = %d, expected 1..%d per call", n_views, kMaxViewsPerCall);
  if (params->shading != SRH_SHADING_TORCH)
    return fail(SRH_E_TYPE, "srh_render_views_bwd_camera: camera, normal and pos gradients exist only under SRH_SHADING_TORCH");
  bool want = false;
  for (int v = 0; camera_grads && v < n_views; ++v)
    want = want || camera_grads[v].eye || camera_grads[v].at || camera_grads[v].up;
  if (want) {
    const int32_t width = cameras[0].viewport[2] - cameras[0].viewport[0], rows = params->row1 - params->row0;
    if (width < 1 || rows < 1) return fail(SRH_E_RANGE, "empty frame %d x %d", width, rows);
    const size_t need = camera_head_bytes(n_views) + (size_t)n_views * camera_scratch_bytes(width, rows);
    if (!camera_scratch || camera_scratch_size < need || ((uintptr_t)camera_scratch % sizeof(double)) != 0)
      return fail(SRH_E_WORKSPACE, "camera scratch: %d views need %zu bytes, 8-byte aligned (got %zu at %p)", n_views,
                  need, camera_scratch_size, camera_scratch);
  }
  return render_views_bwd("srh_render_views_bwd_camera", n_views, cameras, objects, lights, materials, params, workspace,
                          workspace_bytes, grad_images, grad_depths, grad_normals, grad_poses, nearests, depths, grads,
                          want ? camera_grads : nullptr, want ? camera_scratch : nullptr, stream);
}

int srh_bin_counters(const SrhObjects* objects, int32_t width, int32_t height, int32_t row0, int32_t row1,
                     size_t* offset_bytes, int32_t* tiles_x, int32_t* tiles_y, int32_t* ntiles_pad, int32_t* bin_cap) {
  if (!offset_bytes || !tiles_x || !tiles_y || !ntiles_pad || !bin_cap) return fail(SRH_E_NULL, "an output pointer is NULL");
  if (!srh_workspace_bytes(objects, width, height)) return SRH_E_RANGE;         // validates, leaves the message
  if (row0 < 0 || row1 > height || row0 >= row1) return fail(SRH_E_RANGE, "row range [%d,%d) outside the %d image rows", row0, row1, height);
  const WsLayout L = layout_for(objects, width, height);
  FrameDev F;
  memset(&F, 0, sizeof(F));
  F.W = width; F.H = height; F.row0 = row0; F.row1 = row1; F.nseg = objects->n_segments;
  (void)setup_binning(F, L, nullptr);                        // pointers relative to NULL: only the tile arithmetic is used
  *offset_bytes = L.counters;
  *tiles_x = F.tiles_x; *tiles_y = F.tiles_y; *ntiles_pad = F.ntiles_pad; *bin_cap = F.bin_cap;
  return SRH_OK;
}

int srh_camera_ray_flags(const SrhCamera* camera, int32_t orthonormal, int32_t* flags) {
  if (!flags) return fail(SRH_E_NULL, "flags is NULL");
  FrameDev F;
  memset(&F, 0, sizeof(F));
  const int rc = camera_to_frame(camera, &F, orthonormal != 0);
  if (rc) return rc;
  *flags = F.div_shared;
  return SRH_OK;
}

int srh_event_create(void** event) {
  if (!event) return fail(SRH_E_NULL, "event is NULL");
  hipEvent_t ev;
  hipError_t e = hipEventCreate(&ev);
  if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
  *event = (void*)ev;
  return SRH_OK;
}

int srh_event_destroy(void* event) {
  if (!event) return SRH_OK;
  hipError_t e = hipEventDestroy((hipEvent_t)event);
  return e == hipSuccess ? SRH_OK : hip_fail(e, "hipEventDestroy");
}

int srh_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return fail(SRH_E_NULL, "event / ms is NULL");
  hipError_t e = hipEventSynchronize((hipEvent_t)stop);
  if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
  e = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
  return e == hipSuccess ? SRH_OK : hip_fail(e, "hipEventElapsedTime");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// The fused layers.  One section per layer: its argument checks and workspace sizes (no HIP call), then its entry
// points.  What the checks share (check_not_null, check_batch_grid, check_scratch, frame_size, pixel_scales,
// check_pinhole) is at the head of this file.
// ------------------------------------------------------------------------------------------------

// ---- the splat renderer (srh_splat.h) ----------------------------------------------------------------------------
namespace {

constexpr int kSplatMaxSamples = 8;
// argument checks (no HIP call) and the device view of a splat launch
int splat_setup(const SrhSplatParams* p, const SrhSplatInputs* in, const SrhLights* lights, const SrhMaterials* mats,
                SplatDev* S) {
  if (!p || !in) return fail(SRH_E_NULL, "params / inputs is NULL");
  if (int rc = check_batch_grid(p->n_views, p->width, p->height, "grid")) return rc;
  if (p->samples < 1 || p->samples > kSplatMaxSamples)
    return fail(SRH_E_RANGE, "samples = %d, expected 1..%d", p->samples, kSplatMaxSamples);
  if (p->pos_cols != 1 && p->pos_cols != 3) return fail(SRH_E_RANGE, "pos_cols = %d, expected 1 or 3", p->pos_cols);
  if (!(p->focal_length > 0.0) || !(p->fovy > 0.0) || !(p->fovy < M_PI))
    return fail(SRH_E_RANGE, "focal_length must be > 0 and fovy in (0, pi)");
  if (!in->pos || !in->eye) return fail(SRH_E_NULL, "inputs.pos / inputs.eye is NULL");
  if (!in->normal && (p->width < 2 || p->height < 2))
    return fail(SRH_E_RANGE, "normal estimation needs a grid of at least 2 x 2 (got %d x %d)", p->width, p->height);
  if (in->pos_view_stride < 0 || in->normal_view_stride < 0 || in->light_vis_view_stride < 0 ||
      in->eye_view_stride < 0 || in->lights_pos_view_stride < 0)
    return fail(SRH_E_RANGE, "negative view stride");
  if (!lights || !mats) return fail(SRH_E_NULL, "lights / materials is NULL");
  if (p->shade)
    if (int rc = check_lights_materials(lights, mats)) return rc;
  const double up2 = p->up[0] * p->up[0] + p->up[1] * p->up[1] + p->up[2] * p->up[2];
  if (!(up2 > 0.0)) return fail(SRH_E_CAMERA, "camera.up is zero");
  memset(S, 0, sizeof(*S));
  S->B = p->n_views; S->W = p->width; S->H = p->height; S->K = p->samples; S->N = p->width * p->height;
  S->pos_cols = p->pos_cols; S->use_quartic = p->use_quartic != 0; S->shade = p->shade != 0;
  S->estimate = in->normal == nullptr;
  S->nlights = p->shade ? lights->n_lights : 0;
  S->ncolors = lights->n_colors; S->nmat = mats->n_materials;
  const FrameSize fs = frame_size(p->fovy, p->focal_length, p->width, p->height);
  S->f = p->focal_length; S->half_w = fs.w / 2; S->half_h = fs.h / 2;
  S->step_x = p->width > 1 ? 2.0 / (p->width - 1) : 0.0;
  S->step_y = p->height > 1 ? -2.0 / (p->height - 1) : 0.0;
  S->sub_dx = p->samples > 1 ? fs.w / (p->samples * p->width - 1) : 0.0;
  S->sub_dy = p->samples > 1 ? fs.h / (p->samples * p->height - 1) : 0.0;
  S->sub_step = p->samples > 1 ? 2.0 / (p->samples - 1) : 0.0;
  const double ui = 1.0 / eps_len(p->up);
  for (int k = 0; k < 3; ++k) { S->at[k] = p->at[k]; S->up[k] = p->up[k] * ui; }
  S->pos = in->pos; S->pos_vs = in->pos_view_stride;
  S->normal = in->normal; S->nrm_vs = in->normal_view_stride;
  S->vis = in->light_vis; S->vis_vs = in->light_vis_view_stride;
  S->eye = in->eye; S->eye_vs = in->eye_view_stride;
  S->lpos = lights->pos; S->lpos_vs = in->lights_pos_view_stride;
  S->lcidx = lights->color_idx; S->colors = lights->colors; S->latt = lights->attenuation; S->amb = lights->ambient;
  S->mat = in->material_idx; S->albedo = mats->albedo; S->coeffs = mats->coeffs;
  return SRH_OK;
}

size_t splat_ws_bytes(const SplatDev& S) { return S.estimate ? (size_t)S.B * S.N * 9 * sizeof(double) : 0; }

// the host side of srh_view_grad.h, defined below with the lift and the warps
size_t view_ws_bytes(int B, int nblk);
int check_grad_view(const char* name, const double* g);
void launch_view_finish(int B, int nblk, int K, int first, const void* part, double* grad_view, hipStream_t st);
static_assert(kViewBlock == 256, "view_block_reduce's workgroup is the splat kernels'");

// srh_splat_bwd (grad_view = NULL) and srh_splat_bwd_view
int splat_bwd_any(const SrhSplatParams* params, const SrhSplatInputs* inputs, const SrhLights* lights,
                  const SrhMaterials* materials, void* workspace, size_t workspace_bytes, const float* grad_image,
                  const float* grad_depth, const float* grad_pos, const float* grad_normal, const SrhSplatGrads* grads,
                  bool with_view, double* grad_view, void* view_workspace, size_t view_workspace_bytes, void* stream) {
  SplatDev S;
  int rc = splat_setup(params, inputs, lights, materials, &S);
  if (rc) return rc;
  if (!grads) return fail(SRH_E_NULL, "grads is NULL");
  if (!grad_image && !grad_depth && !grad_pos && !grad_normal)
    return fail(SRH_E_NULL, "grad_image, grad_depth, grad_pos and grad_normal are all NULL");
  if (!S.shade && (grad_image || grads->light_vis || grads->lights_pos || grads->colors || grads->attenuation ||
                   grads->ambient || grads->albedo || grads->coeffs))
    return fail(SRH_E_TYPE, "a geometry-only frame (shade = 0) has no image, light_vis or shading gradients");
  if (!S.shade && with_view)
    return fail(SRH_E_TYPE, "a geometry-only frame (shade = 0) does not depend on the camera: no grad_view");
  if (grads->light_vis && !S.vis) return fail(SRH_E_NULL, "grads.light_vis without inputs.light_vis");
  if (grads->normal && !S.normal) return fail(SRH_E_NULL, "grads.normal without inputs.normal (estimated normals)");
  const bool gather = S.estimate && grads->pos;
  if (gather && (rc = check_scratch("workspace", workspace, workspace_bytes, splat_ws_bytes(S)))) return rc;
  const dim3 grid((S.N + 255) / 256, S.B);
  if (with_view) {
    if ((rc = check_grad_view("grad_view", grad_view))) return rc;
    if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, view_ws_bytes(S.B, grid.x)))) return rc;
  }
  SplatGradsDev G;
  G.pos = grads->pos; G.normal = grads->normal; G.vis = grads->light_vis; G.lpos = grads->lights_pos;
  G.colors = grads->colors; G.latt = grads->attenuation; G.amb = grads->ambient; G.albedo = grads->albedo;
  G.coeffs = grads->coeffs;
  if (S.estimate && !gather) {
    G.pos = nullptr;
    if (!with_view && !G.vis && !G.lpos && !G.colors && !G.latt && !G.amb && !G.albedo && !G.coeffs) return SRH_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  // without z gradients the stencil slots are not wanted: k_splat_bwd then needs no workspace
  double* ws = gather ? (double*)workspace : nullptr;
  if (with_view) {
    hipLaunchKernelGGL(k_splat_bwd<true>, grid, dim3(256), 0, st, S, G, grad_image, grad_depth, grad_pos, grad_normal, ws,
                       (double*)view_workspace);
    launch_view_finish(S.B, grid.x, kViewSums, 0, view_workspace, grad_view, st);
  } else {
    hipLaunchKernelGGL(k_splat_bwd<false>, grid, dim3(256), 0, st, S, G, grad_image, grad_depth, grad_pos, grad_normal,
                       ws, (double*)nullptr);
  }
  if (gather) hipLaunchKernelGGL(k_splat_gather, grid, dim3(256), 0, st, S, grads->pos, (const double*)ws);
  return launch_status(with_view ? "splat backward (view) launch" : "splat backward launch");
}

}  // namespace

extern "C" {

size_t srh_splat_workspace_bytes(const SrhSplatParams* params, const SrhSplatInputs* inputs) {
  SrhLights L;
  SrhMaterials M;
  memset(&L, 0, sizeof(L));
  memset(&M, 0, sizeof(M));
  SrhSplatParams p;
  if (!params) { fail(SRH_E_NULL, "params is NULL"); return 0; }
  p = *params;
  p.shade = 0;                                           // the size does not depend on the lights
  SplatDev S;
  if (splat_setup(&p, inputs, &L, &M, &S)) return 0;
  return splat_ws_bytes(S);
}

int srh_splat_fwd(const SrhSplatParams* params, const SrhSplatInputs* inputs, const SrhLights* lights,
                  const SrhMaterials* materials, float* image, float* depth, float* pos, float* normal, void* stream) {
  SplatDev S;
  int rc = splat_setup(params, inputs, lights, materials, &S);
  if (rc) return rc;
  if (!depth || !pos || !normal || (S.shade && !image)) return fail(SRH_E_NULL, "an output buffer is NULL");
  const dim3 grid((S.N + 255) / 256, S.B);
  hipLaunchKernelGGL(k_splat_fwd, grid, dim3(256), 0, (hipStream_t)stream, S, image, depth, pos, normal);
  return launch_status("k_splat_fwd launch");
}

int srh_splat_bwd(const SrhSplatParams* params, const SrhSplatInputs* inputs, const SrhLights* lights,
                  const SrhMaterials* materials, void* workspace, size_t workspace_bytes,
                  const float* grad_image, const float* grad_depth, const float* grad_pos, const float* grad_normal,
                  const SrhSplatGrads* grads, void* stream) {
  return splat_bwd_any(params, inputs, lights, materials, workspace, workspace_bytes, grad_image, grad_depth, grad_pos,
                       grad_normal, grads, false, nullptr, nullptr, 0, stream);
}

int srh_splat_bwd_view(const SrhSplatParams* params, const SrhSplatInputs* inputs, const SrhLights* lights,
                       const SrhMaterials* materials, void* workspace, size_t workspace_bytes, const float* grad_image,
                       const float* grad_depth, const float* grad_pos, const float* grad_normal,
                       const SrhSplatGrads* grads, double* grad_view, void* view_workspace,
                       size_t view_workspace_bytes, void* stream) {
  return splat_bwd_any(params, inputs, lights, materials, workspace, workspace_bytes, grad_image, grad_depth, grad_pos,
                       grad_normal, grads, true, grad_view, view_workspace, view_workspace_bytes, stream);
}

}  // extern "C"

// ---- the NDC splat renderer (srh_splat_ndc.h) --------------------------------------------------------------------
namespace {

// argument checks (no HIP call) and the device view of an NDC splat launch
int splat_ndc_setup(const SrhSplatNdcParams* p, const SrhSplatNdcInputs* in, const SrhLights* lights,
                    const SrhMaterials* mats, SplatNdcDev* D) {
  if (!p || !in) return fail(SRH_E_NULL, "params / inputs is NULL");
  if (int rc = check_batch_grid(p->n_views, p->width, p->height, "grid")) return rc;
  if (p->pos_cols != 3 && p->pos_cols != 4) return fail(SRH_E_RANGE, "pos_cols = %d, expected 3 or 4", p->pos_cols);
  if (!(p->fovy > 0.0) || !(p->fovy < M_PI)) return fail(SRH_E_RANGE, "fovy = %g, expected a value in (0, pi)", p->fovy);
  if (!(p->near_clip > 0.0) || !(p->near_clip < p->far_clip) || !(p->far_clip < HUGE_VAL))
    return fail(SRH_E_RANGE, "near_clip = %g, far_clip = %g, expected 0 < near_clip < far_clip", p->near_clip, p->far_clip);
  if (!in->pos || !in->eye) return fail(SRH_E_NULL, "inputs.pos / inputs.eye is NULL");
  if (p->shade && !in->normal) return fail(SRH_E_NULL, "inputs.normal is NULL");
  if (in->pos_view_stride < 0 || in->normal_view_stride < 0 || in->eye_view_stride < 0 || in->lights_pos_view_stride < 0)
    return fail(SRH_E_RANGE, "negative view stride");
  if (!lights || !mats) return fail(SRH_E_NULL, "lights / materials is NULL");
  if (p->shade) {
    if (lights->n_lights < 1 || lights->n_lights > SRH_MAX_LIGHTS)
      return fail(SRH_E_RANGE, "n_lights = %d, expected 1..%d", lights->n_lights, SRH_MAX_LIGHTS);
    if (int rc = check_lights_materials(lights, mats)) return rc;
  }
  const double up2 = p->up[0] * p->up[0] + p->up[1] * p->up[1] + p->up[2] * p->up[2];
  if (!(up2 > 0.0)) return fail(SRH_E_CAMERA, "degenerate camera: camera.up is zero");
  memset(D, 0, sizeof(*D));
  SplatDev* S = &D->S;
  S->B = p->n_views; S->W = p->width; S->H = p->height; S->K = 1; S->N = p->width * p->height;
  S->pos_cols = p->pos_cols; S->use_quartic = p->use_quartic != 0; S->shade = p->shade != 0;
  S->nlights = p->shade ? lights->n_lights : 0;
  S->ncolors = lights->n_colors; S->nmat = mats->n_materials;
  const double ui = 1.0 / eps_len(p->up);
  for (int k = 0; k < 3; ++k) { S->at[k] = p->at[k]; S->up[k] = p->up[k] * ui; }
  S->pos = in->pos; S->pos_vs = in->pos_view_stride;
  S->normal = in->normal; S->nrm_vs = in->normal_view_stride;
  S->eye = in->eye; S->eye_vs = in->eye_view_stride;
  S->lpos = lights->pos; S->lpos_vs = in->lights_pos_view_stride;
  S->lcidx = lights->color_idx; S->colors = lights->colors; S->latt = lights->attenuation; S->amb = lights->ambient;
  S->mat = in->material_idx; S->albedo = mats->albedo; S->coeffs = mats->coeffs;
  D->double_sided = p->double_sided != 0;
  // perspective_NO_params (diffrend/torch/ops.py:6-20) with the reference's true division for the aspect
  const double aspect = (double)p->width / (double)p->height, t = tan(p->fovy / 2.0);
  D->m00 = 1.0 / (aspect * t);
  D->m11 = 1.0 / t;
  D->m22 = (p->near_clip + p->far_clip) / (p->far_clip - p->near_clip);
  D->m23 = -2.0 * p->near_clip * p->far_clip / (p->far_clip - p->near_clip);
  return SRH_OK;
}

// srh_splat_ndc_bwd (grad_view = NULL) and srh_splat_ndc_bwd_view
int splat_ndc_bwd_any(const SrhSplatNdcParams* params, const SrhSplatNdcInputs* inputs, const SrhLights* lights,
                      const SrhMaterials* materials, const float* grad_image, const float* grad_depth,
                      const float* grad_pos, const SrhSplatNdcGrads* grads, bool with_view, double* grad_view,
                      void* view_workspace, size_t view_workspace_bytes, void* stream) {
  SplatNdcDev D;
  int rc = splat_ndc_setup(params, inputs, lights, materials, &D);
  if (rc) return rc;
  if (!grads) return fail(SRH_E_NULL, "grads is NULL");
  if (!grad_image && !grad_depth && !grad_pos)
    return fail(SRH_E_NULL, "grad_image, grad_depth and grad_pos are all NULL");
  if (!with_view && !grads->pos && !grads->normal && !grads->lights_pos && !grads->colors && !grads->attenuation &&
      !grads->ambient && !grads->albedo && !grads->coeffs)
    return fail(SRH_E_NULL, "the gradient buffers of grads are all NULL");
  if (!D.S.shade && (grad_image || grads->lights_pos || grads->colors || grads->attenuation || grads->ambient ||
                     grads->albedo || grads->coeffs))
    return fail(SRH_E_TYPE, "a geometry-only frame (shade = 0) has no image or shading gradients");
  if (!D.S.shade && with_view)
    return fail(SRH_E_TYPE, "a geometry-only frame (shade = 0) does not depend on the camera: no grad_view");
  const dim3 grid((D.S.N + 255) / 256, D.S.B);
  if (with_view) {
    if ((rc = check_grad_view("grad_view", grad_view))) return rc;
    if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, view_ws_bytes(D.S.B, grid.x))))
      return rc;
  }
  SplatGradsDev G;
  memset(&G, 0, sizeof(G));
  G.pos = grads->pos; G.normal = grads->normal; G.lpos = grads->lights_pos; G.colors = grads->colors;
  G.latt = grads->attenuation; G.amb = grads->ambient; G.albedo = grads->albedo; G.coeffs = grads->coeffs;
  hipStream_t st = (hipStream_t)stream;
  if (with_view) {
    hipLaunchKernelGGL(k_splat_ndc_bwd<true>, grid, dim3(256), 0, st, D, G, grad_image, grad_depth, grad_pos,
                       (double*)view_workspace);
    launch_view_finish(D.S.B, grid.x, kViewSums, 0, view_workspace, grad_view, st);
    return launch_status("splat NDC backward (view) launch");
  }
  hipLaunchKernelGGL(k_splat_ndc_bwd<false>, grid, dim3(256), 0, st, D, G, grad_image, grad_depth, grad_pos,
                     (double*)nullptr);
  return launch_status("k_splat_ndc_bwd launch");
}

}  // namespace

extern "C" {

int srh_splat_ndc_fwd(const SrhSplatNdcParams* params, const SrhSplatNdcInputs* inputs, const SrhLights* lights,
                      const SrhMaterials* materials, float* image, float* depth, float* pos, void* stream) {
  SplatNdcDev D;
  int rc = splat_ndc_setup(params, inputs, lights, materials, &D);
  if (rc) return rc;
  if (!depth || !pos || (D.S.shade && !image)) return fail(SRH_E_NULL, "an output buffer is NULL");
  const dim3 grid((D.S.N + 255) / 256, D.S.B);
  hipLaunchKernelGGL(k_splat_ndc_fwd, grid, dim3(256), 0, (hipStream_t)stream, D, image, depth, pos);
  return launch_status("k_splat_ndc_fwd launch");
}

int srh_splat_ndc_bwd(const SrhSplatNdcParams* params, const SrhSplatNdcInputs* inputs, const SrhLights* lights,
                      const SrhMaterials* materials, const float* grad_image, const float* grad_depth,
                      const float* grad_pos, const SrhSplatNdcGrads* grads, void* stream) {
  return splat_ndc_bwd_any(params, inputs, lights, materials, grad_image, grad_depth, grad_pos, grads, false, nullptr,
                           nullptr, 0, stream);
}

int srh_splat_ndc_bwd_view(const SrhSplatNdcParams* params, const SrhSplatNdcInputs* inputs, const SrhLights* lights,
                           const SrhMaterials* materials, const float* grad_image, const float* grad_depth,
                           const float* grad_pos, const SrhSplatNdcGrads* grads, double* grad_view,
                           void* view_workspace, size_t view_workspace_bytes, void* stream) {
  return splat_ndc_bwd_any(params, inputs, lights, materials, grad_image, grad_depth, grad_pos, grads, true, grad_view,
                           view_workspace, view_workspace_bytes, stream);
}

}  // extern "C"

// ---- the splat regularisers (srh_regularizers.h) -----------------------------------------------------------------
namespace {

// the stencil's own refusal sits before the size test: a grid that fails both is refused with it
int reg_check_grid(int32_t n_views, int32_t width, int32_t height) {
  if (int rc = check_n_views(n_views)) return rc;
  if (width < 2 || height < 2)
    return fail(SRH_E_RANGE, "grid %d x %d: the reflected stencil needs at least 2 x 2", width, height);
  return check_grid_size(width, height, "grid");
}

size_t reg_ws_bytes(int32_t n_views, int32_t width, int32_t height) {
  const size_t nblk = ((size_t)width * height + kRegBlock - 1) / kRegBlock;
  return (size_t)n_views * nblk * kRegSums * sizeof(double);
}

// argument checks (no HIP call) and the device view of a regulariser launch
int reg_setup(const SrhRegularizerParams* p, const float* pos, const float* normal, const float* image,
              const float* depth, RegDev* R) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = reg_check_grid(p->n_views, p->width, p->height)) return rc;
  if (!(p->z_min <= p->z_max)) return fail(SRH_E_RANGE, "z_min = %g > z_max = %g", p->z_min, p->z_max);
  if (!pos || !normal || !image || !depth) return fail(SRH_E_NULL, "pos / normal / image / depth is NULL");
  R->B = p->n_views; R->W = p->width; R->H = p->height; R->N = p->width * p->height;
  R->nblk = (R->N + kRegBlock - 1) / kRegBlock;
  R->z_min = p->z_min; R->z_max = p->z_max; R->z_scale = p->z_scale; R->n_scale = p->unit_normal_scale;
  R->pos = pos; R->normal = normal; R->image = image; R->depth = depth;
  return SRH_OK;
}

}  // namespace

extern "C" {

size_t srh_regularizers_workspace_bytes(int32_t n_views, int32_t width, int32_t height) {
  if (reg_check_grid(n_views, width, height)) return 0;
  return reg_ws_bytes(n_views, width, height);
}

int srh_regularizers_fwd(const SrhRegularizerParams* params, const float* pos, const float* normal, const float* image,
                         const float* depth, void* workspace, size_t workspace_bytes, float* terms, double* stats,
                         void* stream) {
  RegDev R;
  int rc = reg_setup(params, pos, normal, image, depth, &R);
  if (rc) return rc;
  if (!terms || !stats) return fail(SRH_E_NULL, "terms / stats is NULL");
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, reg_ws_bytes(R.B, R.W, R.H)))) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_reg_fwd, dim3(R.nblk, R.B), dim3(kRegBlock), 0, st, R, (double*)workspace);
  hipLaunchKernelGGL(k_reg_finish, dim3(R.B), dim3(64), 0, st, R, (const double*)workspace, terms, stats);
  return launch_status("regularizers forward launch");
}

int srh_regularizers_bwd(const SrhRegularizerParams* params, const float* pos, const float* normal, const float* image,
                         const float* depth, const double* stats, const float* grad_terms, float* g_pos,
                         float* g_normal, float* g_image, float* g_depth, void* stream) {
  RegDev R;
  int rc = reg_setup(params, pos, normal, image, depth, &R);
  if (rc) return rc;
  if (!stats || !grad_terms) return fail(SRH_E_NULL, "stats / grad_terms is NULL");
  if (!g_pos && !g_normal && !g_image && !g_depth)
    return fail(SRH_E_NULL, "g_pos, g_normal, g_image and g_depth are all NULL");
  RegGradsDev G;
  G.pos = g_pos; G.normal = g_normal; G.image = g_image; G.depth = g_depth;
  hipLaunchKernelGGL(k_reg_bwd, dim3(R.nblk, R.B), dim3(kRegBlock), 0, (hipStream_t)stream, R, G, stats, grad_terms);
  return launch_status("k_reg_bwd launch");
}

}  // extern "C"

// ---- the surfel re-projection layer (srh_projection.h) -----------------------------------------------------------
namespace {

static_assert(kProjMaxD == SRH_PROJ_MAX_CHANNELS && kProjMaxHalf == SRH_PROJ_MAX_BLUR_HALF, "srh.h and srh_projection.h");
static_assert(kProjUseDepth == SRH_PROJ_USE_DEPTH && kProjUseCenterDist == SRH_PROJ_USE_CENTER_DIST &&
              kProjBlurRotated == SRH_PROJ_BLUR_ROTATED && kProjDetachMask == SRH_PROJ_DETACH_MASK &&
              kProjDetachMask2 == SRH_PROJ_DETACH_MASK2 && kProjDetachDepthMerge == SRH_PROJ_DETACH_DEPTH_MERGE,
              "srh.h and srh_projection.h");

// what the parameters of the three projection layers share: the batch, the frame and the channel count
int check_proj_frame(int32_t n_views, int32_t width, int32_t height, int32_t channels) {
  if (int rc = check_batch_grid(n_views, width, height, "width x height =")) return rc;
  if (channels < 1 || channels > kProjMaxD) return fail(SRH_E_RANGE, "channels = %d, expected 1..%d", channels, kProjMaxD);
  return SRH_OK;
}

// A layer's workspace as consecutive regions: each *_ws function below is the one statement of a layout, and both the
// size the caller must bring (`bytes`, from no base) and the entry points' pointers come from it.
struct Regions {
  char* base;
  size_t bytes = 0;
  template <class T>
  T* take(size_t count) {
    T* at = base ? (T*)(base + bytes) : nullptr;
    bytes += count * sizeof(T);
    return at;
  }
};

// ---- the camera gradient of the lift and the two warps (srh_view_grad.h): what the *_bwd_view entry points share ----
static_assert(kViewBlock == kProjBlock && kViewBlock == kSurfBlock, "view_block_reduce's workgroup is the layers'");
static_assert(kRProjView2First + kRProjView2Sums == kViewSums, "row 2 of the 3 x 4 matrix");

// the partials of one kView launch: 12 fp64 sums per workgroup (a launch that brings fewer uses the head)
size_t view_ws_bytes(int B, int nblk) { return (size_t)B * nblk * kViewSums * sizeof(double); }

int check_grad_view(const char* name, const double* g) {
  if (!g) return fail(SRH_E_NULL, "%s is NULL", name);
  if ((uintptr_t)g % sizeof(double)) return fail(SRH_E_WORKSPACE, "%s: %p is not 8-byte aligned", name, (const void*)g);
  return SRH_OK;
}

// the K sums per workgroup a kView kernel left in `part` -> entries [first, first + K) of grad_view (B, 12), 0 elsewhere
void launch_view_finish(int B, int nblk, int K, int first, const void* part, double* grad_view, hipStream_t st) {
  hipLaunchKernelGGL(k_view_finish, dim3(1, B), dim3(kViewRows * kViewSums), 0, st, nblk, K, first, (const double*)part,
                     grad_view);
}

// argument checks (no HIP call) and the device view of a projection launch
int proj_setup(const SrhProjectionParams* p, bool has_rotated, ProjDev* P) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_proj_frame(p->n_views, p->width, p->height, p->channels)) return rc;
  if (p->flags & ~63) return fail(SRH_E_TYPE, "flags = %d has unknown bits", p->flags);
  if (p->blur_half < 0 || p->blur_half > kProjMaxHalf)
    return fail(SRH_E_RANGE, "blur_half = %d, expected 0..%d", p->blur_half, kProjMaxHalf);
  if (int rc = check_pinhole("", p->fovy, p->focal_length)) return rc;
  for (int k = 0; k <= p->blur_half; ++k)
    if (!std::isfinite(p->taps[k])) return fail(SRH_E_RANGE, "taps[%d] is not finite", k);
  memset(P, 0, sizeof(*P));
  P->B = p->n_views; P->W = p->width; P->H = p->height; P->N = p->width * p->height; P->D = p->channels;
  P->P = 2 * P->D + 2; P->CS = P->D + 3; P->half = p->blur_half;
  P->flags = p->flags | (has_rotated ? kProjHasRotated : 0);
  P->ncell = (P->W + 1) * (P->H + 1);
  P->nblk = (P->N + kProjBlock - 1) / kProjBlock;
  const PixelScales s = pixel_scales(p->fovy, p->focal_length, P->W, P->H);
  P->fsx = s.fsx; P->fsy = s.fsy; P->cx0 = s.cx0; P->cy0 = s.cy0;
  for (int k = 0; k <= P->half; ++k) P->taps[k] = p->taps[k];
  return SRH_OK;
}

// SRH_PROJ_WS_FWD: rec (B, N, 4) | pre (B, P, N) | tmp (B, P, N) fp64 | range (B, ncell, 2) int32
// SRH_PROJ_WS_SAVED: blr (B, P, N) | cor (B, 4, CS, N) fp64
// SRH_PROJ_WS_BWD: gpl (B, P, N) | gtmp (B, P, N) | gcor (B, 4, CS, N) fp64
struct ProjWs {
  double *rec, *pre, *tmp, *blr, *cor, *gpl, *gtmp, *gcor;
  int32_t* range;
  size_t bytes;
};
ProjWs proj_ws(const ProjDev& P, int which, const void* base = nullptr) {
  const size_t px = (size_t)P.B * P.N;
  Regions r{(char*)base};
  ProjWs w = {};
  switch (which) {
    case SRH_PROJ_WS_FWD:
      w.rec = r.take<double>(px * 4);
      w.pre = r.take<double>(px * P.P);
      w.tmp = r.take<double>(px * P.P);
      w.range = r.take<int32_t>((size_t)P.B * P.ncell * 2);
      break;
    case SRH_PROJ_WS_SAVED:
      w.blr = r.take<double>(px * P.P);
      w.cor = r.take<double>(px * 4 * P.CS);
      break;
    default:
      w.gpl = r.take<double>(px * P.P);
      w.gtmp = r.take<double>(px * P.P);
      w.gcor = r.take<double>(px * 4 * P.CS);
  }
  w.bytes = r.bytes;
  return w;
}
size_t proj_ws_bytes(const ProjDev& P, int which) { return proj_ws(P, which).bytes; }

}  // namespace

extern "C" {

size_t srh_projection_workspace_bytes(const SrhProjectionParams* params, int32_t which) {
  ProjDev P;
  if (proj_setup(params, false, &P)) return 0;
  if (which < SRH_PROJ_WS_FWD || which > SRH_PROJ_WS_BWD) {
    fail(SRH_E_TYPE, "which = %d, expected SRH_PROJ_WS_FWD, _SAVED or _BWD", which);
    return 0;
  }
  return proj_ws_bytes(P, which);
}

int srh_projection_keys(const SrhProjectionParams* params, const double* view, const float* surfels, void* workspace,
                        size_t workspace_bytes, int32_t* keys, void* stream) {
  ProjDev P;
  int rc = proj_setup(params, false, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"view", view}, {"surfels", surfels}, {"keys", keys}}))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, proj_ws_bytes(P, SRH_PROJ_WS_FWD)))) return rc;
  hipLaunchKernelGGL(k_proj_keys, dim3(P.nblk, P.B), dim3(kProjBlock), 0, (hipStream_t)stream, P, view, surfels,
                     proj_ws(P, SRH_PROJ_WS_FWD, workspace).rec, keys);
  return launch_status("k_proj_keys launch");
}

int srh_projection_fwd(const SrhProjectionParams* params, const float* rgb, const float* rotated, const int32_t* keys,
                       const int32_t* order, void* workspace, size_t workspace_bytes, void* saved, size_t saved_bytes,
                       float* out, float* mask, float* image1, float* depth, void* stream) {
  ProjDev P;
  int rc = proj_setup(params, rotated != nullptr, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"rgb", rgb}, {"keys", keys}, {"order", order}}))) return rc;
  if (!out || !mask || !image1) return fail(SRH_E_NULL, "out / mask / image1 is NULL");
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, proj_ws_bytes(P, SRH_PROJ_WS_FWD)))) return rc;
  if (saved && (rc = check_scratch("saved", saved, saved_bytes, proj_ws_bytes(P, SRH_PROJ_WS_SAVED)))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const ProjWs w = proj_ws(P, SRH_PROJ_WS_FWD, workspace), s = proj_ws(P, SRH_PROJ_WS_SAVED, saved);
  const int nb = (rotated && (P.flags & kProjBlurRotated)) ? 2 * P.D + 1 : P.D + 1;
  const dim3 grid(P.nblk, P.B), block(kProjBlock);
  if (hipError_t e = hipMemsetAsync(w.range, 0, (size_t)P.B * P.ncell * 2 * sizeof(int32_t), st))
    return hip_fail(e, "projection cell ranges memset");
  hipLaunchKernelGGL(k_proj_mark, grid, block, 0, st, P, keys, order, w.range);
  hipLaunchKernelGGL(k_proj_gather, grid, block, 0, st, P, (const double*)w.rec, order, (const int32_t*)w.range, rgb,
                     rotated, w.pre, s.cor);
  hipLaunchKernelGGL(k_proj_blur_h, dim3((P.N * nb + kProjBlock - 1) / kProjBlock, P.B), block, 0, st, P, nb,
                     (const double*)w.pre, w.tmp);
  hipLaunchKernelGGL(k_proj_blur_v_merge, grid, block, 0, st, P, nb, (const double*)w.tmp, (const double*)w.pre, rotated,
                     s.blr, out, mask, image1, depth);
  return launch_status("projection forward launch");
}

// srh_projection_bwd, and with `with_view` srh_projection_bwd_view
static int projection_bwd(bool with_view, const SrhProjectionParams* params, const double* view, const float* surfels,
                          const float* rgb, const float* rotated, const void* saved, size_t saved_bytes, void* workspace,
                          size_t workspace_bytes, const float* g_out, const float* g_mask, const float* g_image1,
                          const float* g_depth, float* grad_surfels, float* grad_rgb, float* grad_rotated,
                          double* grad_view, void* view_workspace, size_t view_workspace_bytes, void* stream) {
  ProjDev P;
  int rc = proj_setup(params, rotated != nullptr, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"view", view}, {"surfels", surfels}, {"rgb", rgb}}))) return rc;
  if (!g_out && !g_mask && !g_image1 && !g_depth)
    return fail(SRH_E_NULL, "g_out, g_mask, g_image1 and g_depth are all NULL");
  if (!with_view && !grad_surfels && !grad_rgb && !grad_rotated)
    return fail(SRH_E_NULL, "grad_surfels, grad_rgb and grad_rotated are all NULL");
  if (grad_rotated && !rotated) return fail(SRH_E_NULL, "grad_rotated without rotated");
  if ((rc = check_scratch("saved", saved, saved_bytes, proj_ws_bytes(P, SRH_PROJ_WS_SAVED)))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, proj_ws_bytes(P, SRH_PROJ_WS_BWD)))) return rc;
  if (with_view) {
    if ((rc = check_grad_view("grad_view", grad_view))) return rc;
    if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, view_ws_bytes(P.B, P.nblk))))
      return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  const ProjWs s = proj_ws(P, SRH_PROJ_WS_SAVED, saved), w = proj_ws(P, SRH_PROJ_WS_BWD, workspace);
  double* gcor = (with_view || grad_surfels || grad_rgb) ? w.gcor : nullptr;
  const int nb = (grad_rotated && (P.flags & kProjBlurRotated)) ? 2 * P.D + 1 : P.D + 1;
  const dim3 grid(P.nblk, P.B), block(kProjBlock);
  hipLaunchKernelGGL(k_proj_merge_bwd, grid, block, 0, st, P, (const double*)s.blr, g_out, g_mask, g_image1, g_depth,
                     w.gpl);
  hipLaunchKernelGGL(k_proj_blur_h, dim3((P.N * nb + kProjBlock - 1) / kProjBlock, P.B), block, 0, st, P, nb,
                     (const double*)w.gpl, w.gtmp);
  hipLaunchKernelGGL(k_proj_blur_v_corner, grid, block, 0, st, P, nb, (const double*)w.gtmp, (const double*)w.gpl,
                     (const double*)s.cor, gcor, grad_rotated);
  if (with_view) {
    hipLaunchKernelGGL(k_proj_surfel_bwd<true>, grid, block, 0, st, P, view, surfels, rgb, (const double*)gcor, grad_rgb,
                       grad_surfels, (double*)view_workspace);
    launch_view_finish(P.B, P.nblk, kViewSums, 0, view_workspace, grad_view, st);
  } else if (gcor) {
    hipLaunchKernelGGL(k_proj_surfel_bwd<false>, grid, block, 0, st, P, view, surfels, rgb, (const double*)gcor, grad_rgb,
                       grad_surfels, (double*)nullptr);
  }
  return launch_status("projection backward launch");
}

int srh_projection_bwd(const SrhProjectionParams* params, const double* view, const float* surfels, const float* rgb,
                       const float* rotated, const void* saved, size_t saved_bytes, void* workspace,
                       size_t workspace_bytes, const float* g_out, const float* g_mask, const float* g_image1,
                       const float* g_depth, float* grad_surfels, float* grad_rgb, float* grad_rotated, void* stream) {
  return projection_bwd(false, params, view, surfels, rgb, rotated, saved, saved_bytes, workspace, workspace_bytes, g_out,
                        g_mask, g_image1, g_depth, grad_surfels, grad_rgb, grad_rotated, nullptr, nullptr, 0, stream);
}

int srh_projection_bwd_view(const SrhProjectionParams* params, const double* view, const float* surfels,
                            const float* rgb, const float* rotated, const void* saved, size_t saved_bytes,
                            void* workspace, size_t workspace_bytes, const float* g_out, const float* g_mask,
                            const float* g_image1, const float* g_depth, float* grad_surfels, float* grad_rgb,
                            float* grad_rotated, double* grad_view, void* view_workspace, size_t view_workspace_bytes,
                            void* stream) {
  return projection_bwd(true, params, view, surfels, rgb, rotated, saved, saved_bytes, workspace, workspace_bytes, g_out,
                        g_mask, g_image1, g_depth, grad_surfels, grad_rgb, grad_rotated, grad_view, view_workspace,
                        view_workspace_bytes, stream);
}

}  // extern "C"

// ---- the reverse re-projection layer (srh_reverse_projection.h) --------------------------------------------------
namespace {

// argument checks (no HIP call) and the device view of a reverse projection launch
int rproj_setup(const SrhReverseProjectionParams* p, RProjDev* R) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_proj_frame(p->n_views, p->width, p->height, p->channels)) return rc;
  if (int rc = check_pinhole("1", p->fovy1, p->focal_length1)) return rc;
  if (int rc = check_pinhole("2", p->fovy2, p->focal_length2)) return rc;
  if (!std::isfinite(p->depth_epsilon)) return fail(SRH_E_RANGE, "depth_epsilon = %g, expected finite", p->depth_epsilon);
  memset(R, 0, sizeof(*R));
  R->B = p->n_views; R->W = p->width; R->H = p->height; R->N = p->width * p->height; R->D = p->channels;
  R->ncell = (R->W + 1) * (R->H + 1);
  R->nblk = (R->N + kProjBlock - 1) / kProjBlock;
  const PixelScales s[2] = {pixel_scales(p->fovy1, p->focal_length1, R->W, R->H),
                            pixel_scales(p->fovy2, p->focal_length2, R->W, R->H)};
  for (int c = 0; c < 2; ++c) { R->fsx[c] = s[c].fsx; R->fsy[c] = s[c].fsy; }
  R->cx0 = s[0].cx0;
  R->cy0 = s[0].cy0;
  R->eps = p->depth_epsilon;
  return SRH_OK;
}

// what k_proj_keys and k_proj_mark read of a ProjDev, for camera 1: no weights, so the record is (fx, fy, z, 1)
ProjDev rproj_as_proj(const RProjDev& R) {
  ProjDev P;
  memset(&P, 0, sizeof(P));
  P.B = R.B; P.W = R.W; P.H = R.H; P.N = R.N; P.D = R.D; P.ncell = R.ncell; P.nblk = R.nblk;
  P.fsx = R.fsx[0]; P.fsy = R.fsy[0]; P.cx0 = R.cx0; P.cy0 = R.cy0;
  return P;
}

// SRH_RPROJ_WS_FWD: d_in (B, N) fp64
// SRH_RPROJ_WS_BWD: rec (B, N, 4) | gpl (B, D + 1, N) fp64 | range (B, ncell, 2) int32
// rec is first: srh_reverse_projection_keys writes it through the same workspace
struct RProjWs {
  double *d_in, *rec, *gpl;
  int32_t* range;
  size_t bytes;
};
RProjWs rproj_ws(const RProjDev& R, int which, const void* base = nullptr) {
  const size_t px = (size_t)R.B * R.N;
  Regions r{(char*)base};
  RProjWs w = {};
  if (which == SRH_RPROJ_WS_FWD) {
    w.d_in = r.take<double>(px);
  } else {
    w.rec = r.take<double>(px * 4);
    w.gpl = r.take<double>(px * (R.D + 1));
    w.range = r.take<int32_t>((size_t)R.B * R.ncell * 2);
  }
  w.bytes = r.bytes;
  return w;
}
size_t rproj_ws_bytes(const RProjDev& R, int which) { return rproj_ws(R, which).bytes; }

}  // namespace

extern "C" {

size_t srh_reverse_projection_workspace_bytes(const SrhReverseProjectionParams* params, int32_t which) {
  RProjDev R;
  if (rproj_setup(params, &R)) return 0;
  if (which != SRH_RPROJ_WS_FWD && which != SRH_RPROJ_WS_BWD) {
    fail(SRH_E_TYPE, "which = %d, expected SRH_RPROJ_WS_FWD or _BWD", which);
    return 0;
  }
  return rproj_ws_bytes(R, which);
}

int srh_reverse_projection_fwd(const SrhReverseProjectionParams* params, const double* view1, const double* view2,
                               const float* rgb, const float* in_pos, const float* out_pos, const float* rotated,
                               const float* keep, void* workspace, size_t workspace_bytes, float* out, float* mask,
                               float* image1, float* depth, void* stream) {
  RProjDev R;
  int rc = rproj_setup(params, &R);
  if (rc) return rc;
  if ((rc = check_not_null({{"view1", view1}, {"view2", view2}, {"rgb", rgb}, {"in_pos", in_pos}, {"out_pos", out_pos}})))
    return rc;
  if (rotated && !out) return fail(SRH_E_NULL, "out is NULL with a rotated image");
  if ((rc = check_not_null({{"mask", mask}, {"image1", image1}}))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, rproj_ws_bytes(R, SRH_RPROJ_WS_FWD)))) return rc;
  const dim3 grid(R.nblk, R.B), block(kProjBlock);
  hipStream_t st = (hipStream_t)stream;
  double* d_in = rproj_ws(R, SRH_RPROJ_WS_FWD, workspace).d_in;
  hipLaunchKernelGGL(k_rproj_depth_in, grid, block, 0, st, R, view1, view2, in_pos, out_pos, d_in);
  hipLaunchKernelGGL(k_rproj_fwd, grid, block, 0, st, R, view1, view2, rgb, in_pos, out_pos, rotated, keep,
                     (const double*)d_in, out, mask, image1, depth);
  return launch_status("reverse projection forward launch");
}

int srh_reverse_projection_keys(const SrhReverseProjectionParams* params, const double* view1, const float* out_pos,
                                void* workspace, size_t workspace_bytes, int32_t* keys, void* stream) {
  RProjDev R;
  int rc = rproj_setup(params, &R);
  if (rc) return rc;
  if ((rc = check_not_null({{"view1", view1}, {"out_pos", out_pos}, {"keys", keys}}))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, rproj_ws_bytes(R, SRH_RPROJ_WS_BWD)))) return rc;
  hipLaunchKernelGGL(k_proj_keys, dim3(R.nblk, R.B), dim3(kProjBlock), 0, (hipStream_t)stream, rproj_as_proj(R), view1,
                     out_pos, rproj_ws(R, SRH_RPROJ_WS_BWD, workspace).rec, keys);
  return launch_status("reverse projection k_proj_keys launch");
}

// srh_reverse_projection_bwd, and with `with_view` srh_reverse_projection_bwd_view
static int reverse_projection_bwd(bool with_view, const SrhReverseProjectionParams* params, const double* view1,
                                  const double* view2, const float* rgb, const float* in_pos, const float* out_pos,
                                  const float* mask, const int32_t* keys, const int32_t* order, void* workspace,
                                  size_t workspace_bytes, const float* g_out, const float* g_image1, const float* g_depth,
                                  float* grad_rgb, float* grad_in_pos, float* grad_out_pos, float* grad_rotated,
                                  double* grad_view1, double* grad_view2, void* view_workspace,
                                  size_t view_workspace_bytes, void* stream) {
  RProjDev R;
  int rc = rproj_setup(params, &R);
  if (rc) return rc;
  if ((rc = check_not_null({{"view1", view1}, {"view2", view2}, {"rgb", rgb}, {"in_pos", in_pos}, {"out_pos", out_pos},
                            {"mask", mask}})))
    return rc;
  if (!g_out && !g_image1 && !g_depth) return fail(SRH_E_NULL, "g_out, g_image1 and g_depth are all NULL");
  if (!with_view && !grad_rgb && !grad_in_pos && !grad_out_pos && !grad_rotated)
    return fail(SRH_E_NULL, "grad_rgb, grad_in_pos, grad_out_pos and grad_rotated are all NULL");
  if (with_view) {
    if (!grad_view1 && !grad_view2) return fail(SRH_E_NULL, "grad_view1 and grad_view2 are both NULL");
    if (grad_view1 && (rc = check_grad_view("grad_view1", grad_view1))) return rc;
    if (grad_view2 && (rc = check_grad_view("grad_view2", grad_view2))) return rc;
    if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, view_ws_bytes(R.B, R.nblk))))
      return rc;
  }
  const bool walk = grad_rgb || grad_in_pos || grad_view2;
  if (walk) {
    if ((rc = check_not_null({{"keys", keys}, {"order", order}}))) return rc;
    if ((rc = check_scratch("workspace", workspace, workspace_bytes, rproj_ws_bytes(R, SRH_RPROJ_WS_BWD)))) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  const RProjWs w = rproj_ws(R, SRH_RPROJ_WS_BWD, walk ? workspace : nullptr);   // without the walk, no region is used
  const dim3 grid(R.nblk, R.B), block(kProjBlock);
  if (walk) {
    if (hipError_t e = hipMemsetAsync(w.range, 0, (size_t)R.B * R.ncell * 2 * sizeof(int32_t), st))
      return hip_fail(e, "reverse projection cell ranges memset");
    hipLaunchKernelGGL(k_proj_mark, grid, block, 0, st, rproj_as_proj(R), keys, order, w.range);
  }
  // the two kView kernels share view_workspace: the stream orders camera 1's finish before the texel kernel's stores
  if (grad_view1) {
    hipLaunchKernelGGL(k_rproj_pixel_bwd<true>, grid, block, 0, st, R, view1, view2, rgb, in_pos, out_pos, mask, g_out,
                       g_image1, g_depth, w.gpl, grad_out_pos, grad_rotated, (double*)view_workspace);
    launch_view_finish(R.B, R.nblk, kViewSums, 0, view_workspace, grad_view1, st);
  } else {
    hipLaunchKernelGGL(k_rproj_pixel_bwd<false>, grid, block, 0, st, R, view1, view2, rgb, in_pos, out_pos, mask, g_out,
                       g_image1, g_depth, w.gpl, grad_out_pos, grad_rotated, (double*)nullptr);
  }
  if (grad_view2) {
    hipLaunchKernelGGL(k_rproj_texel_bwd<true>, grid, block, 0, st, R, view2, (const double*)w.rec, order,
                       (const int32_t*)w.range, (const double*)w.gpl, grad_rgb, grad_in_pos, in_pos,
                       (double*)view_workspace);
    launch_view_finish(R.B, R.nblk, kRProjView2Sums, kRProjView2First, view_workspace, grad_view2, st);
  } else if (walk) {
    hipLaunchKernelGGL(k_rproj_texel_bwd<false>, grid, block, 0, st, R, view2, (const double*)w.rec, order,
                       (const int32_t*)w.range, (const double*)w.gpl, grad_rgb, grad_in_pos, in_pos, (double*)nullptr);
  }
  return launch_status("reverse projection backward launch");
}

int srh_reverse_projection_bwd(const SrhReverseProjectionParams* params, const double* view1, const double* view2,
                               const float* rgb, const float* in_pos, const float* out_pos, const float* mask,
                               const int32_t* keys, const int32_t* order, void* workspace, size_t workspace_bytes,
                               const float* g_out, const float* g_image1, const float* g_depth, float* grad_rgb,
                               float* grad_in_pos, float* grad_out_pos, float* grad_rotated, void* stream) {
  return reverse_projection_bwd(false, params, view1, view2, rgb, in_pos, out_pos, mask, keys, order, workspace,
                                workspace_bytes, g_out, g_image1, g_depth, grad_rgb, grad_in_pos, grad_out_pos,
                                grad_rotated, nullptr, nullptr, nullptr, 0, stream);
}

int srh_reverse_projection_bwd_view(const SrhReverseProjectionParams* params, const double* view1, const double* view2,
                                    const float* rgb, const float* in_pos, const float* out_pos, const float* mask,
                                    const int32_t* keys, const int32_t* order, void* workspace, size_t workspace_bytes,
                                    const float* g_out, const float* g_image1, const float* g_depth, float* grad_rgb,
                                    float* grad_in_pos, float* grad_out_pos, float* grad_rotated, double* grad_view1,
                                    double* grad_view2, void* view_workspace, size_t view_workspace_bytes, void* stream) {
  return reverse_projection_bwd(true, params, view1, view2, rgb, in_pos, out_pos, mask, keys, order, workspace,
                                workspace_bytes, g_out, g_image1, g_depth, grad_rgb, grad_in_pos, grad_out_pos,
                                grad_rotated, grad_view1, grad_view2, view_workspace, view_workspace_bytes, stream);
}

}  // extern "C"

// ---- the dense Gaussian re-projection layer (srh_dense_projection.h) ---------------------------------------------
namespace {

// argument checks (no HIP call) and the device view of a dense projection launch
int dproj_setup(const SrhDenseProjectionParams* p, DProjDev* P) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_proj_frame(p->n_views, p->width, p->height, p->channels)) return rc;
  if (p->has_rotated != 0 && p->has_rotated != 1)
    return fail(SRH_E_TYPE, "has_rotated = %d, expected 0 or 1", p->has_rotated);
  if (!(p->sigma > 0.0 && std::isfinite(p->sigma)))
    return fail(SRH_E_RANGE, "sigma = %g, expected positive and finite", p->sigma);
  if (int rc = check_pinhole("", p->fovy, p->focal_length)) return rc;
  memset(P, 0, sizeof(*P));
  P->B = p->n_views; P->W = p->width; P->H = p->height; P->N = p->width * p->height; P->D = p->channels;
  P->flags = p->has_rotated ? kDProjHasRotated : 0;
  P->Wp = (P->W + kDProjStrip - 1) / kDProjStrip * kDProjStrip;
  const PixelScales s = pixel_scales(p->fovy, p->focal_length, P->W, P->H);
  P->fsx = s.fsx; P->fsy = s.fsy; P->cx0 = s.cx0; P->cy0 = s.cy0;
  P->h = 1.0 / (2.0 * p->sigma * p->sigma);
  P->q = exp(-2.0 * P->h);
  return SRH_OK;
}

// the rotated image is there exactly when the parameters say so
int dproj_check_rotated(const DProjDev& P, const float* rotated) {
  if ((P.flags & kDProjHasRotated) && !rotated) return fail(SRH_E_NULL, "rotated is NULL with has_rotated = 1");
  if (!(P.flags & kDProjHasRotated) && rotated) return fail(SRH_E_TYPE, "rotated is given with has_rotated = 0");
  return SRH_OK;
}

// SRH_DPROJ_WS_FWD: uv (B, N, 2) fp64
// SRH_DPROJ_WS_SAVED: sm = S, m (B, D + 1, N) fp64
// SRH_DPROJ_WS_BWD: gt (B, H, Wp, D + 1) fp64
// SRH_DPROJ_WS_VIEW: the partials of k_dproj_surfel_bwd<D, true, true>, 12 fp64 per one-wave workgroup (view_ws_bytes)
struct DProjWs {
  double *uv, *sm, *gt;
  size_t bytes;
};
DProjWs dproj_ws(const DProjDev& P, int which, const void* base = nullptr) {
  Regions r{(char*)base};
  DProjWs w = {};
  switch (which) {
    case SRH_DPROJ_WS_FWD: w.uv = r.take<double>((size_t)P.B * P.N * 2); break;
    case SRH_DPROJ_WS_SAVED: w.sm = r.take<double>((size_t)P.B * P.N * (P.D + 1)); break;
    default: w.gt = r.take<double>((size_t)P.B * P.H * P.Wp * (P.D + 1));
  }
  w.bytes = r.bytes;
  return w;
}
int dproj_bwd_groups(const DProjDev& P) { return (P.N + kDProjBwdBlock - 1) / kDProjBwdBlock; }
size_t dproj_ws_bytes(const DProjDev& P, int which) {
  return which == SRH_DPROJ_WS_VIEW ? view_ws_bytes(P.B, dproj_bwd_groups(P)) : dproj_ws(P, which).bytes;
}

// f(std::integral_constant<int, D>) for the channel count D (validated by dproj_setup)
template <class Fn>
void with_channels(int D, Fn f) {
  switch (D) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

}  // namespace

extern "C" {

size_t srh_dense_projection_workspace_bytes(const SrhDenseProjectionParams* params, int32_t which) {
  DProjDev P;
  if (dproj_setup(params, &P)) return 0;
  if ((which < SRH_DPROJ_WS_FWD || which > SRH_DPROJ_WS_BWD) && which != SRH_DPROJ_WS_VIEW) {
    fail(SRH_E_TYPE, "which = %d, expected SRH_DPROJ_WS_FWD, _SAVED, _BWD or _VIEW", which);
    return 0;
  }
  return dproj_ws_bytes(P, which);
}

int srh_dense_projection_fwd(const SrhDenseProjectionParams* params, const double* view, const float* surfels,
                             const float* rgb, const float* rotated, void* workspace, size_t workspace_bytes,
                             void* saved, size_t saved_bytes, float* out, float* mask, void* stream) {
  DProjDev P;
  int rc = dproj_setup(params, &P);
  if (rc || (rc = dproj_check_rotated(P, rotated))) return rc;
  if ((rc = check_not_null({{"view", view}, {"surfels", surfels}, {"rgb", rgb}, {"out", out}, {"mask", mask}}))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, dproj_ws_bytes(P, SRH_DPROJ_WS_FWD)))) return rc;
  if (saved && (rc = check_scratch("saved", saved, saved_bytes, dproj_ws_bytes(P, SRH_DPROJ_WS_SAVED)))) return rc;
  hipStream_t st = (hipStream_t)stream;
  double* uv = dproj_ws(P, SRH_DPROJ_WS_FWD, workspace).uv;
  hipLaunchKernelGGL(k_dproj_uv, dim3((P.N + kDProjBlock - 1) / kDProjBlock, P.B), dim3(kDProjBlock), 0, st, P, view,
                     surfels, uv);
  const int tiles = ((P.W + kDProjTile - 1) / kDProjTile) * ((P.H + kDProjTile - 1) / kDProjTile);
  with_channels(P.D, [&](auto d) {
    hipLaunchKernelGGL(k_dproj_fwd<decltype(d)::value>, dim3(tiles, P.B), dim3(kDProjFwdBlock), 0, st, P,
                       (const double*)uv, rgb, rotated, dproj_ws(P, SRH_DPROJ_WS_SAVED, saved).sm, out, mask);
  });
  return launch_status("dense projection forward launch");
}

// srh_dense_projection_bwd, and with `with_view` srh_dense_projection_bwd_view
static int dense_projection_bwd(bool with_view, const SrhDenseProjectionParams* params, const double* view,
                                const float* surfels, const float* rgb, const float* rotated, const void* saved,
                                size_t saved_bytes, void* workspace, size_t workspace_bytes, const float* g_out,
                                const float* g_mask, float* grad_surfels, float* grad_rgb, float* grad_rotated,
                                double* grad_view, void* view_workspace, size_t view_workspace_bytes, void* stream) {
  DProjDev P;
  int rc = dproj_setup(params, &P);
  if (rc || (rc = dproj_check_rotated(P, rotated))) return rc;
  if ((rc = check_not_null({{"view", view}, {"surfels", surfels}, {"rgb", rgb}}))) return rc;
  if (!g_out && !g_mask) return fail(SRH_E_NULL, "g_out and g_mask are both NULL");
  if (!with_view && !grad_surfels && !grad_rgb && !grad_rotated)
    return fail(SRH_E_NULL, "grad_surfels, grad_rgb and grad_rotated are all NULL");
  if (grad_rotated && !rotated) return fail(SRH_E_NULL, "grad_rotated without rotated");
  if ((rc = check_scratch("saved", saved, saved_bytes, dproj_ws_bytes(P, SRH_DPROJ_WS_SAVED)))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, dproj_ws_bytes(P, SRH_DPROJ_WS_BWD)))) return rc;
  if (with_view) {
    if ((rc = check_grad_view("grad_view", grad_view))) return rc;
    if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes,
                            dproj_ws_bytes(P, SRH_DPROJ_WS_VIEW))))
      return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  const double* sm = dproj_ws(P, SRH_DPROJ_WS_SAVED, saved).sm;
  double* gt = dproj_ws(P, SRH_DPROJ_WS_BWD, workspace).gt;
  hipLaunchKernelGGL(k_dproj_pixel_bwd, dim3((P.H * P.Wp + kDProjBlock - 1) / kDProjBlock, P.B), dim3(kDProjBlock), 0, st,
                     P, sm, rotated, g_out, g_mask, gt, grad_rotated);
  if (with_view || grad_surfels || grad_rgb) {
    const dim3 grid(dproj_bwd_groups(P), P.B), block(kDProjBwdBlock);
    with_channels(P.D, [&](auto d) {
      constexpr int D = decltype(d)::value;
      if (with_view)
        hipLaunchKernelGGL((k_dproj_surfel_bwd<D, true, true>), grid, block, 0, st, P, view, surfels, rgb,
                           (const double*)gt, grad_rgb, grad_surfels, (double*)view_workspace);
      else if (grad_surfels)
        hipLaunchKernelGGL((k_dproj_surfel_bwd<D, true, false>), grid, block, 0, st, P, view, surfels, rgb,
                           (const double*)gt, grad_rgb, grad_surfels, (double*)nullptr);
      else
        hipLaunchKernelGGL((k_dproj_surfel_bwd<D, false, false>), grid, block, 0, st, P, view, surfels, rgb,
                           (const double*)gt, grad_rgb, grad_surfels, (double*)nullptr);
    });
    if (with_view) launch_view_finish(P.B, grid.x, kViewSums, 0, view_workspace, grad_view, st);
  }
  return launch_status("dense projection backward launch");
}

int srh_dense_projection_bwd(const SrhDenseProjectionParams* params, const double* view, const float* surfels,
                             const float* rgb, const float* rotated, const void* saved, size_t saved_bytes,
                             void* workspace, size_t workspace_bytes, const float* g_out, const float* g_mask,
                             float* grad_surfels, float* grad_rgb, float* grad_rotated, void* stream) {
  return dense_projection_bwd(false, params, view, surfels, rgb, rotated, saved, saved_bytes, workspace, workspace_bytes,
                              g_out, g_mask, grad_surfels, grad_rgb, grad_rotated, nullptr, nullptr, 0, stream);
}

int srh_dense_projection_bwd_view(const SrhDenseProjectionParams* params, const double* view, const float* surfels,
                                  const float* rgb, const float* rotated, const void* saved, size_t saved_bytes,
                                  void* workspace, size_t workspace_bytes, const float* g_out, const float* g_mask,
                                  float* grad_surfels, float* grad_rgb, float* grad_rotated, double* grad_view,
                                  void* view_workspace, size_t view_workspace_bytes, void* stream) {
  return dense_projection_bwd(true, params, view, surfels, rgb, rotated, saved, saved_bytes, workspace, workspace_bytes,
                              g_out, g_mask, grad_surfels, grad_rgb, grad_rotated, grad_view, view_workspace,
                              view_workspace_bytes, stream);
}

}  // extern "C"

// ---- the depth lift (srh_surfels.h) ------------------------------------------------------------------------------
namespace {

static_assert(kSurfFrameCamera == SRH_SURFELS_FRAME_CAMERA && kSurfFrameWorld == SRH_SURFELS_FRAME_WORLD,
              "srh.h and srh_surfels.h");

// argument checks (no HIP call) and the device view of a lift; the view table is needed for the world frame only
int surf_setup(const SrhSurfelsParams* p, const double* view, SurfDev* S) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_batch_grid(p->n_views, p->width, p->height, "width x height =")) return rc;
  if (p->frame != SRH_SURFELS_FRAME_CAMERA && p->frame != SRH_SURFELS_FRAME_WORLD)
    return fail(SRH_E_TYPE, "frame = %d, expected SRH_SURFELS_FRAME_CAMERA or _WORLD", p->frame);
  if (int rc = check_pinhole("", p->fovy, p->focal_length)) return rc;
  if (p->frame == SRH_SURFELS_FRAME_WORLD && !view) return fail(SRH_E_NULL, "view is NULL");
  memset(S, 0, sizeof(*S));
  S->B = p->n_views; S->W = p->width; S->H = p->height; S->N = p->width * p->height; S->frame = p->frame;
  S->nblk = (S->N + kSurfBlock - 1) / kSurfBlock;
  const FrameSize fs = frame_size(p->fovy, p->focal_length, p->width, p->height);
  S->f = p->focal_length; S->half_w = fs.w / 2; S->half_h = fs.h / 2;
  S->step_x = p->width > 1 ? 2.0 / (p->width - 1) : 0.0;
  S->step_y = p->height > 1 ? -2.0 / (p->height - 1) : 0.0;
  return SRH_OK;
}

}  // namespace

extern "C" {

int srh_depth_to_surfels_fwd(const SrhSurfelsParams* params, const double* view, const float* depth, float* out,
                             void* stream) {
  SurfDev S;
  int rc = surf_setup(params, view, &S);
  if (rc) return rc;
  if ((rc = check_not_null({{"depth", depth}, {"out", out}}))) return rc;
  hipLaunchKernelGGL(k_surfels_fwd, dim3(S.nblk, S.B), dim3(kSurfBlock), 0, (hipStream_t)stream, S, view, depth, out);
  return launch_status("k_surfels_fwd launch");
}

int srh_depth_to_surfels_bwd(const SrhSurfelsParams* params, const double* view, const float* depth, const float* g_out,
                             float* grad_depth, void* stream) {
  SurfDev S;
  int rc = surf_setup(params, view, &S);
  if (rc) return rc;
  if ((rc = check_not_null({{"depth", depth}, {"g_out", g_out}, {"grad_depth", grad_depth}}))) return rc;
  hipLaunchKernelGGL(k_surfels_bwd<false>, dim3(S.nblk, S.B), dim3(kSurfBlock), 0, (hipStream_t)stream, S, view, depth,
                     g_out, grad_depth, (double*)nullptr);
  return launch_status("k_surfels_bwd launch");
}

size_t srh_view_grad_workspace_bytes(int32_t n_views, int32_t width, int32_t height) {
  if (check_batch_grid(n_views, width, height, "width x height =")) return 0;
  return view_ws_bytes(n_views, (width * height + kViewBlock - 1) / kViewBlock);
}

int srh_depth_to_surfels_bwd_view(const SrhSurfelsParams* params, const double* view, const float* depth,
                                  const float* g_out, float* grad_depth, double* grad_view, void* view_workspace,
                                  size_t view_workspace_bytes, void* stream) {
  SurfDev S;
  int rc = surf_setup(params, view, &S);
  if (rc) return rc;
  if (S.frame != kSurfFrameWorld)
    return fail(SRH_E_TYPE, "frame = %d: grad_view exists only for SRH_SURFELS_FRAME_WORLD", S.frame);
  if ((rc = check_not_null({{"depth", depth}, {"g_out", g_out}}))) return rc;
  if ((rc = check_grad_view("grad_view", grad_view))) return rc;
  if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, view_ws_bytes(S.B, S.nblk)))) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_surfels_bwd<true>, dim3(S.nblk, S.B), dim3(kSurfBlock), 0, st, S, view, depth, g_out, grad_depth,
                     (double*)view_workspace);
  launch_view_finish(S.B, S.nblk, kViewSums, 0, view_workspace, grad_view, st);
  return launch_status("depth_to_surfels backward (view) launch");
}

}  // extern "C"

// ---- the hard scatter-mean projection (srh_hard_projection.h) ----------------------------------------------------
namespace {

// argument checks (no HIP call) and the device view of a hard projection launch
int hproj_setup(const SrhHardProjectionParams* p, HProjDev* P) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_proj_frame(p->n_views, p->width, p->height, p->channels)) return rc;
  if (int rc = check_pinhole("", p->fovy, p->focal_length)) return rc;
  memset(P, 0, sizeof(*P));
  P->B = p->n_views; P->W = p->width; P->H = p->height; P->N = p->width * p->height; P->D = p->channels;
  P->nblk = (P->N + kProjBlock - 1) / kProjBlock;
  const PixelScales s = pixel_scales(p->fovy, p->focal_length, P->W, P->H);
  P->fsx = s.fsx; P->fsy = s.fsy; P->cx0 = s.cx0; P->cy0 = s.cy0;
  return SRH_OK;
}

}  // namespace

extern "C" {

int srh_hard_projection_keys(const SrhHardProjectionParams* params, const double* view, const float* surfels,
                             int32_t* keys, void* stream) {
  HProjDev P;
  int rc = hproj_setup(params, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"view", view}, {"surfels", surfels}, {"keys", keys}}))) return rc;
  hipLaunchKernelGGL(k_hproj_keys, dim3(P.nblk, P.B), dim3(kProjBlock), 0, (hipStream_t)stream, P, view, surfels, keys);
  return launch_status("k_hproj_keys launch");
}

int srh_hard_projection_fwd(const SrhHardProjectionParams* params, const float* rgb, const int32_t* keys,
                            const int32_t* order, float* out, uint8_t* mask, int32_t* count, void* stream) {
  HProjDev P;
  int rc = hproj_setup(params, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"rgb", rgb}, {"keys", keys}, {"order", order}, {"out", out}, {"mask", mask},
                            {"count", count}})))
    return rc;
  hipLaunchKernelGGL(k_hproj_gather, dim3(P.nblk, P.B), dim3(kProjBlock), 0, (hipStream_t)stream, P, keys, order, rgb,
                     out, mask, count);
  return launch_status("k_hproj_gather launch");
}

int srh_hard_projection_bwd(const SrhHardProjectionParams* params, const int32_t* keys, const int32_t* count,
                            const float* g_out, float* grad_rgb, void* stream) {
  HProjDev P;
  int rc = hproj_setup(params, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"keys", keys}, {"count", count}, {"g_out", g_out}, {"grad_rgb", grad_rgb}}))) return rc;
  hipLaunchKernelGGL(k_hproj_bwd, dim3(P.nblk, P.B), dim3(kProjBlock), 0, (hipStream_t)stream, P, keys, count, g_out,
                     grad_rgb);
  return launch_status("k_hproj_bwd launch");
}

}  // extern "C"

// ---- normals from a grid of points (srh_normals.h) ---------------------------------------------------------------
namespace {

size_t norm_ws_bytes(int32_t n_views, int32_t width, int32_t height) {
  return (size_t)n_views * width * height * kNormMoments * sizeof(double);
}

// argument checks (no HIP call) and the device view of a plane-fit launch.  Every index in srh_normals.h is a size_t
// built from q < W H <= 2^24 and b < 65536, so check_batch_grid's limits are the 32-bit limits too.
int norm_setup(int32_t n_views, int32_t width, int32_t height, NormDev* S) {
  if (int rc = check_batch_grid(n_views, width, height, "width x height =")) return rc;
  if (width < 2 || height < 2)
    return fail(SRH_E_RANGE, "width x height = %d x %d: the reflected 3 x 3 stencil needs both sides >= 2", width, height);
  S->B = n_views; S->W = width; S->H = height; S->N = width * height;
  S->nblk = (S->N + kNormBlock - 1) / kNormBlock;
  return SRH_OK;
}

}  // namespace

extern "C" {

size_t srh_normals_workspace_bytes(int32_t n_views, int32_t width, int32_t height) {
  NormDev S;
  if (norm_setup(n_views, width, height, &S)) return 0;
  return norm_ws_bytes(n_views, width, height);
}

int srh_normals_fwd(int32_t n_views, int32_t width, int32_t height, const double* rot, const float* pos, float* out,
                    void* stream) {
  NormDev S;
  int rc = norm_setup(n_views, width, height, &S);
  if (rc) return rc;
  if ((rc = check_not_null({{"pos", pos}, {"out", out}}))) return rc;
  hipLaunchKernelGGL(k_normals_fwd, dim3(S.nblk, S.B), dim3(kNormBlock), 0, (hipStream_t)stream, S, rot, pos, out);
  return launch_status("k_normals_fwd launch");
}

int srh_normals_bwd(int32_t n_views, int32_t width, int32_t height, const double* rot, const float* pos,
                    const float* g_out, void* workspace, size_t workspace_bytes, float* grad_pos, void* stream) {
  NormDev S;
  int rc = norm_setup(n_views, width, height, &S);
  if (rc) return rc;
  if ((rc = check_not_null({{"pos", pos}, {"g_out", g_out}, {"grad_pos", grad_pos}}))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, norm_ws_bytes(S.B, S.W, S.H)))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_normals_bwd<false>, dim3(S.nblk, S.B), dim3(kNormBlock), 0, st, S, rot, pos, g_out,
                     (double*)workspace, (double*)nullptr);
  hipLaunchKernelGGL(k_normals_gather, dim3(S.nblk, S.B), dim3(kNormBlock), 0, st, S, pos, (const double*)workspace,
                     grad_pos);
  return launch_status("normals backward launch");
}

int srh_normals_bwd_view(int32_t n_views, int32_t width, int32_t height, const double* rot, const float* pos,
                         const float* g_out, void* workspace, size_t workspace_bytes, float* grad_pos, double* grad_rot,
                         void* view_workspace, size_t view_workspace_bytes, void* stream) {
  static_assert(kViewBlock == kNormBlock, "view_block_reduce's workgroup is the plane fit's");
  NormDev S;
  int rc = norm_setup(n_views, width, height, &S);
  if (rc) return rc;
  if ((rc = check_not_null({{"rot", rot}, {"pos", pos}, {"g_out", g_out}}))) return rc;
  if (grad_pos && (rc = check_scratch("workspace", workspace, workspace_bytes, norm_ws_bytes(S.B, S.W, S.H)))) return rc;
  if ((rc = check_grad_view("grad_rot", grad_rot))) return rc;
  if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, view_ws_bytes(S.B, S.nblk)))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_normals_bwd<true>, dim3(S.nblk, S.B), dim3(kNormBlock), 0, st, S, rot, pos, g_out,
                     grad_pos ? (double*)workspace : nullptr, (double*)view_workspace);
  launch_view_finish(S.B, S.nblk, 9, 0, view_workspace, grad_rot, st);
  if (grad_pos)
    hipLaunchKernelGGL(k_normals_gather, dim3(S.nblk, S.B), dim3(kNormBlock), 0, st, S, pos, (const double*)workspace,
                       grad_pos);
  return launch_status("normals backward (view) launch");
}

}  // extern "C"

// ---- the frame transforms and the point projection (srh_frames.h) ------------------------------------------------
namespace {

static_assert(kViewBlock == kFrameBlock, "view_block_reduce's workgroup is the frame kernels'");

constexpr int32_t kFrameMaxPoints = 1 << 24;

// argument checks (no HIP call) and the device view of a frame transform; a table is needed where its input is there
int frame_setup(const SrhFrameParams* p, const double* view_pos, const double* view_normal, FramesDev* F) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_n_views(p->n_views)) return rc;
  if (p->n_pos < 0 || p->n_pos > kFrameMaxPoints) return fail(SRH_E_RANGE, "n_pos = %d, expected 0..2^24", p->n_pos);
  if (p->n_normal < 0 || p->n_normal > kFrameMaxPoints)
    return fail(SRH_E_RANGE, "n_normal = %d, expected 0..2^24", p->n_normal);
  if (p->n_pos == 0 && p->n_normal == 0) return fail(SRH_E_RANGE, "n_pos and n_normal are both 0");
  if (p->n_pos && p->pos_cols != 3 && p->pos_cols != 4)
    return fail(SRH_E_RANGE, "pos_cols = %d, expected 3 or 4", p->pos_cols);
  if (p->n_normal && p->normal_cols != 3 && p->normal_cols != 4)
    return fail(SRH_E_RANGE, "normal_cols = %d, expected 3 or 4", p->normal_cols);
  if (p->n_pos && !view_pos) return fail(SRH_E_NULL, "view_pos is NULL");
  if (p->n_normal && !view_normal) return fail(SRH_E_NULL, "view_normal is NULL");
  memset(F, 0, sizeof(*F));
  F->B = p->n_views; F->n_pos = p->n_pos; F->n_normal = p->n_normal;
  F->pos_cols = p->pos_cols; F->normal_cols = p->normal_cols;
  F->nblk = ((p->n_pos > p->n_normal ? p->n_pos : p->n_normal) + kFrameBlock - 1) / kFrameBlock;
  return SRH_OK;
}

// the pointers of the half that is there: `pos_*` with n_pos > 0, `normal_*` with n_normal > 0
int frame_check_halves(const FramesDev& F, NamedPtr pos_a, NamedPtr pos_b, NamedPtr normal_a, NamedPtr normal_b) {
  if (F.n_pos)
    if (int rc = check_not_null({pos_a, pos_b})) return rc;
  if (F.n_normal)
    if (int rc = check_not_null({normal_a, normal_b})) return rc;
  return SRH_OK;
}

// argument checks (no HIP call) and the device view of a projection of points
int pcoord_setup(const SrhProjectCoordsParams* p, PCoordDev* P) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_n_views(p->n_views)) return rc;
  if (p->n_points < 1 || p->n_points > kFrameMaxPoints)
    return fail(SRH_E_RANGE, "n_points = %d, expected 1..2^24", p->n_points);
  if (p->cols != 3 && p->cols != 4) return fail(SRH_E_RANGE, "cols = %d, expected 3 or 4", p->cols);
  if (int rc = check_grid_size(p->width, p->height, "width x height =")) return rc;
  if (int rc = check_pinhole("", p->fovy, p->focal_length)) return rc;
  memset(P, 0, sizeof(*P));
  P->B = p->n_views; P->N = p->n_points; P->cols = p->cols; P->W = p->width; P->H = p->height;
  P->nblk = (P->N + kFrameBlock - 1) / kFrameBlock;
  const FrameSize fs = frame_size(p->fovy, p->focal_length, P->W, P->H);
  P->f = p->focal_length;
  P->sx = -(double)(P->W - 1) / fs.w; P->sy = (double)(P->H - 1) / fs.h;
  P->hx = P->W / 2.0; P->hy = P->H / 2.0;
  const PixelScales s = pixel_scales(p->fovy, p->focal_length, P->W, P->H);
  P->fsx = s.fsx; P->fsy = s.fsy; P->cx0 = s.cx0; P->cy0 = s.cy0;
  return SRH_OK;
}

int project_coordinates_bwd(bool with_view, const SrhProjectCoordsParams* params, const double* view,
                            const float* surfels, const float* g_plane, const float* g_coord, float* grad_surfels,
                            double* grad_view, void* view_workspace, size_t view_workspace_bytes, void* stream) {
  PCoordDev P;
  int rc = pcoord_setup(params, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"view", view}, {"surfels", surfels}}))) return rc;
  if (!g_plane && !g_coord) return fail(SRH_E_NULL, "g_plane and g_coord are both NULL");
  const hipStream_t st = (hipStream_t)stream;
  if (!with_view) {
    if ((rc = check_not_null({{"grad_surfels", grad_surfels}}))) return rc;
    hipLaunchKernelGGL(k_project_bwd<false>, dim3(P.nblk, P.B), dim3(kFrameBlock), 0, st, P, view, surfels, g_plane,
                       g_coord, grad_surfels, (double*)nullptr);
    return launch_status("k_project_bwd launch");
  }
  if ((rc = check_grad_view("grad_view", grad_view))) return rc;
  if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, view_ws_bytes(P.B, P.nblk)))) return rc;
  hipLaunchKernelGGL(k_project_bwd<true>, dim3(P.nblk, P.B), dim3(kFrameBlock), 0, st, P, view, surfels, g_plane,
                     g_coord, grad_surfels, (double*)view_workspace);
  launch_view_finish(P.B, P.nblk, kViewSums, 0, view_workspace, grad_view, st);
  return launch_status("project_coordinates backward (view) launch");
}

}  // namespace

extern "C" {

int srh_frame_transform_fwd(const SrhFrameParams* params, const double* view_pos, const double* view_normal,
                            const float* pos, const float* normal, float* out_pos, float* out_normal, void* stream) {
  FramesDev F;
  int rc = frame_setup(params, view_pos, view_normal, &F);
  if (rc) return rc;
  if ((rc = frame_check_halves(F, {"pos", pos}, {"out_pos", out_pos}, {"normal", normal}, {"out_normal", out_normal})))
    return rc;
  hipLaunchKernelGGL(k_frames_fwd, dim3(F.nblk, F.B), dim3(kFrameBlock), 0, (hipStream_t)stream, F, view_pos,
                     view_normal, pos, normal, out_pos, out_normal);
  return launch_status("k_frames_fwd launch");
}

int srh_frame_transform_bwd(const SrhFrameParams* params, const double* view_pos, const double* view_normal,
                            const float* g_pos, const float* g_normal, float* grad_pos, float* grad_normal,
                            void* stream) {
  FramesDev F;
  int rc = frame_setup(params, view_pos, view_normal, &F);
  if (rc) return rc;
  if ((rc = frame_check_halves(F, {"g_pos", g_pos}, {"g_pos", g_pos}, {"g_normal", g_normal}, {"g_normal", g_normal})))
    return rc;
  if (!(F.n_pos && grad_pos) && !(F.n_normal && grad_normal))
    return fail(SRH_E_NULL, "grad_pos and grad_normal are both NULL or absent");
  hipLaunchKernelGGL(k_frames_bwd<false>, dim3(F.nblk, F.B), dim3(kFrameBlock), 0, (hipStream_t)stream, F, view_pos,
                     view_normal, (const float*)nullptr, (const float*)nullptr, g_pos, g_normal, grad_pos, grad_normal,
                     (double*)nullptr, (double*)nullptr);
  return launch_status("k_frames_bwd launch");
}

int srh_frame_transform_bwd_view(const SrhFrameParams* params, const double* view_pos, const double* view_normal,
                                 const float* pos, const float* normal, const float* g_pos, const float* g_normal,
                                 float* grad_pos, float* grad_normal, double* grad_view_pos, double* grad_view_normal,
                                 void* view_workspace, size_t view_workspace_bytes, void* stream) {
  FramesDev F;
  int rc = frame_setup(params, view_pos, view_normal, &F);
  if (rc) return rc;
  if ((rc = frame_check_halves(F, {"pos", pos}, {"g_pos", g_pos}, {"normal", normal}, {"g_normal", g_normal})))
    return rc;
  if (!grad_view_pos && !grad_view_normal) return fail(SRH_E_NULL, "grad_view_pos and grad_view_normal are both NULL");
  if (grad_view_pos && (rc = check_grad_view("grad_view_pos", grad_view_pos))) return rc;
  if (grad_view_normal && (rc = check_grad_view("grad_view_normal", grad_view_normal))) return rc;
  const size_t half = view_ws_bytes(F.B, F.nblk);
  if ((rc = check_scratch("view_workspace", view_workspace, view_workspace_bytes, 2 * half))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  double* part_pos = grad_view_pos ? (double*)view_workspace : nullptr;
  double* part_normal = grad_view_normal ? (double*)((char*)view_workspace + half) : nullptr;
  hipLaunchKernelGGL(k_frames_bwd<true>, dim3(F.nblk, F.B), dim3(kFrameBlock), 0, st, F, view_pos, view_normal, pos,
                     normal, g_pos, g_normal, F.n_pos ? grad_pos : nullptr, F.n_normal ? grad_normal : nullptr,
                     part_pos, part_normal);
  if (part_pos) launch_view_finish(F.B, F.nblk, kViewSums, 0, part_pos, grad_view_pos, st);
  if (part_normal) launch_view_finish(F.B, F.nblk, kViewSums, 0, part_normal, grad_view_normal, st);
  return launch_status("frame_transform backward (view) launch");
}

int srh_project_coordinates_fwd(const SrhProjectCoordsParams* params, const double* view, const float* surfels,
                                float* plane, float* px_coord, int32_t* px_idx, void* stream) {
  PCoordDev P;
  int rc = pcoord_setup(params, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"view", view}, {"surfels", surfels}}))) return rc;
  if (!plane && !px_coord && !px_idx) return fail(SRH_E_NULL, "plane, px_coord and px_idx are all NULL");
  hipLaunchKernelGGL(k_project_fwd, dim3(P.nblk, P.B), dim3(kFrameBlock), 0, (hipStream_t)stream, P, view, surfels,
                     plane, px_coord, px_idx);
  return launch_status("k_project_fwd launch");
}

int srh_project_coordinates_bwd(const SrhProjectCoordsParams* params, const double* view, const float* surfels,
                                const float* g_plane, const float* g_coord, float* grad_surfels, void* stream) {
  return project_coordinates_bwd(false, params, view, surfels, g_plane, g_coord, grad_surfels, nullptr, nullptr, 0,
                                 stream);
}

int srh_project_coordinates_bwd_view(const SrhProjectCoordsParams* params, const double* view, const float* surfels,
                                     const float* g_plane, const float* g_coord, float* grad_surfels, double* grad_view,
                                     void* view_workspace, size_t view_workspace_bytes, void* stream) {
  return project_coordinates_bwd(true, params, view, surfels, g_plane, g_coord, grad_surfels, grad_view, view_workspace,
                                 view_workspace_bytes, stream);
}

}  // extern "C"

// ---- nearest points between two point sets (srh_pointsets.h) -----------------------------------------------------
namespace {

constexpr int32_t kPsMaxPoints = 1 << 24;

// argument checks (no HIP call) and the device view of a point-set launch.  Every index in srh_pointsets.h is a size_t
// built from a point < 2^24, a view < 65536 and a column < 4.
int ps_setup(const SrhPointSetParams* p, const float* u, const float* v, PsDev* P) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_n_views(p->n_views)) return rc;
  if (p->n_u < 1 || p->n_u > kPsMaxPoints) return fail(SRH_E_RANGE, "n_u = %d, expected 1..2^24", p->n_u);
  if (p->n_v < 1 || p->n_v > kPsMaxPoints) return fail(SRH_E_RANGE, "n_v = %d, expected 1..2^24", p->n_v);
  if (p->dims < 1 || p->dims > kPsMaxD) return fail(SRH_E_RANGE, "dims = %d, expected 1..%d", p->dims, kPsMaxD);
  if (int rc = check_not_null({{"u", u}, {"v", v}})) return rc;
  memset(P, 0, sizeof(*P));
  P->B = p->n_views; P->N = p->n_u; P->M = p->n_v; P->D = p->dims; P->squared = p->squared != 0;
  return SRH_OK;
}

// f(std::integral_constant<int, D>) for D = `dims` (validated by ps_setup)
template <class Fn>
void with_ps_dims(int dims, Fn f) {
  switch (dims) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// the x extent of a grid over the sides `first` .. `first + count - 1` (0 = u, 1 = v), `block` points per workgroup
unsigned ps_blocks(const PsDev& P, int first, int count, int block) {
  int n = 0;
  for (int s = first; s < first + count; ++s) n = std::max(n, s ? P.M : P.N);
  return (unsigned)((n + block - 1) / block);
}

}  // namespace

extern "C" {

int srh_nearest_points_fwd(const SrhPointSetParams* params, const float* u, const float* v, float* dist_u,
                           int32_t* idx_u, float* dist_v, int32_t* idx_v, void* stream) {
  PsDev P;
  int rc = ps_setup(params, u, v, &P);
  if (rc) return rc;
  if (!dist_u != !idx_u) return fail(SRH_E_NULL, "%s is NULL and its partner is not", dist_u ? "idx_u" : "dist_u");
  if (!dist_v != !idx_v) return fail(SRH_E_NULL, "%s is NULL and its partner is not", dist_v ? "idx_v" : "dist_v");
  if (!dist_u && !dist_v) return fail(SRH_E_NULL, "dist_u / idx_u and dist_v / idx_v are all NULL");
  const int first = dist_u ? 0 : 1, count = (dist_u ? 1 : 0) + (dist_v ? 1 : 0);
  const dim3 grid(ps_blocks(P, first, count, kPsQueries), P.B, count);
  with_ps_dims(P.D, [&](auto d) {
    hipLaunchKernelGGL(k_ps_nearest<decltype(d)::value>, grid, dim3(kPsBlock), 0, (hipStream_t)stream, P, first, u, v,
                       dist_u, idx_u, dist_v, idx_v);
  });
  return launch_status("k_ps_nearest launch");
}

int srh_nearest_points_bwd(const SrhPointSetParams* params, const float* u, const float* v, const int32_t* idx_u,
                           const int32_t* idx_v, const int32_t* order_u, const int32_t* order_v, const double* g_dist_u,
                           const double* g_dist_v, float* grad_u, float* grad_v, void* stream) {
  PsDev P;
  int rc = ps_setup(params, u, v, &P);
  if (rc) return rc;
  if (!grad_u && !grad_v) return fail(SRH_E_NULL, "grad_u and grad_v are both NULL");
  // what an upstream gradient needs: its side's indices, and their order where the other side's gradient is wanted
  if (g_dist_u && !idx_u) return fail(SRH_E_NULL, "idx_u is NULL (g_dist_u is given)");
  if (g_dist_v && !idx_v) return fail(SRH_E_NULL, "idx_v is NULL (g_dist_v is given)");
  if (g_dist_u && grad_v && !order_u) return fail(SRH_E_NULL, "order_u is NULL (g_dist_u and grad_v are given)");
  if (g_dist_v && grad_u && !order_v) return fail(SRH_E_NULL, "order_v is NULL (g_dist_v and grad_u are given)");
  const int first = grad_u ? 0 : 1, count = (grad_u ? 1 : 0) + (grad_v ? 1 : 0);
  const dim3 grid(ps_blocks(P, first, count, kPsBwdBlock), P.B, count);
  with_ps_dims(P.D, [&](auto d) {
    hipLaunchKernelGGL(k_ps_bwd<decltype(d)::value>, grid, dim3(kPsBwdBlock), 0, (hipStream_t)stream, P, first, u, v,
                       idx_u, idx_v, order_u, order_v, g_dist_u, g_dist_v, grad_u, grad_v);
  });
  return launch_status("k_ps_bwd launch");
}

}  // extern "C"

// ---- uniform surface samples of a mesh (srh_mesh.h) --------------------------------------------------------------
namespace {

constexpr int32_t kMeshMax = 1 << 24;

// argument checks (no HIP call) and the device view of a mesh-sampling launch.  Every index in srh_mesh.h is an int32
// below 3 * 2^24 (a corner), or a size_t built from it, a view < 65536 and a column < 9.
int mesh_setup(const SrhMeshSampleParams* p, MeshDev* P) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_n_views(p->n_views)) return rc;
  if (p->n_vertices < 1 || p->n_vertices > kMeshMax)
    return fail(SRH_E_RANGE, "n_vertices = %d, expected 1..2^24", p->n_vertices);
  if (p->n_faces < 1 || p->n_faces > kMeshMax) return fail(SRH_E_RANGE, "n_faces = %d, expected 1..2^24", p->n_faces);
  if (p->n_samples < 1 || p->n_samples > kMeshMax)
    return fail(SRH_E_RANGE, "n_samples = %d, expected 1..2^24", p->n_samples);
  memset(P, 0, sizeof(*P));
  P->B = p->n_views; P->V = p->n_vertices; P->F = p->n_faces; P->S = p->n_samples;
  P->f_per_view = p->faces_per_view != 0; P->eye_per_view = p->eye_per_view != 0;
  return SRH_OK;
}

size_t mesh_cdf_bytes(const MeshDev& P) { return align_up((size_t)P.B * P.F * sizeof(double)); }

dim3 mesh_grid(int n, const MeshDev& P) { return dim3((unsigned)((n + kMeshBlock - 1) / kMeshBlock), P.B); }

}  // namespace

extern "C" {

size_t srh_mesh_sample_workspace_bytes(const SrhMeshSampleParams* params, int32_t which) {
  MeshDev P;
  if (mesh_setup(params, &P)) return 0;
  switch (which) {
    case SRH_MESH_WS_FWD: return mesh_cdf_bytes(P) + align_up((size_t)P.B * sizeof(double));
    case SRH_MESH_WS_BWD: return align_up((size_t)P.B * P.F * 9 * sizeof(double));
    default: fail(SRH_E_RANGE, "which = %d, expected SRH_MESH_WS_FWD or SRH_MESH_WS_BWD", which); return 0;
  }
}

int srh_mesh_sample_fwd(const SrhMeshSampleParams* params, const float* v, const int32_t* f, const double* eye,
                        const double* uniforms, void* workspace, size_t workspace_bytes, float* pos, float* normal,
                        int32_t* face, float* bary, void* stream) {
  MeshDev P;
  int rc = mesh_setup(params, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"v", v}, {"f", f}, {"uniforms", uniforms}, {"pos", pos}, {"normal", normal},
                            {"face", face}, {"bary", bary}})))
    return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes,
                          srh_mesh_sample_workspace_bytes(params, SRH_MESH_WS_FWD))))
    return rc;
  double* cdf = (double*)workspace;
  double* total = (double*)((char*)workspace + mesh_cdf_bytes(P));
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mesh_faces, mesh_grid(P.F, P), dim3(kMeshBlock), 0, s, P, v, f, eye, cdf);
  hipLaunchKernelGGL(k_mesh_scan, dim3(P.B), dim3(kMeshScanBlock), 0, s, P, cdf, total);
  hipLaunchKernelGGL(k_mesh_sample, mesh_grid(P.S, P), dim3(kMeshBlock), 0, s, P, v, f, uniforms, cdf, total, pos,
                     normal, face, bary);
  return launch_status("mesh sampling forward launch");
}

int srh_mesh_sample_bwd(const SrhMeshSampleParams* params, const float* v, const int32_t* f, const double* uniforms,
                        const int32_t* face, const int32_t* sample_order, const int32_t* corner_order,
                        const float* g_pos, const float* g_normal, void* workspace, size_t workspace_bytes,
                        float* grad_v, void* stream) {
  MeshDev P;
  int rc = mesh_setup(params, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"v", v}, {"f", f}, {"uniforms", uniforms}, {"face", face}, {"sample_order", sample_order},
                            {"corner_order", corner_order}, {"grad_v", grad_v}})))
    return rc;
  if (!g_pos && !g_normal) return fail(SRH_E_NULL, "g_pos and g_normal are both NULL");
  if ((rc = check_scratch("workspace", workspace, workspace_bytes,
                          srh_mesh_sample_workspace_bytes(params, SRH_MESH_WS_BWD))))
    return rc;
  double* corner = (double*)workspace;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mesh_bwd_faces, mesh_grid(P.F, P), dim3(kMeshBlock), 0, s, P, v, f, uniforms, face,
                     sample_order, g_pos, g_normal, corner);
  hipLaunchKernelGGL(k_mesh_bwd_vertices, mesh_grid(P.V, P), dim3(kMeshBlock), 0, s, P, f, corner_order, corner,
                     grad_v);
  return launch_status("mesh sampling backward launch");
}

}  // extern "C"

// ---- SH9 environment lighting (srh_sh9.h) ------------------------------------------------------------------------
namespace {

static_assert(kSh9MaxC == SRH_SH9_MAX_CHANNELS, "srh.h and srh_sh9.h");
constexpr int32_t kSh9MaxPoints = 1 << 24;

// argument checks (no HIP call) and the device view of an SH9 launch: `probe` checks the envmap's frame, else the
// normals' count.  Every index in srh_sh9.h is a size_t built from a pixel or normal < 2^24, a view < 65536, a channel
// < 4 and a column < 16.
int sh9_setup(const SrhSh9Params* p, bool probe, Sh9Dev* P) {
  if (!p) return fail(SRH_E_NULL, "params is NULL");
  if (int rc = check_n_views(p->n_views)) return rc;
  if (p->channels < 1 || p->channels > kSh9MaxC)
    return fail(SRH_E_RANGE, "channels = %d, expected 1..%d", p->channels, kSh9MaxC);
  if (probe) {
    if (int rc = check_grid_size(p->width, p->height, "width x height =")) return rc;
  } else if (p->n_points < 1 || p->n_points > kSh9MaxPoints) {
    return fail(SRH_E_RANGE, "n_points = %d, expected 1..2^24", p->n_points);
  }
  memset(P, 0, sizeof(*P));
  P->B = p->n_views; P->C = p->channels; P->m_per_view = p->m_per_view != 0;
  if (probe) { P->H = p->height; P->W = p->width; }
  else P->N = p->n_points;
  return SRH_OK;
}

// f(std::integral_constant<int, C>) for C = `channels` (validated by sh9_setup)
template <class Fn>
void with_sh9_channels(int channels, Fn f) {
  switch (channels) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

unsigned sh9_groups(int n) { return (unsigned)((n + kSh9Block - 1) / kSh9Block); }

// the partials of a reducing launch, and behind them (irradiance only) the finished monomial sums (B, C, 10)
size_t sh9_part_bytes(const Sh9Dev& P, int n, int K) {
  return align_up((size_t)P.C * P.B * sh9_groups(n) * K * sizeof(double));
}
size_t sh9_mono_bytes(const Sh9Dev& P) { return align_up((size_t)P.B * P.C * kSh9Monomials * sizeof(double)); }

}  // namespace

extern "C" {

size_t srh_sh9_workspace_bytes(const SrhSh9Params* params, int32_t which) {
  Sh9Dev P;
  switch (which) {
    case SRH_SH9_WS_PROJECT:
      if (sh9_setup(params, true, &P)) return 0;
      return sh9_part_bytes(P, P.H * P.W, kSh9Coeffs);
    case SRH_SH9_WS_IRRADIANCE_BWD:
      if (sh9_setup(params, false, &P)) return 0;
      return sh9_part_bytes(P, P.N, kSh9Monomials) + sh9_mono_bytes(P);
    default:
      fail(SRH_E_RANGE, "which = %d, expected SRH_SH9_WS_PROJECT or SRH_SH9_WS_IRRADIANCE_BWD", which);
      return 0;
  }
}

int srh_sh9_project_fwd(const SrhSh9Params* params, const float* envmap, void* workspace, size_t workspace_bytes,
                        float* L, void* stream) {
  Sh9Dev P;
  int rc = sh9_setup(params, true, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"envmap", envmap}, {"L", L}}))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes, srh_sh9_workspace_bytes(params, SRH_SH9_WS_PROJECT))))
    return rc;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned groups = sh9_groups(P.H * P.W);
  double* part = (double*)workspace;
  with_sh9_channels(P.C, [&](auto c) {
    hipLaunchKernelGGL(k_sh9_project<decltype(c)::value>, dim3(groups, P.B), dim3(kSh9Block), 0, s, P, envmap, part);
  });
  hipLaunchKernelGGL(k_sh9_finish<float>, dim3(P.C, P.B), dim3(kViewRows * kViewSums), 0, s, (int)groups, kSh9Coeffs,
                     (const double*)part, L);
  return launch_status("SH9 projection forward launch");
}

int srh_sh9_project_bwd(const SrhSh9Params* params, const float* g_L, float* grad_envmap, void* stream) {
  Sh9Dev P;
  int rc = sh9_setup(params, true, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"g_L", g_L}, {"grad_envmap", grad_envmap}}))) return rc;
  with_sh9_channels(P.C, [&](auto c) {
    hipLaunchKernelGGL(k_sh9_project_bwd<decltype(c)::value>, dim3(sh9_groups(P.H * P.W), P.B), dim3(kSh9Block), 0,
                       (hipStream_t)stream, P, g_L, grad_envmap);
  });
  return launch_status("k_sh9_project_bwd launch");
}

int srh_sh9_irradiance_fwd(const SrhSh9Params* params, const float* M, const float* normal, float* E, void* stream) {
  Sh9Dev P;
  int rc = sh9_setup(params, false, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"M", M}, {"normal", normal}, {"E", E}}))) return rc;
  with_sh9_channels(P.C, [&](auto c) {
    hipLaunchKernelGGL(k_sh9_irradiance_fwd<decltype(c)::value>, dim3(sh9_groups(P.N), P.B), dim3(kSh9Block), 0,
                       (hipStream_t)stream, P, M, normal, E);
  });
  return launch_status("k_sh9_irradiance_fwd launch");
}

int srh_sh9_irradiance_bwd(const SrhSh9Params* params, const float* M, const float* normal, const float* g_E,
                           float* grad_normal, double* grad_M, void* workspace, size_t workspace_bytes, void* stream) {
  Sh9Dev P;
  int rc = sh9_setup(params, false, &P);
  if (rc) return rc;
  if ((rc = check_not_null({{"M", M}, {"normal", normal}, {"g_E", g_E}}))) return rc;
  if (!grad_normal && !grad_M) return fail(SRH_E_NULL, "grad_normal and grad_M are both NULL");
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid(sh9_groups(P.N), P.B);
  if (!grad_M) {                        // an M that needs no gradient costs no reduction and no workspace
    with_sh9_channels(P.C, [&](auto c) {
      hipLaunchKernelGGL((k_sh9_irradiance_bwd<decltype(c)::value, false>), grid, dim3(kSh9Block), 0, s, P, M, normal,
                         g_E, grad_normal, (double*)nullptr);
    });
    return launch_status("k_sh9_irradiance_bwd launch");
  }
  if ((rc = check_grad_view("grad_M", grad_M))) return rc;
  if ((rc = check_scratch("workspace", workspace, workspace_bytes,
                          srh_sh9_workspace_bytes(params, SRH_SH9_WS_IRRADIANCE_BWD))))
    return rc;
  double* part = (double*)workspace;
  double* mono = (double*)((char*)workspace + sh9_part_bytes(P, P.N, kSh9Monomials));
  with_sh9_channels(P.C, [&](auto c) {
    hipLaunchKernelGGL((k_sh9_irradiance_bwd<decltype(c)::value, true>), grid, dim3(kSh9Block), 0, s, P, M, normal, g_E,
                       grad_normal, part);
  });
  hipLaunchKernelGGL(k_sh9_finish<double>, dim3(P.C, P.B), dim3(kViewRows * kViewSums), 0, s, (int)grid.x,
                     kSh9Monomials, (const double*)part, mono);
  const size_t entries = (size_t)(P.m_per_view ? P.B : 1) * 16 * P.C;
  hipLaunchKernelGGL(k_sh9_spread_M, dim3((unsigned)((entries + kSh9SpreadBlock - 1) / kSh9SpreadBlock)),
                     dim3(kSh9SpreadBlock), 0, s, P, (const double*)mono, grad_M);
  return launch_status("SH9 irradiance backward launch");
}

}  // extern "C"
