// The reference's surfel re-projection layer (projection_renderer_differentiable_fast, diffrend/torch/
// projection_layer.py:170-278 with project_image_coordinates :45-85, scatter_weighted_blended_oit torch/utils.py:178-215
// and blur :155-167), forward and analytic backward, restated as gathers; many views per launch (the view is grid
// dimension y).  See DESIGN.md "The surfel re-projection layer".
//
// Per view, N = W H surfels (world position p, D-channel value v):
//   cc = M [p, 1]                                  M = the view's 3 x 4 world-to-camera matrix, fp64, made by the host
//   (u, v) = (fsx X / nz(Z) + W/2 - 1/2, fsy Y / nz(Z) + H/2 - 1/2),  z = -Z,  nz(0) = 1
//   cell = floor(u, v), (fx, fy) = (u, v) - cell
//   a = alpha w,  alpha = exp(-2 (fx^2 + fy^2)) 2 / pi,  w = exp(-2 z)
//   corner k = 2 dx + dy sends the surfel to pixel cell + (dx, dy) with beta_k = (dx ? fx : 1 - fx)(dy ? fy : 1 - fy)
// and per pixel q, per corner k, over the surfels S(q, k) of cell q - (dx, dy), in ascending surfel index:
//   Q_k = sum v beta_k a / (nz(sum a) + 1e-8)      for v = the D channels, 1 (mask) and z (depth)
// The pre-blur image is sum_k Q_k; channels and mask are blurred (separable, normalised taps, zero padding), the depth is
// not; proj_merge_fwd is the reference's lines 251-276.
//
// Forward: k_proj_keys (one lane per surfel: record + cell key) -> the caller orders the keys (stable, ascending) ->
// k_proj_mark (cell ranges in the ordered list) -> k_proj_gather (one lane per pixel walks its four cells' lists) ->
// k_proj_blur_h -> k_proj_blur_v_merge.  Backward: k_proj_merge_bwd (per pixel) -> k_proj_blur_h -> k_proj_blur_v_corner
// (the blur is its own adjoint; per-corner gradients of numerators and denominators) -> k_proj_surfel_bwd (one lane per
// surfel reads its four destination pixels).  fp64 arithmetic, fp32 results, no float atomic, every output element
// written once: values and gradients are identical from run to run.
//
// Cells are indexed on the (W + 1) x (H + 1) grid of cell + (1, 1): a cell in column -1 or row -1 still reaches the
// frame through its +1 corners.  A surfel none of whose corners is in the frame gets the key (W + 1)(H + 1).
//
// The per-element arithmetic (proj_point, proj_surfel, proj_merge_fwd, proj_merge_bwd) is host-callable.
#pragma once
#include "srh_device.h"   // as_constant
#include "srh_view_grad.h"

namespace srh {

constexpr int kProjBlock = 256;
constexpr int kProjMaxD = 4;
constexpr int kProjMaxHalf = 64;
constexpr int kProjMaxBlur = 2 * kProjMaxD + 1;   // blurred channels: value, mask, rotated image

// SrhProjectionParams.flags (SRH_PROJ_*), plus what the entry points derive
constexpr int kProjUseDepth = 1, kProjUseCenterDist = 2, kProjBlurRotated = 4, kProjDetachMask = 8,
              kProjDetachMask2 = 16, kProjDetachDepthMerge = 32, kProjHasRotated = 1 << 8;

// Per-pixel planes (pre-blur, half-blurred, blurred, and their gradients) share one layout of P = 2 D + 2 channels:
// value [0, D), mask D, rotated image [D + 1, 2 D + 1), depth 2 D + 1.  The first D + 1 or 2 D + 1 of them are blurred.
// Per-corner rows have CS = D + 3 slots: Q of the D channels, of the mask, of the depth, then 1 / (nz(sum a) + 1e-8).
// Both are stored channel-major, (B, P, N) and (B, 4, CS, N) fp64 (proj_plane, proj_corner): the lanes of a wave hold
// neighbouring pixels, so each of their loads and stores covers consecutive addresses.
struct ProjDev {
  int B, W, H, N, D, P, CS, half, flags, ncell, nblk;
  double fsx, fsy, cx0, cy0;          // u = fsx X / Z + cx0, v = fsy Y / Z + cy0
  double taps[kProjMaxHalf + 1];      // taps[|d|]
};

__host__ __device__ __forceinline__ size_t proj_plane(const ProjDev& P, int b, int ch, int q) {
  return ((size_t)b * P.P + ch) * P.N + q;
}
__host__ __device__ __forceinline__ size_t proj_corner(const ProjDev& P, int b, int k, int slot, int q) {
  return (((size_t)b * 4 + k) * P.CS + slot) * P.N + q;
}

// A world point seen by a camera with the pixel scales (fsx, fsy, cx0, cy0) in a W x H frame: camera coordinates,
// (u, v), the cell floor(u, v) and the fractions.  The one copy of this arithmetic: the reverse layer walks the records
// k_proj_keys writes with it, so both layers must get the same cell and fractions bit for bit.
struct ProjPoint {
  double X, Y, Z, Zd, u, v, fx, fy;
  int ix, iy;      // the cell
  bool live;       // at least one corner can be in the frame
};

__host__ __device__ __forceinline__ ProjPoint proj_point(double fsx, double fsy, double cx0, double cy0, int W, int H,
                                                         const double* M, const float* p) {
  ProjPoint S;
  const double x = p[0], y = p[1], z = p[2];
  S.X = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  S.Y = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  S.Z = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  S.Zd = S.Z != 0.0 ? S.Z : 1.0;                       // nonzero_divide
  S.u = fsx * (S.X / S.Zd) + cx0;
  S.v = fsy * (S.Y / S.Zd) + cy0;
  const double cu = floor(S.u), cv = floor(S.v);
  // NaN and anything an int cannot hold fail these comparisons
  S.live = cu >= -1.0 && cu <= (double)(W - 1) && cv >= -1.0 && cv <= (double)(H - 1);
  S.ix = S.live ? (int)cu : 0;
  S.iy = S.live ? (int)cv : 0;
  S.fx = S.u - cu;
  S.fy = S.v - cv;
  return S;
}

// the projected point (without u, v: the cell and the fractions are all the kernels read) plus the surfel's depth and
// its two weights
struct ProjSurfel {
  double X, Y, Z, Zd, fx, fy, z, alpha, w;
  int ix, iy;
  bool live;
};

__host__ __device__ inline ProjSurfel proj_surfel(const ProjDev& P, const double* M, const float* p) {
  const ProjPoint Q = proj_point(P.fsx, P.fsy, P.cx0, P.cy0, P.W, P.H, M, p);
  ProjSurfel S;
  S.X = Q.X; S.Y = Q.Y; S.Z = Q.Z; S.Zd = Q.Zd; S.fx = Q.fx; S.fy = Q.fy; S.ix = Q.ix; S.iy = Q.iy; S.live = Q.live;
  S.z = -S.Z;
  S.alpha = (P.flags & kProjUseCenterDist) ? exp(-2.0 * (S.fx * S.fx + S.fy * S.fy)) * 0.63661977236758134308 : 1.0;
  S.w = (P.flags & kProjUseDepth) ? exp(-2.0 * S.z) : 1.0;
  return S;
}

__host__ __device__ __forceinline__ double proj_beta(int k, double fx, double fy) {
  return ((k & 2) ? fx : 1.0 - fx) * ((k & 1) ? fy : 1.0 - fy);
}

// The merge of one pixel (projection_layer.py:251-276): rb, rot D channels, m the blurred mask, dp the pre-blur depth.
__host__ __device__ inline void proj_merge_fwd(const ProjDev& P, const double rb[kProjMaxD], double m, double dp,
                                               const double rot[kProjMaxD], double out[kProjMaxD],
                                               double image1[kProjMaxD], double& depth) {
  const bool pos = m > 0.0;
  const double mnz = (pos ? m : 1.0) + 1.0e-20;
  depth = pos ? dp / mnz : dp;
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    if (c >= P.D) continue;
    image1[c] = pos ? rb[c] / mnz : rb[c];
    if (!(P.flags & kProjHasRotated)) out[c] = image1[c];
    else if (!(P.flags & kProjDetachMask) && (P.flags & kProjDetachMask2)) out[c] = m * image1[c] + (1.0 - m) * rot[c];
    else out[c] = m > 1.0 ? rb[c] / mnz : rb[c] + rot[c] * (1.0 - m);
  }
}

// Its vector-Jacobian product; g_* are the upstream gradients (0 where not wanted).  The detach flags cut the paths
// the reference cuts: detach_mask the mask in both branches of `out`, detach_mask2 the mask as the blend weight (the
// mask inside image1 keeps its gradient).
__host__ __device__ inline void proj_merge_bwd(const ProjDev& P, const double rb[kProjMaxD], double m, double dp,
                                               const double rot[kProjMaxD], const double g_out[kProjMaxD], double g_mask,
                                               const double g_image1[kProjMaxD], double g_depth, double g_rb[kProjMaxD],
                                               double& g_m, double g_rot[kProjMaxD], double& g_dp) {
  const bool pos = m > 0.0;
  const double mnz = (pos ? m : 1.0) + 1.0e-20;
  g_m = g_mask;
  g_dp = pos ? g_depth / mnz : g_depth;
  if (pos) g_m -= g_depth * dp / (mnz * mnz);
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    g_rb[c] = 0.0; g_rot[c] = 0.0;
    if (c >= P.D) continue;
    double g_i1 = g_image1[c];          // gradient reaching image1 = pos ? rb / mnz : rb
    if (!(P.flags & kProjHasRotated)) g_i1 += g_out[c];
    else if (!(P.flags & kProjDetachMask) && (P.flags & kProjDetachMask2)) {
      g_i1 += g_out[c] * m;
      g_rot[c] = g_out[c] * (1.0 - m);
    } else {
      const bool cut = P.flags & kProjDetachMask;
      if (m > 1.0) {
        g_rb[c] += g_out[c] / mnz;
        if (!cut) g_m -= g_out[c] * rb[c] / (mnz * mnz);
      } else {
        g_rb[c] += g_out[c];
        g_rot[c] = g_out[c] * (1.0 - m);
        if (!cut) g_m -= g_out[c] * rot[c];
      }
    }
    if (pos) {
      g_rb[c] += g_i1 / mnz;
      g_m -= g_i1 * rb[c] / (mnz * mnz);
    } else {
      g_rb[c] += g_i1;
    }
  }
}

// the view's matrix is the same for every lane and written before the launch: scalar loads
__device__ __forceinline__ void proj_load_view(const double* view, int b, double M[12]) {
  const auto* m = as_constant(view) + (size_t)b * 12;
#pragma unroll
  for (int j = 0; j < 12; ++j) M[j] = m[j];
}

// Forward 1: one lane per surfel.  rec (B, N, 4) fp64 = fx, fy, z, a; keys (B, N) int32.
__global__ __launch_bounds__(kProjBlock) void k_proj_keys(ProjDev P, const double* __restrict__ view,
                                                          const float* __restrict__ surfels, double* __restrict__ rec,
                                                          int32_t* __restrict__ keys) {
  const int s = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= P.N) return;
  const size_t o = (size_t)b * P.N + s;
  double M[12];
  proj_load_view(view, b, M);
  const ProjSurfel S = proj_surfel(P, M, surfels + 3 * o);
  rec[4 * o] = S.fx; rec[4 * o + 1] = S.fy; rec[4 * o + 2] = S.z; rec[4 * o + 3] = S.alpha * S.w;
  keys[o] = S.live ? (S.iy + 1) * (P.W + 1) + (S.ix + 1) : P.ncell;
}

// Forward 2: one lane per position of the ordered list; range (B, ncell, 2) int32 = [first, last + 1) of each cell's
// run, zero-filled before (an empty cell keeps [0, 0)).  Each slot has one writer.
__global__ __launch_bounds__(kProjBlock) void k_proj_mark(ProjDev P, const int32_t* __restrict__ keys,
                                                          const int32_t* __restrict__ order, int32_t* __restrict__ range) {
  const int i = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= P.N) return;
  const size_t base = (size_t)b * P.N;
  auto key_at = [&](int j) {
    const int32_t s = order[base + j];
    return (uint32_t)s < (uint32_t)P.N ? keys[base + s] : P.ncell;   // a bad `order` entry joins the dropped ones
  };
  const int32_t k = key_at(i);
  if ((uint32_t)k >= (uint32_t)P.ncell) return;
  int32_t* r = range + ((size_t)b * P.ncell + k) * 2;
  if (i == 0 || key_at(i - 1) != k) r[0] = i;
  if (i == P.N - 1 || key_at(i + 1) != k) r[1] = i + 1;
}

// Forward 3: one lane per pixel walks the lists of its four source cells and accumulates in list order.  pre (planes)
// gets the pre-blur value, mask, depth and (when it is to be blurred) the rotated image; cor (corner rows) the
// per-corner quotients for the backward, NULL = not wanted.
__global__ __launch_bounds__(kProjBlock) void k_proj_gather(ProjDev P, const double* __restrict__ rec,
                                                            const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ range,
                                                            const float* __restrict__ rgb, const float* __restrict__ rot,
                                                            double* __restrict__ pre, double* __restrict__ cor) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= P.N) return;
  const int qy = q / P.W, qx = q - qy * P.W;
  const size_t base = (size_t)b * P.N;
  double tot[kProjMaxD + 2];
#pragma unroll
  for (int c = 0; c < kProjMaxD + 2; ++c) tot[c] = 0.0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int cell = (qy - (k & 1) + 1) * (P.W + 1) + (qx - (k >> 1) + 1);
    const int32_t* r = range + ((size_t)b * P.ncell + cell) * 2;
    const int i0 = r[0], i1 = r[1];
    double num[kProjMaxD + 2], den = 0.0;
#pragma unroll
    for (int c = 0; c < kProjMaxD + 2; ++c) num[c] = 0.0;
    for (int i = i0; i < i1; ++i) {
      const int32_t s = order[base + i];
      if ((uint32_t)s >= (uint32_t)P.N) continue;
      const double* e = rec + 4 * (base + s);
      const double a = e[3], wgt = proj_beta(k, e[0], e[1]) * a;
      const float* v = rgb + (base + s) * P.D;
#pragma unroll
      for (int c = 0; c < kProjMaxD; ++c)
        if (c < P.D) num[c] += (double)v[c] * wgt;
      num[kProjMaxD] += wgt;
      num[kProjMaxD + 1] += e[2] * wgt;
      den += a;
    }
    const double inv = 1.0 / ((den != 0.0 ? den : 1.0) + 1.0e-8);
#pragma unroll
    for (int c = 0; c < kProjMaxD + 2; ++c) {
      if (c < kProjMaxD && c >= P.D) continue;
      const double Q = num[c] * inv;
      tot[c] += Q;
      if (cor) cor[proj_corner(P, b, k, c < kProjMaxD ? c : P.D + (c - kProjMaxD), q)] = Q;
    }
    if (cor) cor[proj_corner(P, b, k, P.D + 2, q)] = inv;
  }
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    if (c >= P.D) continue;
    pre[proj_plane(P, b, c, q)] = tot[c];
    if ((P.flags & kProjHasRotated) && (P.flags & kProjBlurRotated))
      pre[proj_plane(P, b, P.D + 1 + c, q)] = rot[(base + q) * P.D + c];
  }
  pre[proj_plane(P, b, P.D, q)] = tot[kProjMaxD];
  pre[proj_plane(P, b, 2 * P.D + 1, q)] = tot[kProjMaxD + 1];
}

// Horizontal blur of the first nb channels of every pixel, zero padding; one lane per (channel, pixel).
__global__ __launch_bounds__(kProjBlock) void k_proj_blur_h(ProjDev P, int nb, const double* __restrict__ in,
                                                            double* __restrict__ out) {
  const int e = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (e >= P.N * nb) return;
  const int ch = e / P.N, q = e - ch * P.N;
  const int x = q % P.W;
  const double* row = in + proj_plane(P, b, ch, q);
  double acc = 0.0;
  const int d0 = max(-P.half, -x), d1 = min(P.half, P.W - 1 - x);
  for (int d = d0; d <= d1; ++d) acc += P.taps[abs(d)] * row[d];
  out[proj_plane(P, b, ch, q)] = acc;
}

// the vertical half of the blur of pixel (x, y): the first nb channels of `in` into acc
__device__ __forceinline__ void proj_blur_v(const ProjDev& P, int nb, const double* __restrict__ in, int b, int x,
                                            int y, double acc[kProjMaxBlur]) {
#pragma unroll
  for (int c = 0; c < kProjMaxBlur; ++c) acc[c] = 0.0;
  const int d0 = max(-P.half, -y), d1 = min(P.half, P.H - 1 - y);
  for (int d = d0; d <= d1; ++d) {
    const double t = P.taps[abs(d)];
    const double* row = in + proj_plane(P, b, 0, (y + d) * P.W + x);
#pragma unroll
    for (int c = 0; c < kProjMaxBlur; ++c)
      if (c < nb) acc[c] += t * row[(size_t)c * P.N];
  }
}

// Forward 5: vertical blur fused with the merge; one lane per pixel.  blr (planes) keeps the blurred value, mask,
// rotated image as merged and the pre-blur depth for the backward (NULL = not wanted); depth may be NULL.
__global__ __launch_bounds__(kProjBlock) void k_proj_blur_v_merge(ProjDev P, int nb, const double* __restrict__ tmp,
                                                                  const double* __restrict__ pre,
                                                                  const float* __restrict__ rot, double* __restrict__ blr,
                                                                  float* __restrict__ out, float* __restrict__ mask,
                                                                  float* __restrict__ image1, float* __restrict__ depth) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= P.N) return;
  const int y = q / P.W, x = q - y * P.W;
  const size_t base = (size_t)b * P.N;
  double acc[kProjMaxBlur];
  proj_blur_v(P, nb, tmp, b, x, y, acc);
  double rb[kProjMaxD], rt[kProjMaxD], m = 0.0;
#pragma unroll
  for (int c = 0; c < kProjMaxBlur; ++c) {       // static register indices only
    if (c < kProjMaxD && c < P.D) rb[c] = acc[c];
    if (c == P.D) m = acc[c];
  }
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    rt[c] = 0.0;
    if (c >= P.D || !(P.flags & kProjHasRotated)) continue;
    if (P.flags & kProjBlurRotated) {
#pragma unroll
      for (int j = 0; j < kProjMaxBlur; ++j)
        if (j == P.D + 1 + c) rt[c] = acc[j];
    } else {
      rt[c] = rot[(base + q) * P.D + c];
    }
  }
  const double dp = pre[proj_plane(P, b, 2 * P.D + 1, q)];
  double o[kProjMaxD], i1[kProjMaxD], dep;
  proj_merge_fwd(P, rb, m, dp, rt, o, i1, dep);
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    if (c >= P.D) continue;
    out[(base + q) * P.D + c] = (float)o[c];
    image1[(base + q) * P.D + c] = (float)i1[c];
    if (blr) { blr[proj_plane(P, b, c, q)] = rb[c]; blr[proj_plane(P, b, P.D + 1 + c, q)] = rt[c]; }
  }
  mask[base + q] = (float)m;
  if (depth) depth[base + q] = (float)dep;
  if (blr) { blr[proj_plane(P, b, P.D, q)] = m; blr[proj_plane(P, b, 2 * P.D + 1, q)] = dp; }
}

// Backward 1: the merge, one lane per pixel.  Upstream gradients fp32, NULL = none.  gpl: their planes.
__global__ __launch_bounds__(kProjBlock) void k_proj_merge_bwd(ProjDev P, const double* __restrict__ blr,
                                                               const float* __restrict__ g_out,
                                                               const float* __restrict__ g_mask,
                                                               const float* __restrict__ g_image1,
                                                               const float* __restrict__ g_depth,
                                                               double* __restrict__ gpl) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= P.N) return;
  const size_t o = (size_t)b * P.N + q;
  double rb[kProjMaxD], rt[kProjMaxD], go[kProjMaxD], gi[kProjMaxD];
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    const bool in = c < P.D;
    rb[c] = in ? blr[proj_plane(P, b, c, q)] : 0.0;
    rt[c] = in ? blr[proj_plane(P, b, P.D + 1 + c, q)] : 0.0;
    go[c] = in && g_out ? (double)g_out[o * P.D + c] : 0.0;
    gi[c] = in && g_image1 ? (double)g_image1[o * P.D + c] : 0.0;
  }
  double g_rb[kProjMaxD], g_rt[kProjMaxD], g_m, g_dp;
  proj_merge_bwd(P, rb, blr[proj_plane(P, b, P.D, q)], blr[proj_plane(P, b, 2 * P.D + 1, q)], rt, go, g_mask ? (double)g_mask[o] : 0.0, gi,
                 g_depth ? (double)g_depth[o] : 0.0, g_rb, g_m, g_rt, g_dp);
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    if (c >= P.D) continue;
    gpl[proj_plane(P, b, c, q)] = g_rb[c];
    gpl[proj_plane(P, b, P.D + 1 + c, q)] = g_rt[c];
  }
  gpl[proj_plane(P, b, P.D, q)] = g_m;
  gpl[proj_plane(P, b, 2 * P.D + 1, q)] = g_dp;
}

// Backward 3: the vertical half of the adjoint blur, then per corner the gradients the surfels gather: gcor (corner
// rows) = g_value[c] / dd, g_mask / dd, g_depth / dd and the gradient of the denominator, -sum_v g_v Q_v / dd (0 for an
// empty corner: its Q are 0).  g_rot (B, N, D) fp32 is the rotated image's gradient; gcor and g_rot may be NULL.
__global__ __launch_bounds__(kProjBlock) void k_proj_blur_v_corner(ProjDev P, int nb, const double* __restrict__ gtmp,
                                                                   const double* __restrict__ gpl,
                                                                   const double* __restrict__ cor,
                                                                   double* __restrict__ gcor, float* __restrict__ g_rot) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= P.N) return;
  const int y = q / P.W, x = q - y * P.W;
  const size_t base = (size_t)b * P.N;
  double acc[kProjMaxBlur];
  proj_blur_v(P, nb, gtmp, b, x, y, acc);
  double gv[kProjMaxD + 2];     // value channels, mask, depth
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) gv[c] = 0.0;
  gv[kProjMaxD] = 0.0;
#pragma unroll
  for (int c = 0; c < kProjMaxBlur; ++c) {
    if (c < kProjMaxD && c < P.D) gv[c] = acc[c];
    if (c == P.D) gv[kProjMaxD] = acc[c];
  }
  gv[kProjMaxD + 1] = gpl[proj_plane(P, b, 2 * P.D + 1, q)];
  if (g_rot) {
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c) {
      if (c >= P.D) continue;
      double r = gpl[proj_plane(P, b, P.D + 1 + c, q)];
      if (P.flags & kProjBlurRotated) {
#pragma unroll
        for (int j = 0; j < kProjMaxBlur; ++j)
          if (j == P.D + 1 + c) r = acc[j];
      }
      g_rot[(base + q) * P.D + c] = (float)r;
    }
  }
  if (!gcor) return;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const double inv = cor[proj_corner(P, b, k, P.D + 2, q)];
    double S = gv[kProjMaxD] * cor[proj_corner(P, b, k, P.D, q)] + gv[kProjMaxD + 1] * cor[proj_corner(P, b, k, P.D + 1, q)];
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c) {
      if (c >= P.D) continue;
      S += gv[c] * cor[proj_corner(P, b, k, c, q)];
      gcor[proj_corner(P, b, k, c, q)] = gv[c] * inv;
    }
    gcor[proj_corner(P, b, k, P.D, q)] = gv[kProjMaxD] * inv;
    gcor[proj_corner(P, b, k, P.D + 1, q)] = gv[kProjMaxD + 1] * inv;
    gcor[proj_corner(P, b, k, P.D + 2, q)] = -S * inv;
  }
}

// Backward 4: one lane per surfel reads the rows of its four destination pixels and writes g_rgb (B, N, D) and
// g_surfels (B, N, 3), each element once; either may be NULL.  A surfel none of whose corners can be in the frame (NaN,
// inf and huge ones among them) gets exact zeros in both, whatever its coordinates and its rgb hold.
// kView: also the gradient of the view's matrix: cc = M [p, 1], so g_M = sum_s g_cc (x) [p_s, 1] with g_cc = (g_X, g_Y,
// g_Z) below, zeros for a surfel outside the frame.  The lane keeps g_cc and the point (vg, vp), each workgroup stores
// the sums of their 12 products to view_part (srh_view_grad.h), and g_rgb and g_surfels may then both be NULL.  Without
// kView the trailing argument is unused and the code is what it was without it.
template <bool kView>
__global__ __launch_bounds__(kProjBlock) void k_proj_surfel_bwd(ProjDev P, const double* __restrict__ view,
                                                                const float* __restrict__ surfels,
                                                                const float* __restrict__ rgb,
                                                                const double* __restrict__ gcor,
                                                                float* __restrict__ g_rgb, float* __restrict__ g_surfels,
                                                                double* __restrict__ view_part) {
  const int s = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  double vg[3] = {0.0, 0.0, 0.0}, vp[3] = {0.0, 0.0, 0.0};      // kView: g_cc and the point; zeros bring zeros
  do {                                  // a lane that is done leaves by `break`: with kView every lane reaches the reduce
  if (s >= P.N) break;
  const size_t base = (size_t)b * P.N, o = base + s;
  double M[12];
  proj_load_view(view, b, M);
  const ProjSurfel S = proj_surfel(P, M, surfels + 3 * o);
  if (!S.live) {                        // zero rows before any arithmetic on S: its alpha, w, X, Y may be inf or NaN
    if (g_rgb) {
#pragma unroll
      for (int c = 0; c < kProjMaxD; ++c)
        if (c < P.D) g_rgb[o * P.D + c] = 0.0f;
    }
    if (g_surfels) {
#pragma unroll
      for (int j = 0; j < 3; ++j) g_surfels[3 * o + j] = 0.0f;
    }
    break;
  }
  const double a = S.alpha * S.w;
  double v[kProjMaxD], gc[kProjMaxD];
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    v[c] = c < P.D ? (double)rgb[o * P.D + c] : 0.0;
    gc[c] = 0.0;
  }
  double g_fx = 0.0, g_fy = 0.0, g_a = 0.0, g_zv = 0.0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int qx = S.ix + (k >> 1), qy = S.iy + (k & 1);
    if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
    const double* g = gcor + proj_corner(P, b, k, 0, qy * P.W + qx);      // slot s of the row: g[s N]
    const double beta = proj_beta(k, S.fx, S.fy);
    const double g_dep = g[(size_t)(P.D + 1) * P.N];
    double T = g[(size_t)P.D * P.N] + S.z * g_dep;
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c) {
      if (c >= P.D) continue;
      const double gvc = g[(size_t)c * P.N];
      T += v[c] * gvc;
      gc[c] += beta * a * gvc;
    }
    const double g_beta = a * T;
    g_fx += g_beta * ((k & 2) ? 1.0 : -1.0) * ((k & 1) ? S.fy : 1.0 - S.fy);
    g_fy += g_beta * ((k & 1) ? 1.0 : -1.0) * ((k & 2) ? S.fx : 1.0 - S.fx);
    g_a += beta * T + g[(size_t)(P.D + 2) * P.N];
    g_zv += beta * a * g_dep;
  }
  if (g_rgb) {
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c)
      if (c < P.D) g_rgb[o * P.D + c] = (float)gc[c];
  }
  if (!kView && !g_surfels) break;
  if (P.flags & kProjUseCenterDist) {
    const double g_alpha = g_a * S.w;
    g_fx -= g_alpha * 4.0 * S.fx * S.alpha;
    g_fy -= g_alpha * 4.0 * S.fy * S.alpha;
  }
  double g_z = 0.0;
  if (!(P.flags & kProjDetachDepthMerge)) {
    g_z = g_zv;
    if (P.flags & kProjUseDepth) g_z -= g_a * S.alpha * 2.0 * S.w;
  }
  const double g_X = g_fx * P.fsx / S.Zd, g_Y = g_fy * P.fsy / S.Zd;
  const double g_Z = (S.Z != 0.0 ? -(g_X * S.X + g_Y * S.Y) / S.Zd : 0.0) - g_z;
  if (kView) {
    vg[0] = g_X; vg[1] = g_Y; vg[2] = g_Z;
#pragma unroll
    for (int c = 0; c < 3; ++c) vp[c] = (double)surfels[3 * o + c];
  }
  if (kView && !g_surfels) break;
#pragma unroll
  for (int j = 0; j < 3; ++j) g_surfels[3 * o + j] = (float)((M[j] * g_X + M[4 + j] * g_Y) + M[8 + j] * g_Z);
  } while (false);
  if (kView) view_block_reduce<kViewSums>([&](int k) { return view_outer_term(vg, vp, k); }, view_part);
}
}  // namespace srh
