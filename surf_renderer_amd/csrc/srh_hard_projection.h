// The reference's hard scatter-mean projection, projection_renderer (diffrend/torch/projection_layer.py:88-106 with
// project_image_coordinates :45-85 and scatter_mean_dim0 torch/utils.py:146-175), forward and backward, restated as a
// gather; many views per launch (the view is grid dimension y).  See DESIGN.md "The depth lift and the hard projection".
//
// Per view, N = W H surfels (world position p, D-channel value v):
//   (u, v) = proj_point's (srh_projection.h): the reference's pixel coordinate minus 1/2, with Z = 0 divided by 1 and a
//            surfel behind the camera projected like any other
//   pixel  = (rint u, rint v), ties to even (torch.round); a surfel whose pixel is outside the frame, is NaN or fits no
//            int is dropped
//   out[q] = (sum of v over the surfels of pixel q, in ascending surfel index) / count[q], 0 where count[q] = 0
//   mask[q] = count[q] == 0                         TRUE WHERE NOTHING LANDED -- the reference's sense
// Backward: g_rgb[s] = g_out[q(s)] / count[q(s)], 0 for a dropped surfel.  The surfels get no gradient.
//
// k_hproj_keys (one lane per surfel: pixel index, N for a dropped surfel) -> the caller orders the keys (stable,
// ascending) -> k_hproj_gather (one lane per pixel finds its run in the ordered keys by binary search and sums it) and
// k_hproj_bwd (one lane per surfel).  fp64 sums, fp32 results, no atomic, every element written once: values and
// gradients are identical from run to run.
#pragma once
#include "srh_projection.h"

namespace srh {

struct HProjDev {
  int B, W, H, N, D, nblk;
  double fsx, fsy, cx0, cy0;
};

// The pixel index of a surfel at (u, v), `dump` for a dropped one.  The one copy of this arithmetic: k_project_fwd
// (srh_frames.h) takes project_image_coordinates' index from it, so the two agree bit for bit.
__device__ __forceinline__ int32_t hproj_key(int W, int H, int dump, double u, double v) {
  const double ru = rint(u), rv = rint(v);
  // NaN and anything an int cannot hold fail these comparisons
  const bool in = ru >= 0.0 && ru <= (double)(W - 1) && rv >= 0.0 && rv <= (double)(H - 1);
  return in ? (int)rv * W + (int)ru : dump;
}

// one lane per surfel: keys (B, N) int32
__global__ __launch_bounds__(kProjBlock) void k_hproj_keys(HProjDev P, const double* __restrict__ view,
                                                           const float* __restrict__ surfels,
                                                           int32_t* __restrict__ keys) {
  const int s = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= P.N) return;
  const size_t o = (size_t)b * P.N + s;
  double M[12];
  proj_load_view(view, b, M);
  const ProjPoint S = proj_point(P.fsx, P.fsy, P.cx0, P.cy0, P.W, P.H, M, surfels + 3 * o);
  keys[o] = hproj_key(P.W, P.H, P.N, S.u, S.v);
}

// One lane per pixel q.  order (B, N): per view a stable ascending permutation of the keys; an entry outside 0..N-1
// counts as dropped in the search and is skipped in the walk.  out (B, N, D) fp32, mask (B, N) bytes, count (B, N) int32.
__global__ __launch_bounds__(kProjBlock) void k_hproj_gather(HProjDev P, const int32_t* __restrict__ keys,
                                                             const int32_t* __restrict__ order,
                                                             const float* __restrict__ rgb, float* __restrict__ out,
                                                             uint8_t* __restrict__ mask, int32_t* __restrict__ count) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= P.N) return;
  const size_t base = (size_t)b * P.N;
  int lo = 0, hi = P.N;                 // the first position whose key is >= q
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int32_t s = order[base + mid];
    const int32_t k = (uint32_t)s < (uint32_t)P.N ? keys[base + s] : P.N;
    if (k < q) lo = mid + 1;
    else hi = mid;
  }
  double acc[kProjMaxD];
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) acc[c] = 0.0;
  int n = 0;
  for (int i = lo; i < P.N; ++i) {
    const int32_t s = order[base + i];
    if ((uint32_t)s >= (uint32_t)P.N) continue;
    if (keys[base + s] != q) break;
    const float* v = rgb + (base + s) * P.D;
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c)
      if (c < P.D) acc[c] += (double)v[c];
    ++n;
  }
  const double den = n > 0 ? (double)n : 1.0;
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c)
    if (c < P.D) out[(base + q) * P.D + c] = (float)(acc[c] / den);
  mask[base + q] = n == 0 ? 1 : 0;
  count[base + q] = n;
}

// one lane per surfel: g_rgb (B, N, D) fp32, every element written
__global__ __launch_bounds__(kProjBlock) void k_hproj_bwd(HProjDev P, const int32_t* __restrict__ keys,
                                                          const int32_t* __restrict__ count,
                                                          const float* __restrict__ g_out, float* __restrict__ g_rgb) {
  const int s = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= P.N) return;
  const size_t base = (size_t)b * P.N;
  const int32_t q = keys[base + s];
  const bool landed = (uint32_t)q < (uint32_t)P.N;
  const int32_t n = landed ? count[base + q] : 0;
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    if (c >= P.D) continue;
    g_rgb[(base + s) * P.D + c] = n > 0 ? (float)((double)g_out[(base + q) * P.D + c] / (double)n) : 0.0f;
  }
}
}  // namespace srh
