// The all-pairs render kernels (gfx950): every pixel against every primitive, no tile bins.
//
//   k_rays          generate_rays as an output
//   k_render_exact  every (pixel, primitive) pair through the fp64 intersection: the checker of the other modes
//   k_render_ortho  the same for the torch backend's orthographic projection
//   k_render_fast   fp32 screen-space reject per pair, fp64 confirmation of the survivors
// One 256-thread workgroup per 64x4-pixel tile; every wave owns 64 consecutive pixels of one image row, so depth /
// nearest / RGB stores are full-wave coalesced rows.  The primitive stream is wave-uniform (every lane walks the same
// record), so records arrive through the scalar cache into SGPRs; no LDS staging is needed for uniform reads.
#pragma once
#include "srh_device.h"

namespace srh {

// ------------------------------------------------------------------------------------------------
// k_rays: generate_rays as an output (reference returns 'ray_dir' (4,N))
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rays(FrameDev F, float* ray_dir) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int r = F.row0 + blockIdx.y * 4 + threadIdx.y;
  if (c >= F.W || r >= F.row1) return;
  double d[3];
  pixel_ray(F, c, r, d);
  const size_t n = (size_t)(F.row1 - F.row0) * F.W;
  const size_t p = (size_t)(r - F.row0) * F.W + c;
  ray_dir[p] = (float)d[0];
  ray_dir[n + p] = (float)d[1];
  ray_dir[2 * n + p] = (float)d[2];
  ray_dir[3 * n + p] = 0.0f;
}

// ------------------------------------------------------------------------------------------------
// k_render_exact: every (pixel, primitive) pair through the fp64 intersection
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_pixel(const FrameDev& F, int c, int r, const float rgb[3], double z, int win,
                                            float* __restrict__ image, float* __restrict__ depth,
                                            int32_t* __restrict__ nearest, const float* aux = nullptr) {
  const size_t row = (size_t)(r - F.row0);
  float* px = image + row * F.img_stride + 3 * (size_t)c;
  px[0] = rgb[0];
  px[1] = rgb[1];
  px[2] = rgb[2];
  depth[row * F.depth_stride + c] = background_depth(F, z);
  if (nearest) nearest[row * F.near_stride + c] = win;
  if (aux) store_aux(F, row, c, aux);
}

__global__ __launch_bounds__(256) void k_render_exact(FrameDev F, float* __restrict__ image,
                                                       float* __restrict__ depth, int32_t* __restrict__ nearest) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int r = F.row0 + blockIdx.y * 4 + threadIdx.y;
  const bool live = (c < F.W) && (r < F.row1);
  double d[3];
  pixel_ray(F, live ? c : F.W - 1, live ? r : F.row1 - 1, d);

  double best = __builtin_inf();
  int besti = 0;
  for (int s = 0; s < F.nseg; ++s) {
    const SegDev& S = F.seg[s];
    const int stride = kRec64Stride[S.type];
    for (int i = 0; i < S.count; ++i) {
      const double t = hit_any64(S.type, S.rec64 + (size_t)i * stride, F.o, d, F.shading != 0);
      resolve(F, t, S.first + i, best, besti);
    }
  }
  float rgb[3], aux[6];
  const bool want_aux = F.normal_out || F.pos_out;
  shade_pixel(F, d, best, besti, rgb, want_aux ? aux : nullptr);
  if (live) store_pixel(F, c, r, rgb, best, besti, image, depth, nearest, want_aux ? aux : nullptr);
}

// ------------------------------------------------------------------------------------------------
// k_render_ortho: orthographic projection of the torch backend (torch/utils.py:461-468): every ray has the direction
// -z of the camera basis and its own origin eye + x X + y Y.  All pairs in fp64 (the screen-space reject records are
// derived for a pinhole); the reference's own ortho branch only works for images below one 4096-pixel tile.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_render_ortho(FrameDev F, float* __restrict__ image,
                                                       float* __restrict__ depth, int32_t* __restrict__ nearest) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int r = F.row0 + blockIdx.y * 4 + threadIdx.y;
  const bool live = (c < F.W) && (r < F.row1);
  double q[3], org[3], d[3];
  ortho_ray(F, live ? c : F.W - 1, live ? r : F.row1 - 1, q, d);
#pragma unroll
  for (int i = 0; i < 3; ++i) org[i] = F.o[i] + q[i];
  double best = __builtin_inf();
  int besti = 0;
  for (int s = 0; s < F.nseg; ++s) {
    const SegDev& S = F.seg[s];
    const int stride = kRec64Stride[S.type];
    for (int i = 0; i < S.count; ++i)
      resolve(F, hit_any64_from(S.type, S.rec64 + (size_t)i * stride, F.o, q, d), S.first + i, best, besti);
  }
  float rgb[3], aux[6];
  const bool want_aux = F.normal_out || F.pos_out;
  shade_pixel_t<true>(F, d, best, besti, rgb, want_aux ? aux : nullptr, nullptr, org);
  if (live) store_pixel(F, c, r, rgb, best, besti, image, depth, nearest, want_aux ? aux : nullptr);
}

// ------------------------------------------------------------------------------------------------
// k_render_fast<P>: fp32 screen-space reject per pair, fp64 confirmation of the survivors.
// A wave owns 64*P consecutive pixels of one row: lane l holds columns c0 + l + 64*j, j < P.  Reject
// records are wave-uniform reads (scalar loads); the survivor branch is entered by a wave only when one
// of its 64*P pixels passes the reject test, which for small primitives is a fraction of a percent of
// the primitives, so the loop is bound by ~3 VALU operations per pair.
// ------------------------------------------------------------------------------------------------
template <int P>
__device__ __forceinline__ void confirm(const FrameDev& F, const SegDev& S, int i, int r, int cbase,
                                        const float (&q)[P], bool ge_zero, double (&best)[P], int (&besti)[P]) {
  const double* R = S.rec64 + (size_t)i * kRec64Stride[S.type];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const bool cand = ge_zero ? (q[j] >= 0.0f) : (q[j] <= 0.0f);
    const int c = cbase + 64 * j;
    if (cand && c < F.W) {
      double d[3];
      pixel_ray(F, c, r, d);
      resolve(F, hit_any64(S.type, R, F.o, d, F.shading != 0), S.first + i, best[j], besti[j]);
    }
  }
}

template <int P>
__global__ __launch_bounds__(256) void k_render_fast(FrameDev F, float* __restrict__ image,
                                                      float* __restrict__ depth, int32_t* __restrict__ nearest) {
  const int cbase = blockIdx.x * (64 * P) + threadIdx.x;
  const int r_raw = F.row0 + blockIdx.y * 4 + threadIdx.y;
  const bool row_live = r_raw < F.row1;
  const int r = row_live ? r_raw : F.row1 - 1;
  const float rf = (float)r;
  float cf[P];
  double best[P];
  int besti[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    cf[j] = (float)(cbase + 64 * j);
    best[j] = __builtin_inf();
    besti[j] = 0;
  }

  for (int s = 0; s < F.nseg; ++s) {
    const SegDev& S = F.seg[s];
    if (S.type == SRH_PRIM_DISK || S.type == SRH_PRIM_SPHERE) {
      for (int i = 0; i < S.count; ++i) {
        const float* Q = S.rec32 + (size_t)i * kRec32Stride[SRH_PRIM_DISK];
        const float dr = rf - Q[1];
        float q[P];
        float m = __builtin_inff();
        {
          const float e = Q[3] * dr;
          const float g = __builtin_fmaf(Q[4] * dr, dr, -1.0f);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const float dc = cf[j] - Q[0];
            q[j] = __builtin_fmaf(dc, __builtin_fmaf(Q[2], dc, e), g);
            m = fminf(m, q[j]);
          }
        }
        if (m <= 0.0f) confirm<P>(F, S, i, r, cbase, q, false, best, besti);
      }
    } else if (S.type == SRH_PRIM_TRIANGLE) {
      for (int i = 0; i < S.count; ++i) {
        const float* Q = S.rec32 + (size_t)i * kRec32Stride[SRH_PRIM_TRIANGLE];
        const float r0 = __builtin_fmaf(Q[1], rf, Q[2]);
        const float r1 = __builtin_fmaf(Q[5], rf, Q[6]);
        const float r2 = __builtin_fmaf(Q[9], rf, Q[10]);
        float q[P];
        float m = -__builtin_inff();
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const float e0 = __builtin_fmaf(Q[0], cf[j], r0);
          const float e1 = __builtin_fmaf(Q[4], cf[j], r1);
          const float e2 = __builtin_fmaf(Q[8], cf[j], r2);
          q[j] = fminf(fminf(e0, e1), e2);
          m = fmaxf(m, q[j]);
        }
        if (m >= 0.0f) confirm<P>(F, S, i, r, cbase, q, true, best, besti);
      }
    } else {
      float q[P];
#pragma unroll
      for (int j = 0; j < P; ++j) q[j] = 0.0f;
      for (int i = 0; i < S.count; ++i) confirm<P>(F, S, i, r, cbase, q, false, best, besti);
    }
  }

#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int c = cbase + 64 * j;
    if (c < F.W) {      // wave-divergent only in the last column block
      double d[3];
      pixel_ray(F, c, r, d);
      float rgb[3], aux[6];
      const bool want_aux = F.normal_out || F.pos_out;
      shade_pixel(F, d, best[j], besti[j], rgb, want_aux ? aux : nullptr);
      if (row_live) store_pixel(F, c, r_raw, rgb, best[j], besti[j], image, depth, nearest, want_aux ? aux : nullptr);
    }
  }
}

}  // namespace srh
