// The reference's dense Gaussian re-projection, projection_renderer_differentiable (diffrend/torch/projection_layer.py:
// 108-152 with project_image_coordinates :45-85), forward and analytic backward; many views per launch (the view is
// grid dimension y).  See DESIGN.md "The dense Gaussian re-projection layer".
//
// Per view, N = W H surfels (world position p, D-channel value c) and P = W H pixels (i, j):
//   (u, v) = proj_point(p)                        the pixel coordinate less 1/2, so pixel centre (i + 1/2, j + 1/2) is (i, j)
//   s[p, n] = ex[n, i] ey[n, j],  ex[n, i] = exp(-(u_n - i)^2 / (2 sigma^2)),  ey[n, j] = exp(-(v_n - j)^2 / (2 sigma^2))
//   m[p] = sum_n s[p, n],  S[p, d] = sum_n s[p, n] c[n, d]                    every surfel counts, in ascending n
//   out = S / (m + 1e-10)  without a rotated image,  S + rot (1 - m)  with one;  mask = m
// The reference forms s as a (B, P, N) tensor and s c as (B, P, N, D); here no buffer grows with P N.
//
// Forward: k_dproj_uv (one lane per surfel: u, v) -> k_dproj_fwd<D> (one workgroup per tile of kDProjTile^2 pixels streams
// the view's surfels in chunks of kDProjChunk: per chunk it fills LDS with ex for the tile's columns, ey for its rows and
// the values as fp64 -- six exp per surfel and tile, the rest by recurrence -- and every lane adds the chunk to the
// D + 1 fp64 sums of its eight pixels).  Backward: k_dproj_pixel_bwd (per pixel: the effective upstream row
// gt[p, 0..D] and the rotated image's gradient) -> k_dproj_surfel_bwd<D, POS, kView> (one lane per surfel sweeps the frame in strips of kDProjStrip columns,
// ex of the strip in registers, one exp per row and strip; gt is the same for every lane: scalar loads) with the chain
// rule through the projection.  fp64 arithmetic, fp32 results, no atomic, every sum in a fixed order, every output
// element written once: values and gradients are identical from run to run, and a batch equals its views.
#pragma once
#include "srh_device.h"       // as_constant
#include "srh_projection.h"   // proj_point, proj_load_view, kProjMaxD

namespace srh {

constexpr int kDProjBlock = 256;      // the per-surfel and per-pixel kernels
constexpr int kDProjTile = 32;        // k_dproj_fwd: a tile is kDProjTile x kDProjTile pixels
constexpr int kDProjFwdBlock = 128;   //   lane t: columns t % 16 + {0, 16}, rows t / 16 + {0, 8, 16, 24}
constexpr int kDProjChunk = 64;       //   surfels per LDS fill
constexpr int kDProjStrip = 16;       // k_dproj_surfel_bwd: columns whose ex a lane keeps in registers
constexpr int kDProjBwdBlock = 64;    //   one wave: no LDS, no barrier

constexpr int kDProjHasRotated = 1;

struct DProjDev {
  int B, W, H, N, D, flags;
  int Wp;                             // W rounded up to whole strips: the row pitch of gt
  double fsx, fsy, cx0, cy0;          // u = fsx X / Z + cx0, v = fsy Y / Z + cy0
  double h, q;                        // 1 / (2 sigma^2), exp(-1 / sigma^2)
};

// saved (B, D + 1, P) fp64: S of the D channels, then m.  gt (B, H, Wp, D + 1) fp64, channel fastest, zero in the
// padding columns: a strip of one row is one contiguous run.
__host__ __device__ __forceinline__ size_t dproj_saved(const DProjDev& P, int b, int ch, int q) {
  return ((size_t)b * (P.D + 1) + ch) * P.N + q;
}

// Forward 1: one lane per surfel; uv (B, N, 2) fp64
__global__ __launch_bounds__(kDProjBlock) void k_dproj_uv(DProjDev P, const double* __restrict__ view,
                                                          const float* __restrict__ surfels, double* __restrict__ uv) {
  const int s = blockIdx.x * kDProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= P.N) return;
  const size_t o = (size_t)b * P.N + s;
  double M[12];
  proj_load_view(view, b, M);
  const ProjPoint Q = proj_point(P.fsx, P.fsy, P.cx0, P.cy0, P.W, P.H, M, surfels + 3 * o);
  uv[2 * o] = Q.u;
  uv[2 * o + 1] = Q.v;
}

// Forward 2: blockIdx.x = the tile (row-major over ceil(W / T) x ceil(H / T)), blockIdx.y = the view.
template <int D>
__global__ __launch_bounds__(kDProjFwdBlock) void k_dproj_fwd(DProjDev P, const double* __restrict__ uv,
                                                              const float* __restrict__ rgb, const float* __restrict__ rot,
                                                              double* __restrict__ saved, float* __restrict__ out,
                                                              float* __restrict__ mask) {
  constexpr int T = kDProjTile, C = kDProjChunk;
  __shared__ double e[C][2 * T + 1];  // ex of the tile's columns, then ey of its rows; padded: a lane fills a row
  __shared__ double val[C][D];
  const int t = threadIdx.x, b = blockIdx.y;
  const int tiles_x = (P.W + T - 1) / T;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int cx = t & 15, ry = t >> 4;
  const size_t base = (size_t)b * P.N;
  double m[2][4], S[2][4][D];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[a][r] = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) S[a][r][d] = 0.0;
    }
  // the fill: wave 0 makes ex, wave 1 ey, lane = the surfel of the chunk
  const int axis = t >> 6, ln = t & 63;
  const double origin = axis ? (double)(ty * T) : (double)(tx * T);
  for (int n0 = 0; n0 < P.N; n0 += C) {
    const int cn = min(C, P.N - n0);
    if (ln < cn) {
      // The T values of one surfel and axis from three exp: exact at the tile's column nearest the surfel, then outwards
      // by e[i +- 1] = e[i] r, r <- r q with q = exp(-1 / sigma^2).  Every factor used is <= 1: the values only decay
      // away from the centre, so nothing overflows and what underflows is negligible in exact arithmetic too.
      const double p = uv[2 * (base + n0 + ln) + axis] - origin;
      const double cf = fmin(fmax(rint(p), 0.0), (double)(T - 1));
      const int c = (int)cf;
      const double d = cf - p;
      double eu = exp(-(d * d) * P.h), ed = eu;
      double ru = exp(-(2.0 * d + 1.0) * P.h), rd = exp((2.0 * d - 1.0) * P.h);
      double* row = &e[ln][axis * T];
      row[c] = eu;
      for (int k = 1; k < T; ++k) {
        eu *= ru; ru *= P.q;
        ed *= rd; rd *= P.q;
        if (c + k < T) row[c + k] = eu;
        if (c - k >= 0) row[c - k] = ed;
      }
    }
    for (int i = t; i < cn * D; i += kDProjFwdBlock) val[i / D][i % D] = (double)rgb[(base + n0) * D + i];
    __syncthreads();
#pragma unroll 2
    for (int n = 0; n < cn; ++n) {
      const double ex[2] = {e[n][cx], e[n][cx + 16]};
      double c[D];
#pragma unroll
      for (int d = 0; d < D; ++d) c[d] = val[n][d];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double ey = e[n][T + ry + 8 * r];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const double s = ex[a] * ey;
          m[a][r] += s;
#pragma unroll
          for (int d = 0; d < D; ++d) S[a][r][d] = __builtin_fma(s, c[d], S[a][r][d]);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = tx * T + cx + 16 * a, y = ty * T + ry + 8 * r;
      if (x >= P.W || y >= P.H) continue;
      const int q = y * P.W + x;
      const double mm = m[a][r];
      mask[base + q] = (float)mm;
      if (saved) saved[dproj_saved(P, b, D, q)] = mm;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double Sd = S[a][r][d];
        const double o = (P.flags & kDProjHasRotated) ? Sd + (double)rot[(base + q) * D + d] * (1.0 - mm)
                                                      : Sd / (mm + 1.0e-10);
        out[(base + q) * D + d] = (float)o;
        if (saved) saved[dproj_saved(P, b, d, q)] = Sd;
      }
    }
}

// Backward 1: one lane per slot of the padded frame (H x Wp).  gt[p, d] = d loss / d S[p, d], gt[p, D] = d loss / d m[p];
// g_rot (B, N, D) fp32 is the rotated image's gradient (NULL = not wanted); g_out, g_mask fp32, NULL = none.
__global__ __launch_bounds__(kDProjBlock) void k_dproj_pixel_bwd(DProjDev P, const double* __restrict__ saved,
                                                                 const float* __restrict__ rot,
                                                                 const float* __restrict__ g_out,
                                                                 const float* __restrict__ g_mask, double* __restrict__ gt,
                                                                 float* __restrict__ g_rot) {
  const int e = blockIdx.x * kDProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (e >= P.H * P.Wp) return;
  const int y = e / P.Wp, x = e - y * P.Wp;
  double* g = gt + ((size_t)b * P.H * P.Wp + e) * (P.D + 1);
  if (x >= P.W) {
    for (int d = 0; d <= P.D; ++d) g[d] = 0.0;
    return;
  }
  const int q = y * P.W + x;
  const size_t o = (size_t)b * P.N + q;
  const double mm = saved[dproj_saved(P, b, P.D, q)];
  const double inv = 1.0 / (mm + 1.0e-10);
  double gm = g_mask ? (double)g_mask[o] : 0.0;
  for (int d = 0; d < P.D; ++d) {
    const double go = g_out ? (double)g_out[o * P.D + d] : 0.0;
    if (P.flags & kDProjHasRotated) {
      g[d] = go;
      gm -= go * (double)rot[o * P.D + d];
      if (g_rot) g_rot[o * P.D + d] = (float)(go * (1.0 - mm));
    } else {
      g[d] = go * inv;
      gm -= (go * saved[dproj_saved(P, b, d, q)]) * (inv * inv);
    }
  }
  g[P.D] = gm;
}

// Backward 2: one lane per surfel.  With R_c[j] = sum_i gt[(i, j), c] ex[i] and Rx_c[j] = sum_i gt[(i, j), c] ex[i] (i - u)
// over a strip's columns, and c_D = 1:
//   g_rgb[d] = sum_j ey[j] R_d[j]
//   g_u = sum_j ey[j] sum_c c_c Rx_c[j] / sigma^2,  g_v = sum_j ey[j] (j - v) sum_c c_c R_c[j] / sigma^2
// summed over the strips in ascending order.  POS: grad_surfels is wanted (else the Rx sums are not formed).  g_rgb
// (B, N, D) and g_surfels (B, N, 3) are written, each element once; g_rgb may be NULL.
// kView (with POS: it needs the Rx sums): also the gradient of the view's matrix: cc = M [p, 1], so g_M = sum_s g_cc (x)
// [p_s, 1] with g_cc = (g_X, g_Y, g_Z) below -- every surfel counts, and one at Z = 0 brings (g_X, g_Y, 0) as its
// g_surfels does.  The lane keeps g_cc and re-reads its point (vg, vp); a lane past N stays for the butterfly and brings
// zeros; each workgroup -- one wave -- stores the sums of the 12 products to view_part (view_wave_reduce,
// srh_view_grad.h), and g_rgb and g_surfels may then both be NULL.  Without kView the trailing argument is unused and
// the code is what it was without it.
template <int D, bool POS, bool kView>
__global__ __launch_bounds__(kDProjBwdBlock) void k_dproj_surfel_bwd(DProjDev P, const double* __restrict__ view,
                                                                     const float* __restrict__ surfels,
                                                                     const float* __restrict__ rgb,
                                                                     const double* __restrict__ gt,
                                                                     float* __restrict__ g_rgb,
                                                                     float* __restrict__ g_surfels,
                                                                     double* __restrict__ view_part) {
  static_assert(POS || !kView, "the view's gradient needs the Rx sums");
  constexpr int K = kDProjStrip, CH = D + 1;
  const int b = blockIdx.y;
  // a lane past the end repeats the last surfel and stores nothing: the loops below stay uniform
  const int s = min((int)(blockIdx.x * kDProjBwdBlock + threadIdx.x), P.N - 1);
  const bool live = blockIdx.x * kDProjBwdBlock + threadIdx.x < (unsigned)P.N;
  const size_t o = (size_t)b * P.N + s;
  double M[12];
  proj_load_view(view, b, M);
  const ProjPoint Q = proj_point(P.fsx, P.fsy, P.cx0, P.cy0, P.W, P.H, M, surfels + 3 * o);
  double c[CH];
#pragma unroll
  for (int d = 0; d < D; ++d) c[d] = (double)rgb[o * D + d];
  c[D] = 1.0;
  double gc[D], gu = 0.0, gv = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) gc[d] = 0.0;
  // the same rows for every lane, written by k_dproj_pixel_bwd before this launch
  const auto g_view = as_constant(gt) + (size_t)b * P.H * P.Wp * CH;
  for (int i0 = 0; i0 < P.Wp; i0 += K) {
    double ex[K], exd[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double d = (double)(i0 + k) - Q.u;
      ex[k] = exp(-(d * d) * P.h);
      if (POS) exd[k] = ex[k] * d;
    }
    for (int j = 0; j < P.H; ++j) {
      const auto g = g_view + ((size_t)j * P.Wp + i0) * CH;
      double R[CH], Rx[CH];
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) R[ch] = Rx[ch] = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
          const double gk = g[k * CH + ch];
          R[ch] = __builtin_fma(gk, ex[k], R[ch]);
          if (POS) Rx[ch] = __builtin_fma(gk, exd[k], Rx[ch]);
        }
      const double dy = (double)j - Q.v;
      const double ey = exp(-(dy * dy) * P.h);
#pragma unroll
      for (int d = 0; d < D; ++d) gc[d] = __builtin_fma(ey, R[d], gc[d]);
      if (POS) {
        double A = Rx[D], Bv = R[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
          A = __builtin_fma(c[d], Rx[d], A);
          Bv = __builtin_fma(c[d], R[d], Bv);
        }
        gu = __builtin_fma(ey, A, gu);
        gv = __builtin_fma(ey * dy, Bv, gv);
      }
    }
  }
  double vg[3] = {0.0, 0.0, 0.0}, vp[3] = {0.0, 0.0, 0.0};      // kView: g_cc and the point; zeros bring zeros
  do {                                  // a lane that is done leaves by `break`: with kView every lane reaches the reduce
  if (!live) break;
  if (g_rgb) {
#pragma unroll
    for (int d = 0; d < D; ++d) g_rgb[o * D + d] = (float)gc[d];
  }
  if (!POS) break;
  gu *= 2.0 * P.h;
  gv *= 2.0 * P.h;
  const double g_X = gu * P.fsx / Q.Zd, g_Y = gv * P.fsy / Q.Zd;
  const double g_Z = Q.Z != 0.0 ? -(g_X * Q.X + g_Y * Q.Y) / Q.Zd : 0.0;
  if (kView) {
    vg[0] = g_X; vg[1] = g_Y; vg[2] = g_Z;
#pragma unroll
    for (int c = 0; c < 3; ++c) vp[c] = (double)surfels[3 * o + c];
    if (!g_surfels) break;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) g_surfels[3 * o + j] = (float)((M[j] * g_X + M[4 + j] * g_Y) + M[8 + j] * g_Z);
  } while (false);
  if (kView) view_wave_reduce<kViewSums>([&](int k) { return view_outer_term(vg, vp, k); }, view_part);
}
}  // namespace srh
