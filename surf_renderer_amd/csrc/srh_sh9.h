// Order-2 spherical-harmonic (SH9) environment lighting: the reference's radiance_SH9 and irradiance
// (diffrend/numpy/sph.py:46-138) for B views per launch, forward and backward.  See DESIGN.md "SH9 environment lighting".
//
// Projection, per view envmap (H, W, C) fp32 -> L (C, 9) fp32.  Pixel (i, j), with the reference's swapped scales kept:
//   v = (W/2 - i) / (W/2),  u = (j - H/2) / (H/2),  r = sqrt(u^2 + v^2),  inside = r <= 1,  theta = pi r
//   domega = (2 pi / W) (2 pi / H) sinc(theta),  sinc(x) = sin(pi x) / (pi x), 1 at 0     (numpy's normalised sinc)
//   X = cos(phi) sin(theta), Y = sin(phi) sin(theta), Z = cos(theta),  cos(phi) = u / r, sin(phi) = v / r (1, 0 at r = 0)
//   L[c][k] = sum over the pixels inside of (envmap[i][j][c] Y_k(X, Y, Z)) domega
// A pixel outside the disc is NOT READ (the reference multiplies it by 0, so a NaN there poisons its channel).
//   k_sh9_project      one pixel per lane; the nine products of a channel go through view_block_reduce<9> to
//                      part[c][b][workgroup][9]; lanes past H W or outside the disc bring zeros.
//   k_sh9_finish       one workgroup per (channel, view) adds the partials in k_view_finish's order -- row j of
//                      kViewRows takes the workgroups j, j + kViewRows, ... ascending, then the rows are halved through
//                      LDS -- which depends on the number of workgroups alone, and stores out[b][c][K] once.
//   k_sh9_project_bwd  grad_env[b][i][j][c] = domega sum_k Y_k gL[b][c][k] inside, exactly 0 outside; no reduction.
//
// Irradiance, per view M (4, 4, C) fp32 (one per view, or one shared) and normal (N, 3) fp32 -> E (N, C) fp32:
//   E_c = [n, 1]^T M_c [n, 1], as a = n M[:3, :] + M[3, :], E = a[:3] . n + a[3]; any M, n not normalised.
//   k_sh9_irradiance_fwd  one normal per lane, M through scalar loads.
//   k_sh9_irradiance_bwd  grad_normal = sum_c gE_c ((M33_c + M33_c^T) n + M_c[:3, 3] + M_c[3, :3]) per lane; with kGradM
//                         also the ten distinct monomials h_r h_s of h = [n, 1] times gE_c through view_block_reduce<10>.
//   k_sh9_spread_M        the finished monomial sums (B, C, 10) -> grad_M (4, 4, C) fp64 per view, M[r][s] and M[s][r]
//                         getting the same sum; a shared M gets the views' sums added in ascending view order.
// fp64 arithmetic on the fp32 inputs, no atomic, every output element written once: results are identical from run to
// run, and a view of a batch gets the bits of the same view alone (the view is grid dimension y).
#pragma once
#include "srh_device.h"       // as_constant
#include "srh_view_grad.h"    // view_block_reduce, kViewRows

namespace srh {

constexpr int kSh9Block = kViewBlock;
constexpr int kSh9MaxC = 4;
constexpr int kSh9Coeffs = 9;
constexpr int kSh9Monomials = 10;                 // h_r h_s, r <= s, of h = [n, 1]
constexpr int kSh9SpreadBlock = 64;
static_assert(kSh9Monomials <= kViewSums, "view_block_reduce holds at most kViewSums sums");

struct Sh9Dev {
  int B, H, W, N, C, m_per_view;
};

constexpr double kSh9Pi = 3.14159265358979323846;

// The nine real harmonics in the reference's order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), in
// its order of operations (RealSH9_cart).  The constants are what numpy's sqrt(1 / pi) etc. round to.
__device__ __forceinline__ void sh9_basis(double X, double Y, double Z, double (&S)[kSh9Coeffs]) {
  const double s1 = 0.5 * sqrt(1.0 / kSh9Pi), s3 = 0.5 * sqrt(3.0 / kSh9Pi), s15 = 0.5 * sqrt(15.0 / kSh9Pi);
  const double q5 = 0.25 * sqrt(5.0 / kSh9Pi), q15 = 0.25 * sqrt(15.0 / kSh9Pi);
  S[0] = s1;
  S[1] = s3 * Y;
  S[2] = s3 * Z;
  S[3] = s3 * X;
  S[4] = s15 * X * Y;
  S[5] = s15 * Y * Z;
  S[6] = q5 * (3.0 * (Z * Z) - 1.0);
  S[7] = s15 * X * Z;
  S[8] = q15 * (X * X - Y * Y);
}

// Pixel p = i W + j of an (H, W) probe: whether it lies inside the disc, and then its harmonics and solid angle.
__device__ __forceinline__ bool sh9_pixel(int H, int W, int p, double (&S)[kSh9Coeffs], double& domega) {
  const int i = p / W, j = p - i * W;
  const double hw = 0.5 * (double)W, hh = 0.5 * (double)H;
  const double v = (hw - (double)i) / hw, u = ((double)j - hh) / hh;
  const double r = sqrt(u * u + v * v);
  if (!(r <= 1.0)) return false;
  const double theta = kSh9Pi * r, y = kSh9Pi * theta;
  const double sinc = r == 0.0 ? 1.0 : sin(y) / y;
  domega = ((2.0 * kSh9Pi / (double)W) * (2.0 * kSh9Pi / (double)H)) * sinc;
  const double st = sin(theta), ct = cos(theta);
  const double cp = r == 0.0 ? 1.0 : u / r, sp = r == 0.0 ? 0.0 : v / r;
  sh9_basis(cp * st, sp * st, ct, S);
  return true;
}

// grid (ceil(H W / 256), B).  part (C, B, gridDim.x, 9) fp64, every element written.
template <int C>
__global__ __launch_bounds__(kSh9Block) void k_sh9_project(Sh9Dev P, const float* __restrict__ env,
                                                           double* __restrict__ part) {
  const int b = blockIdx.y, p = blockIdx.x * kSh9Block + threadIdx.x, HW = P.H * P.W;
  double S[kSh9Coeffs], domega = 0.0, e[C];
#pragma unroll
  for (int k = 0; k < kSh9Coeffs; ++k) S[k] = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) e[c] = 0.0;
  const bool inside = p < HW && sh9_pixel(P.H, P.W, p, S, domega);
  if (inside) {
    const float* px = env + ((size_t)b * HW + p) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = (double)px[c];
  }
  const size_t per_channel = (size_t)gridDim.y * gridDim.x * kSh9Coeffs;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (c) __syncthreads();             // the reduce's LDS is one array for every channel
    view_block_reduce<kSh9Coeffs>([&](int k) { return inside ? (e[c] * S[k]) * domega : 0.0; },
                                  part + c * per_channel);
  }
}

// part (C, B, ngroups, K) fp64 -> out (B, C, K), every element written.  grid (C, B), block kViewRows * kViewSums.
template <class Out>
__global__ __launch_bounds__(kViewRows * kViewSums) void k_sh9_finish(int ngroups, int K,
                                                                      const double* __restrict__ part,
                                                                      Out* __restrict__ out) {
  __shared__ double rows[kViewRows][kViewSums];
  const int c = blockIdx.x, b = blockIdx.y;
  const int j = threadIdx.x / kViewSums, k = threadIdx.x % kViewSums;
  const double* p = part + ((size_t)c * gridDim.y + b) * ngroups * K;
  double acc = 0.0;
  if (k < K)
    for (int g = j; g < ngroups; g += kViewRows) acc += p[(size_t)g * K + k];
  rows[j][k] = acc;
  __syncthreads();
#pragma unroll 1
  for (int h = kViewRows / 2; h >= 1; h >>= 1) {
    if (j < h) rows[j][k] += rows[j + h][k];
    __syncthreads();
  }
  if (j == 0 && k < K) out[((size_t)b * gridDim.x + c) * K + k] = (Out)rows[0][k];
}

// grid (ceil(H W / 256), B).  g_L (B, C, 9) fp32, read at wave-uniform addresses; grad_env (B, H, W, C) fp32.
template <int C>
__global__ __launch_bounds__(kSh9Block) void k_sh9_project_bwd(Sh9Dev P, const float* __restrict__ g_L,
                                                               float* __restrict__ grad_env) {
  const int b = blockIdx.y, p = blockIdx.x * kSh9Block + threadIdx.x, HW = P.H * P.W;
  if (p >= HW) return;
  double S[kSh9Coeffs], domega = 0.0;
  const bool inside = sh9_pixel(P.H, P.W, p, S, domega);
  const auto g = as_constant(g_L + (size_t)b * C * kSh9Coeffs);
  float* out = grad_env + ((size_t)b * HW + p) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double acc = 0.0;
    if (inside) {
#pragma unroll
      for (int k = 0; k < kSh9Coeffs; ++k) acc += S[k] * (double)g[c * kSh9Coeffs + k];
      acc *= domega;
    }
    out[c] = (float)acc;
  }
}

// M[r][s] of channel c in a (4, 4, C) fp32 block
template <int C, class Ptr>
__device__ __forceinline__ double sh9_m(Ptr M, int r, int s, int c) {
  return (double)M[(r * 4 + s) * C + c];
}

// grid (ceil(N / 256), B).  M (B, 4, 4, C) or (4, 4, C) fp32, normal (B, N, 3) fp32, E (B, N, C) fp32.
template <int C>
__global__ __launch_bounds__(kSh9Block) void k_sh9_irradiance_fwd(Sh9Dev P, const float* __restrict__ M,
                                                                  const float* __restrict__ normal,
                                                                  float* __restrict__ E) {
  const int b = blockIdx.y, i = blockIdx.x * kSh9Block + threadIdx.x;
  if (i >= P.N) return;
  const auto Mb = as_constant(M + (P.m_per_view ? (size_t)b * 16 * C : 0));
  const float* np = normal + ((size_t)b * P.N + i) * 3;
  const double n[3] = {(double)np[0], (double)np[1], (double)np[2]};
  float* out = E + ((size_t)b * P.N + i) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
      a[s] = ((n[0] * sh9_m<C>(Mb, 0, s, c) + n[1] * sh9_m<C>(Mb, 1, s, c)) + n[2] * sh9_m<C>(Mb, 2, s, c)) +
             sh9_m<C>(Mb, 3, s, c);
    out[c] = (float)(((a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]) + a[3]);
  }
}

// the monomial k of h = [n, 1]: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
__device__ __forceinline__ constexpr int sh9_mono_r(int k) { return k < 4 ? 0 : (k < 7 ? 1 : (k < 9 ? 2 : 3)); }
__device__ __forceinline__ constexpr int sh9_mono_s(int k) { return k < 4 ? k : (k < 7 ? k - 3 : (k < 9 ? k - 5 : 3)); }
__device__ __host__ __forceinline__ constexpr int sh9_mono_of(int r, int s) {
  const int lo = r < s ? r : s, hi = r < s ? s : r;
  return (lo == 0 ? 0 : (lo == 1 ? 4 : (lo == 2 ? 7 : 9))) + (hi - lo);
}

// grid (ceil(N / 256), B).  g_E (B, N, C) fp32; grad_normal (B, N, 3) fp32 may be NULL = not wanted.  With kGradM,
// part (C, B, gridDim.x, 10) fp64, every element written; a lane past N brings zeros.
template <int C, bool kGradM>
__global__ __launch_bounds__(kSh9Block) void k_sh9_irradiance_bwd(Sh9Dev P, const float* __restrict__ M,
                                                                  const float* __restrict__ normal,
                                                                  const float* __restrict__ g_E,
                                                                  float* __restrict__ grad_normal,
                                                                  double* __restrict__ part) {
  const int b = blockIdx.y, i = blockIdx.x * kSh9Block + threadIdx.x;
  const bool live = i < P.N;
  if (!kGradM && !live) return;
  double h[4] = {0.0, 0.0, 0.0, 1.0}, g[C];
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = 0.0;
  if (live) {
    const float* np = normal + ((size_t)b * P.N + i) * 3;
    const float* gp = g_E + ((size_t)b * P.N + i) * C;
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = (double)np[r];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = (double)gp[c];
  }
  if (live && grad_normal) {
    const auto Mb = as_constant(M + (P.m_per_view ? (size_t)b * 16 * C : 0));
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double d = sh9_m<C>(Mb, r, 3, c) + sh9_m<C>(Mb, 3, r, c);
#pragma unroll
        for (int s = 0; s < 3; ++s) d += (sh9_m<C>(Mb, r, s, c) + sh9_m<C>(Mb, s, r, c)) * h[s];
        acc[r] += g[c] * d;
      }
    }
    float* out = grad_normal + ((size_t)b * P.N + i) * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = (float)acc[r];
  }
  if (kGradM) {
    const size_t per_channel = (size_t)gridDim.y * gridDim.x * kSh9Monomials;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (c) __syncthreads();           // the reduce's LDS is one array for every channel
      view_block_reduce<kSh9Monomials>(
          [&](int k) { return live ? (k == kSh9Monomials - 1 ? g[c] : g[c] * (h[sh9_mono_r(k)] * h[sh9_mono_s(k)])) : 0.0; },
          part + c * per_channel);
    }
  }
}

// mono (B, C, 10) fp64 -> grad_M fp64: (B, 4, 4, C) per view, or (4, 4, C) shared = the views added in ascending order.
// One lane per element of grad_M.
__global__ __launch_bounds__(kSh9SpreadBlock) void k_sh9_spread_M(Sh9Dev P, const double* __restrict__ mono,
                                                                  double* __restrict__ grad_M) {
  const int per_view = 16 * P.C;
  const size_t t = (size_t)blockIdx.x * kSh9SpreadBlock + threadIdx.x;
  const size_t total = (size_t)(P.m_per_view ? P.B : 1) * per_view;
  if (t >= total) return;
  const int b = (int)(t / per_view), e = (int)(t % per_view);
  const int c = e % P.C, rs = e / P.C;
  const int k = sh9_mono_of(rs >> 2, rs & 3);
  if (P.m_per_view) {
    grad_M[t] = mono[((size_t)b * P.C + c) * kSh9Monomials + k];
  } else {
    double acc = 0.0;
    for (int v = 0; v < P.B; ++v) acc += mono[((size_t)v * P.C + c) * kSh9Monomials + k];
    grad_M[t] = acc;
  }
}

}  // namespace srh
