// The seven geometric regularisers the reference's trainers put on every rendered splat view (diffrend/torch/GAN/
// gan.py:601-640 with diffrend/torch/utils.py:731-851), forward and analytic backward, many views per launch (the view
// is grid dimension y).  See DESIGN.md "The splat regularisers".
//
// Per view, N = H W pixels of pos / normal / image (H, W, 3) and depth (H, W); d_k(x) = x[neighbour k] - x[centre] over
// the 3 x 3 stencil without its centre, reflected at the borders (grad_spatial2d):
//   0 z                        mean (s relu(z_min - |p_z|))^2 + (s relu(|p_z| - z_max))^2
//   1 unit_normal              mean (c (|n| - 1))^2
//   2 normal_consistency       mean over the 8 N pairs of |u_k . n|,  u_k = d_k(pos) / sqrt(|d_k|^2 + 3e-10)
//   3 spatial                  mean over the 8 N pairs of sum_c |d_k(pos)_c|
//   4 spatial_var              1 / (var p_x + var p_y + var p_z + 1e-4), unbiased variances
//   5 image_depth_consistency  mean over the 8 N pairs of | |d_k(mean_c image)| - |d_k(depth)| |
//   6 away_from_camera         SUM of relu(n . p / sqrt(|p|^2 + 3e-10))
// Everything is computed in fp64 and stored as fp32.  No atomics anywhere: the forward reduces per workgroup into one
// row of partial sums and a one-wave finish kernel adds the rows in a fixed order; the backward is a gather that writes
// every gradient element once.  Values and gradients are therefore identical from run to run.
//
// The variances are taken of p - p_0 (p_0 = the view's first pixel), which has the same variance and none of the
// cancellation of sum p^2 - (sum p)^2 / N for a cloud that is thin against its distance from the origin.
//
// The per-pixel arithmetic (reg_pixel_fwd / reg_finish / reg_pixel_bwd) is host-callable so that it can be checked
// without a GPU: tests/host/regularizers_host.hip, run by tests/test_regularizers_host_cpu.py.
#pragma once
#include "srh_device.h"   // as_constant

namespace srh {

constexpr int kRegTerms = 7;
constexpr int kRegSums = 12;      // z, unit, consistency, spatial, image-depth, away, sum q (3), sum q^2 (3)
constexpr int kRegStats = 4;      // mean p (3), variance sum
constexpr int kRegBlock = 256;

struct RegDev {
  int B, W, H, N, nblk;
  double z_min, z_max, z_scale, n_scale;
  const float* pos;
  const float* normal;
  const float* image;
  const float* depth;
};

struct RegGradsDev {
  float* pos;
  float* normal;
  float* image;
  float* depth;
};

__host__ __device__ __forceinline__ double reg_sgn(double x) { return (double)(x > 0.0) - (double)(x < 0.0); }
// torch.relu: a NaN stays a NaN (fmax(x, 0) would return 0)
__host__ __device__ __forceinline__ double reg_relu(double x) { return x < 0.0 ? 0.0 : x; }
__host__ __device__ __forceinline__ double reg_dot(const double a[3], const double b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__host__ __device__ __forceinline__ double reg_unit_inv(const double v[3]) { return 1.0 / sqrt(reg_dot(v, v) + 3.0e-10); }
__host__ __device__ __forceinline__ int reg_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
// how many of a's three stencil offsets land on b after reflection (|a - b| <= 1)
__host__ __device__ __forceinline__ int reg_hits(int a, int b, int n) {
  return (int)(reg_reflect(a - 1, n) == b) + (int)(a == b) + (int)(reg_reflect(a + 1, n) == b);
}
__host__ __device__ __forceinline__ void reg_load3(const float* p, size_t i, double v[3]) {
  v[0] = p[3 * i]; v[1] = p[3 * i + 1]; v[2] = p[3 * i + 2];
}
__host__ __device__ __forceinline__ double reg_grey(const float* image, size_t i) {
  return (((double)image[3 * i] + (double)image[3 * i + 1]) + (double)image[3 * i + 2]) / 3.0;
}

// The contributions of pixel (i, j) of view b, as the centre of its eight pairs, to the kRegSums sums; p0 = the
// view's first pixel.
__host__ __device__ inline void reg_pixel_fwd(const RegDev& R, int b, int i, int j, const double p0[3],
                                              double acc[kRegSums]) {
  const size_t base = (size_t)b * R.N;
  const size_t c = base + (size_t)i * R.W + j;
  double p[3], n[3];
  reg_load3(R.pos, c, p);
  reg_load3(R.normal, c, n);
  const double grey = reg_grey(R.image, c), dep = R.depth[c];
  const double az = fabs(p[2]);
  const double lo = R.z_scale * reg_relu(R.z_min - az), hi = R.z_scale * reg_relu(az - R.z_max);
  acc[0] = lo * lo + hi * hi;
  const double e = R.n_scale * (sqrt(reg_dot(n, n)) - 1.0);
  acc[1] = e * e;
  acc[5] = reg_relu(reg_dot(n, p) * reg_unit_inv(p));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double q = p[k] - p0[k];
    acc[6 + k] = q;
    acc[9 + k] = q * q;
  }
  double cons = 0.0, spat = 0.0, idc = 0.0;
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    if (k == 4) continue;
    const size_t nb = base + (size_t)reg_reflect(i + k / 3 - 1, R.H) * R.W + reg_reflect(j + k % 3 - 1, R.W);
    double pk[3];
    reg_load3(R.pos, nb, pk);
    const double d[3] = {pk[0] - p[0], pk[1] - p[1], pk[2] - p[2]};
    spat += (fabs(d[0]) + fabs(d[1])) + fabs(d[2]);
    cons += fabs(reg_dot(d, n) * reg_unit_inv(d));
    idc += fabs(fabs(reg_grey(R.image, nb) - grey) - fabs((double)R.depth[nb] - dep));
  }
  acc[2] = cons; acc[3] = spat; acc[4] = idc;
}

// terms (fp32) and stats of one view from its kRegSums totals
__host__ __device__ inline void reg_finish(const RegDev& R, const double S[kRegSums], const double p0[3],
                                           float terms[kRegTerms], double stats[kRegStats]) {
  const double N = (double)R.N;
  double V = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mq = S[6 + k] / N;
    V += (S[9 + k] - S[6 + k] * mq) / (N - 1.0);
    stats[k] = p0[k] + mq;
  }
  stats[3] = V;
  terms[0] = (float)(S[0] / N);
  terms[1] = (float)(S[1] / N);
  terms[2] = (float)(S[2] / (8.0 * N));
  terms[3] = (float)(S[3] / (8.0 * N));
  terms[4] = (float)(1.0 / (V + 1.0e-4));
  terms[5] = (float)(S[4] / (8.0 * N));
  terms[6] = (float)S[5];
}

// d loss / d (pos, normal, image, depth) of pixel (qi, qj) of view b for the upstream weights w of the view's seven
// terms: its own terms, its eight pairs as their centre, and every pair of a neighbouring centre whose reflected
// stencil lands on it.  A pair of centre a and neighbour c depends on (a, c) alone, so the slots of a that land on c
// -- more than one at a border -- enter as a multiplicity.  want_geo / want_img: skip the work nobody stores.
__host__ __device__ inline void reg_pixel_bwd(const RegDev& R, int b, int qi, int qj, const double w[kRegTerms],
                                              const double stats[kRegStats], bool want_geo, bool want_img,
                                              double gp[3], double gn[3], double& g_grey, double& g_dep) {
  const size_t base = (size_t)b * R.N;
  const size_t q = base + (size_t)qi * R.W + qj;
  const double N = (double)R.N;
  gp[0] = gp[1] = gp[2] = gn[0] = gn[1] = gn[2] = 0.0;
  g_grey = g_dep = 0.0;
  double p[3], n[3] = {0.0, 0.0, 0.0};
  double grey = 0.0, dep = 0.0;
  reg_load3(R.pos, q, p);
  if (want_geo) {
    reg_load3(R.normal, q, n);
    // z: relu has no gradient at 0, |.| none at 0
    const double az = fabs(p[2]), sz = reg_sgn(p[2]);
    const double lo = R.z_min - az, hi = az - R.z_max;
    const double s2 = 2.0 * R.z_scale * R.z_scale;
    double gz = 0.0;
    if (lo > 0.0) gz -= s2 * lo * sz;
    if (hi > 0.0) gz += s2 * hi * sz;
    gp[2] += (w[0] / N) * gz;
    // unit_normal: a zero normal gets no gradient
    const double r = sqrt(reg_dot(n, n));
    if (r > 0.0) {
      const double f = (w[1] / N) * (2.0 * R.n_scale * R.n_scale) * (r - 1.0) / r;
#pragma unroll
      for (int k = 0; k < 3; ++k) gn[k] += f * n[k];
    }
    // spatial_var = 1 / (V + 1e-4)
    const double den = stats[3] + 1.0e-4;
    const double fv = -(w[4] / (den * den)) * (2.0 / (N - 1.0));
#pragma unroll
    for (int k = 0; k < 3; ++k) gp[k] += fv * (p[k] - stats[k]);
    // away_from_camera: t = (n . p) si
    const double si = reg_unit_inv(p), np = reg_dot(n, p);
    if (np * si > 0.0) {
      const double si3 = si * si * si;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        gn[k] += w[6] * p[k] * si;
        gp[k] += w[6] * (n[k] * si - p[k] * (np * si3));
      }
    }
  }
  if (want_img) {
    grey = reg_grey(R.image, q);
    dep = R.depth[q];
  }
  const double w_cons = w[2] / (8.0 * N), w_spat = w[3] / (8.0 * N), w_idc = w[5] / (8.0 * N);
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    const int ci = qi + k / 3 - 1, cj = qj + k % 3 - 1;
    if (k == 4 || ci < 0 || ci >= R.H || cj < 0 || cj >= R.W) continue;
    const size_t c = base + (size_t)ci * R.W + cj;
    const double m_qc = (double)(reg_hits(qi, ci, R.H) * reg_hits(qj, cj, R.W));   // q the centre, c its neighbour
    const double m_cq = (double)(reg_hits(ci, qi, R.H) * reg_hits(cj, qj, R.W));   // c the centre, q its neighbour
    if (want_geo) {
      double pc[3], nc[3];
      reg_load3(R.pos, c, pc);
      reg_load3(R.normal, c, nc);
      const double d[3] = {pc[0] - p[0], pc[1] - p[1], pc[2] - p[2]};
      const double si = reg_unit_inv(d);
      const double u[3] = {d[0] * si, d[1] * si, d[2] * si};
      const double tq = reg_dot(u, n), sq = reg_sgn(tq);       // centre q: |u . n_q|
      const double tc = -reg_dot(u, nc), sc = reg_sgn(tc);     // centre c: its difference is -d, |-u . n_c|
      const double fq = w_cons * m_qc, fc = w_cons * m_cq, fs = w_spat * (m_qc + m_cq);
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        // d |t| / d d = sgn(t) (n - u t) si for t = u . n;  q is the pair's centre once (- d/dd) and its neighbour once
        gp[m] -= fq * (sq * (n[m] - u[m] * tq) * si);
        gp[m] += fc * (sc * (nc[m] + u[m] * tc) * si);
        gn[m] += fq * sq * u[m];
        gp[m] -= fs * reg_sgn(d[m]);
      }
    }
    if (want_img) {
      const double a = reg_grey(R.image, c) - grey, e = (double)R.depth[c] - dep;
      const double s = w_idc * (m_qc + m_cq) * reg_sgn(fabs(a) - fabs(e));
      g_grey -= s * reg_sgn(a);
      g_dep += s * reg_sgn(e);
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// the view's first pixel: a wave-uniform address of an input no kernel here writes -> scalar loads
__device__ __forceinline__ void reg_first_pixel(const RegDev& R, int b, double p0[3]) {
  const auto* q = as_constant(R.pos) + 3 * (size_t)b * R.N;
  p0[0] = q[0]; p0[1] = q[1]; p0[2] = q[2];
}

// Forward, pass 1: one lane per pixel of view blockIdx.y; one row of kRegSums partial sums per workgroup into
// ws (B, nblk, kRegSums).  Within the workgroup: xor-butterfly over each wave, then the four waves in order.
__global__ __launch_bounds__(kRegBlock) void k_reg_fwd(RegDev R, double* __restrict__ ws) {
  __shared__ double part[kRegBlock / 64][kRegSums];
  const int pix = blockIdx.x * kRegBlock + threadIdx.x;
  const int b = blockIdx.y;
  double acc[kRegSums];
#pragma unroll
  for (int k = 0; k < kRegSums; ++k) acc[k] = 0.0;
  if (pix < R.N) {
    double p0[3];
    reg_first_pixel(R, b, p0);
    reg_pixel_fwd(R, b, pix / R.W, pix - (pix / R.W) * R.W, p0, acc);
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kRegSums; ++k) {
    const double s = wave_sum_f64(acc[k]);
    if ((threadIdx.x & 63) == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kRegSums) {
    double s = part[0][threadIdx.x];
#pragma unroll
    for (int v = 1; v < kRegBlock / 64; ++v) s += part[v][threadIdx.x];
    ws[((size_t)b * R.nblk + blockIdx.x) * kRegSums + threadIdx.x] = s;
  }
}

// Forward, pass 2: one wave per view adds the partial rows (lane l takes rows l, l + 64, ... in order, then the
// butterfly) and writes terms (B, kRegTerms) fp32 and stats (B, kRegStats) fp64.
__global__ __launch_bounds__(64) void k_reg_finish(RegDev R, const double* __restrict__ ws, float* __restrict__ terms,
                                                   double* __restrict__ stats) {
  const int b = blockIdx.x;
  double S[kRegSums];
#pragma unroll
  for (int k = 0; k < kRegSums; ++k) S[k] = 0.0;
  for (int r = threadIdx.x; r < R.nblk; r += 64) {
    const double* row = ws + ((size_t)b * R.nblk + r) * kRegSums;
#pragma unroll
    for (int k = 0; k < kRegSums; ++k) S[k] += row[k];
  }
#pragma unroll
  for (int k = 0; k < kRegSums; ++k) S[k] = wave_sum_f64(S[k]);
  if (threadIdx.x == 0) {
    double p0[3];
    reg_first_pixel(R, b, p0);
    float t[kRegTerms];
    double st[kRegStats];
    reg_finish(R, S, p0, t, st);
#pragma unroll
    for (int k = 0; k < kRegTerms; ++k) terms[(size_t)b * kRegTerms + k] = t[k];
#pragma unroll
    for (int k = 0; k < kRegStats; ++k) stats[(size_t)b * kRegStats + k] = st[k];
  }
}

// Backward: one lane per pixel, a gather (reg_pixel_bwd); every element of every requested buffer is written once.
// grad_terms (B, kRegTerms) fp32 and stats are per view: wave-uniform, written by earlier launches, scalar loads.
__global__ __launch_bounds__(kRegBlock) void k_reg_bwd(RegDev R, RegGradsDev G, const double* __restrict__ stats,
                                                       const float* __restrict__ grad_terms) {
  const int pix = blockIdx.x * kRegBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (pix >= R.N) return;
  double w[kRegTerms], st[kRegStats];
  const auto* gt = as_constant(grad_terms) + (size_t)b * kRegTerms;
  const auto* sv = as_constant(stats) + (size_t)b * kRegStats;
#pragma unroll
  for (int k = 0; k < kRegTerms; ++k) w[k] = gt[k];
#pragma unroll
  for (int k = 0; k < kRegStats; ++k) st[k] = sv[k];
  double gp[3], gn[3], g_grey, g_dep;
  reg_pixel_bwd(R, b, pix / R.W, pix - (pix / R.W) * R.W, w, st, G.pos || G.normal, G.image || G.depth, gp, gn, g_grey,
                g_dep);
  const size_t o = (size_t)b * R.N + pix;
  if (G.pos) { G.pos[3 * o] = (float)gp[0]; G.pos[3 * o + 1] = (float)gp[1]; G.pos[3 * o + 2] = (float)gp[2]; }
  if (G.normal) { G.normal[3 * o] = (float)gn[0]; G.normal[3 * o + 1] = (float)gn[1]; G.normal[3 * o + 2] = (float)gn[2]; }
  if (G.image) {
    const float g = (float)(g_grey / 3.0);
    G.image[3 * o] = g; G.image[3 * o + 1] = g; G.image[3 * o + 2] = g;
  }
  if (G.depth) G.depth[o] = (float)g_dep;
}
}  // namespace srh
