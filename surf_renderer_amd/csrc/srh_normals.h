// The reference's constrained plane fit as a layer of its own: estimate_surface_normals_plane_fit_batched
// (diffrend/torch/utils.py:926-963) on a grid of arbitrary camera-space points, forward and analytic backward to all
// three components of every point; many views per launch (the view is grid dimension y).  See DESIGN.md "Normals from a
// grid of points".  The arithmetic is plane_fit / plane_fit_bwd of srh_splat.h, restated here on points that are READ
// (there they are rebuilt from z along the pixel rays, and the gradient goes to z alone); srh_splat.h is not touched.
//
// Per view, N = W H points P_q, q = i W + j.  At centre c, over the 8 neighbours k of the reflected 3 x 3 stencil
// (dy-major; reflect_idx: -1 -> 1, n -> n - 2, so both sides must be at least 2):
//   u_k = (P_k - P_c) / sqrt(|P_k - P_c|^2 + 3e-10)
//   a = sum ux^2, b = sum ux uy, d = sum uy^2, r = -(sum ux uz, sum uy uz)
//   D = a d - b^2 + 1e-12,  (nx, ny) = adj([[a, b], [b, d]]) r / D,  n = (nx, ny, 1) / sqrt(nx^2 + ny^2 + 1 + 3e-10)
// and with a rotation (the view's orthonormal lookat basis R = [x y z], 9 fp64 per view, row-major, made by the host)
// the stored normal is R n, the value of cam_to_world_batched(None, n, camera)['normal'].
//
// Backward, two launches, no atomic, every element of grad_pos written once:
//   k_normals_bwd     per centre c: the fit again, then d loss / d (a, b, d, r0, r1) -- five fp64 to the workspace
//                     (B, N, 5).  Everything a stencil slot's gradient needs beyond the two points it joins.
//   k_normals_gather  per point q, over its (at most 8) distinct neighbours p inside the grid: v = P_p - P_q is, up to
//                     sign, both the slot of centre q that lands on p and the slot of centre p that lands on q, so one
//                     rsqrt serves both.  With gv(u, C) the gradient of a slot's difference vector under the moments'
//                     gradients C,
//                       g_q = - sum_p [ m(q -> p) gv(u, C_q) + m(p -> q) gv(u, C_p) ]
//                     where m(c -> t) counts the stencil slots of centre c that reflection lands on t (1, 2 or 4).
// This is k_splat_bwd + k_splat_gather's form with the 9 slot gradients (here 27 fp64 per point) replaced by the 5 they
// are linear in.  fp64 arithmetic, one fp32 store per element; neighbours are read through the cache, no LDS.
#pragma once
#include "srh_splat.h"   // reflect_idx, unit_inv3
#include "srh_view_grad.h"

namespace srh {

constexpr int kNormBlock = 256;
constexpr int kNormMoments = 5;   // g_a, g_b, g_d, g_r0, g_r1

struct NormDev {
  int B, W, H, N, nblk;
};

struct NormFit {
  double a, b, d, r0, r1, D, nx, ny, s_inv;
};

__device__ __forceinline__ void norm_load(const float* __restrict__ pos, size_t o, double P[3]) {
  P[0] = (double)pos[3 * o]; P[1] = (double)pos[3 * o + 1]; P[2] = (double)pos[3 * o + 2];
}

// the view's rotation is the same for every lane and written before the launch: scalar loads (proj_load_view's form)
__device__ __forceinline__ void norm_load_rot(const double* rot, int b, double R[9]) {
  const auto* m = as_constant(rot) + (size_t)b * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = m[k];
}

// the plane fit at centre (i, j) of view `base` (the view's first point)
__device__ inline void norm_fit(const NormDev& S, const float* __restrict__ pos, size_t base, int i, int j,
                                const double Pc[3], NormFit& F) {
  double a = 0, b = 0, d = 0, r0 = 0, r1 = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if (k == 4) continue;
    double Pk[3];
    norm_load(pos, base + (size_t)(reflect_idx(i + k / 3 - 1, S.H) * S.W + reflect_idx(j + k % 3 - 1, S.W)), Pk);
    const double v[3] = {Pk[0] - Pc[0], Pk[1] - Pc[1], Pk[2] - Pc[2]};
    const double si = unit_inv3(v);
    const double u0 = v[0] * si, u1 = v[1] * si, u2 = v[2] * si;
    a += u0 * u0; b += u0 * u1; d += u1 * u1; r0 -= u0 * u2; r1 -= u1 * u2;
  }
  F.a = a; F.b = b; F.d = d; F.r0 = r0; F.r1 = r1;
  F.D = (a * d - b * b) + 1.0e-12;
  F.nx = (d * r0 - b * r1) / F.D;
  F.ny = (a * r1 - b * r0) / F.D;
  const double v[3] = {F.nx, F.ny, 1.0};
  F.s_inv = unit_inv3(v);
}

// pos (B, N, 3) fp32 -> out (B, N, 3) fp32; rot (B, 9) fp64 or NULL (the camera frame)
__global__ __launch_bounds__(kNormBlock) void k_normals_fwd(NormDev S, const double* __restrict__ rot,
                                                            const float* __restrict__ pos, float* __restrict__ out) {
  const int q = blockIdx.x * kNormBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= S.N) return;
  const size_t base = (size_t)b * S.N;
  const int i = q / S.W, j = q - i * S.W;
  double Pc[3];
  norm_load(pos, base + q, Pc);
  NormFit F;
  norm_fit(S, pos, base, i, j, Pc, F);
  double n[3] = {F.nx * F.s_inv, F.ny * F.s_inv, F.s_inv};
  if (rot) {
    double R[9];
    norm_load_rot(rot, b, R);
    const double x = n[0], y = n[1], z = n[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) n[r] = (R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) out[3 * (base + q) + r] = (float)n[r];
}

// Backward, pass 1: g_out (B, N, 3) fp32 -> ws (B, N, 5) fp64, d loss / d (a, b, d, r0, r1) of every centre.
// kView (with rot): also the gradient of the view's rotation: out = R n, so g_R = sum_q g_out[q] (x) n[q] with n the
// unit camera-space normal formed below.  The lane keeps g_out and n (vg, vn), a lane past N brings zeros, and each
// workgroup stores its 9 sums to view_part (srh_view_grad.h); ws may then be NULL = grad_pos is not wanted.  Without
// kView the trailing argument is unused and the code is what it was without it.
template <bool kView>
__global__ __launch_bounds__(kNormBlock) void k_normals_bwd(NormDev S, const double* __restrict__ rot,
                                                            const float* __restrict__ pos,
                                                            const float* __restrict__ g_out, double* __restrict__ ws,
                                                            double* __restrict__ view_part) {
  const int q = blockIdx.x * kNormBlock + threadIdx.x;
  const int b = blockIdx.y;
  double vg[3] = {0.0, 0.0, 0.0}, vn[3] = {0.0, 0.0, 0.0};      // kView: g_out and n; zeros bring zeros
  do {                                  // a lane that is done leaves by `break`: with kView every lane reaches the reduce
  if (q >= S.N) break;
  const size_t base = (size_t)b * S.N;
  const int i = q / S.W, j = q - i * S.W;
  double Pc[3], g_n[3];
  norm_load(pos, base + q, Pc);
  norm_load(g_out, base + q, g_n);
  if (kView) {
#pragma unroll
    for (int c = 0; c < 3; ++c) vg[c] = g_n[c];
  }
  if (rot) {                                   // R^T g
    double R[9];
    norm_load_rot(rot, b, R);
    const double gx = g_n[0], gy = g_n[1], gz = g_n[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) g_n[c] = (R[c] * gx + R[3 + c] * gy) + R[6 + c] * gz;
  }
  NormFit F;
  norm_fit(S, pos, base, i, j, Pc, F);
  const double n[3] = {F.nx * F.s_inv, F.ny * F.s_inv, F.s_inv};
  if (kView) {
#pragma unroll
    for (int c = 0; c < 3; ++c) vn[c] = n[c];
    if (!ws) break;
  }
  const double proj = (n[0] * g_n[0] + n[1] * g_n[1]) + n[2] * g_n[2];
  const double g_nx = (g_n[0] - n[0] * proj) * F.s_inv, g_ny = (g_n[1] - n[1] * proj) * F.s_inv;
  const double g_D = -(F.nx * g_nx + F.ny * g_ny) / F.D;
  double* w = ws + (base + q) * kNormMoments;
  w[0] = (F.r1 * g_ny) / F.D + g_D * F.d;                                  // g_a
  w[1] = (-F.r1 * g_nx - F.r0 * g_ny) / F.D - 2.0 * g_D * F.b;             // g_b
  w[2] = (F.r0 * g_nx) / F.D + g_D * F.a;                                  // g_d
  w[3] = (F.d * g_nx - F.b * g_ny) / F.D;                                  // g_r0
  w[4] = (F.a * g_ny - F.b * g_nx) / F.D;                                  // g_r1
  } while (false);
  if (kView) view_block_reduce<9>([&](int k) { return vg[k / 3] * vn[k % 3]; }, view_part);
}

// how many of the offsets -1, 0, 1 from `from` reflection lands on `to`, along an axis of n samples
__device__ __forceinline__ int norm_hits(int from, int to, int n) {
  return (reflect_idx(from - 1, n) == to) + (from == to) + (reflect_idx(from + 1, n) == to);
}

// d loss / d v of a slot with unit difference u = v si, under the moments' gradients C
__device__ __forceinline__ void norm_slot_grad(const double u[3], double si, const double* __restrict__ C, double gv[3]) {
  const double gu[3] = {2.0 * u[0] * C[0] + u[1] * C[1] - u[2] * C[3], 2.0 * u[1] * C[2] + u[0] * C[1] - u[2] * C[4],
                        -u[0] * C[3] - u[1] * C[4]};
  const double pu = (u[0] * gu[0] + u[1] * gu[1]) + u[2] * gu[2];
#pragma unroll
  for (int m = 0; m < 3; ++m) gv[m] = (gu[m] - u[m] * pu) * si;
}

// Backward, pass 2: ws (B, N, 5) fp64 -> grad_pos (B, N, 3) fp32, every element written
__global__ __launch_bounds__(kNormBlock) void k_normals_gather(NormDev S, const float* __restrict__ pos,
                                                               const double* __restrict__ ws,
                                                               float* __restrict__ grad_pos) {
  const int q = blockIdx.x * kNormBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= S.N) return;
  const size_t base = (size_t)b * S.N;
  const int qi = q / S.W, qj = q - qi * S.W;
  double Pq[3], Cq[kNormMoments], g[3] = {0.0, 0.0, 0.0};
  norm_load(pos, base + q, Pq);
#pragma unroll
  for (int m = 0; m < kNormMoments; ++m) Cq[m] = ws[(base + q) * kNormMoments + m];
  for (int pi = qi - 1; pi <= qi + 1; ++pi) {
    if (pi < 0 || pi >= S.H) continue;
    for (int pj = qj - 1; pj <= qj + 1; ++pj) {
      if (pj < 0 || pj >= S.W || (pi == qi && pj == qj)) continue;
      const size_t p = base + (size_t)(pi * S.W + pj);
      double Pp[3], Cp[kNormMoments];
      norm_load(pos, p, Pp);
#pragma unroll
      for (int m = 0; m < kNormMoments; ++m) Cp[m] = ws[p * kNormMoments + m];
      const double v[3] = {Pp[0] - Pq[0], Pp[1] - Pq[1], Pp[2] - Pq[2]};
      const double si = unit_inv3(v);
      const double u[3] = {v[0] * si, v[1] * si, v[2] * si};
      const double own = (double)(norm_hits(qi, pi, S.H) * norm_hits(qj, pj, S.W));    // slots of centre q on p
      const double nbr = (double)(norm_hits(pi, qi, S.H) * norm_hits(pj, qj, S.W));    // slots of centre p on q
      double gq[3], gp[3];
      norm_slot_grad(u, si, Cq, gq);
      norm_slot_grad(u, si, Cp, gp);
#pragma unroll
      for (int m = 0; m < 3; ++m) g[m] -= own * gq[m] + nbr * gp[m];
    }
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) grad_pos[3 * (base + q) + m] = (float)g[m];
}
}  // namespace srh
