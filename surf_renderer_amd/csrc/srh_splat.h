// The reference's splat renderer, render_splats_along_ray (diffrend/torch/renderer.py:537-751): one splat per base
// pixel, given by its camera-space depth z, shaded where it lies -- no intersection, no occlusion.  Forward and analytic
// backward, many views per launch (the view is grid dimension y).  See DESIGN.md "The splat renderer".
//
//   grid       x_j = fp32(linspace(-1, 1, W)_j w / 2),  y_i = fp32(linspace(1, -1, H)_i h / 2)
//   position   Z = min(z, 0) (-relu(-z)),  P = (-Z x / f, -Z y / f, Z)
//   normal     given (as is), or the plane fit over the reflected 3x3 stencil of P (plane_fit below)
//   sub-pixels K > 1: ray r = unit(x + sx dx / 2, y + sy dy / 2, -f), pos = (P.n / r.n) r; sub-pixel (c, r) of base
//              pixel (i, j) is output pixel (i K + c, j K + r) -- the x shift runs down the rows, as in the reference
//   shading    the torch backend's Phong with double_sided off, lights in camera coordinates (R^T (l - l_w eye), R the
//              orthonormal lookat basis of the view's eye), light_vis on colour x albedo, relu over the light sum
// Everything is computed in fp64 and stored as fp32.  One lane per BASE pixel: it evaluates the K x K sub-pixels of
// its splat, so the plane fit runs once per splat and the backward sums over sub-pixels in registers, without atomics.
//
// Backward (k_splat_bwd + k_splat_gather): the per-pixel gradients (z, given normals, light_vis) are WRITTEN, each by
// the one lane that owns the pixel, so they are identical from run to run.  The plane fit couples a splat to its eight
// neighbours: k_splat_bwd stores, per splat, d loss / d Z of each of the 9 stencil slots (fp64 workspace), and
// k_splat_gather sums for every splat the slots of its neighbours that land on it (reflection included).  Scene
// parameters (lights, colours, materials) are reduced over the wave and added with fp32 atomics, as srh_backward.h does.
//
// The camera (k_splat_bwd<true>, k_splat_ndc_bwd<true>): it enters only through the lights' camera coordinates
// L = M (l_xyz, l_w), M = [R^T | -R^T eye] the view's 3 x 4 world-to-camera matrix, so d loss / d M[r][c] is the sum
// over pixels, sub-pixels and lights of g_v[r] l[c] (view_light_terms).  The lane keeps the twelve sums in fp64 across
// both loops and the workgroup reduces them once, after the loops (srh_view_grad.h): no atomics, fp64 to the end.
#pragma once
#include "srh_backward.h"   // wave_sum
#include "srh_device.h"
#include "srh_view_grad.h"

namespace srh {

struct SplatDev {
  int B, W, H, K, N, pos_cols, nlights, ncolors, nmat, use_quartic, shade, estimate;
  double f, half_w, half_h, step_x, step_y, sub_dx, sub_dy, sub_step;
  double at[3], up[3];                       // up already unit (the reference normalises it with eps 1e-10)
  const float* pos;        int64_t pos_vs;
  const float* normal;     int64_t nrm_vs;
  const float* vis;        int64_t vis_vs;
  const float* eye;        int64_t eye_vs;
  const float* lpos;       int64_t lpos_vs;
  const int32_t* lcidx;
  const float* colors;
  const float* latt;       // NULL = (1, 0, 0)
  const float* amb;        // NULL = 0
  const int32_t* mat;      // NULL = material 0
  const float* albedo;
  const float* coeffs;     // NULL = (1, 0, 0)
};

struct SplatGradsDev {
  float* pos;
  float* normal;
  float* vis;
  float* lpos;
  float* colors;
  float* latt;
  float* amb;
  float* albedo;
  float* coeffs;
};

__device__ __forceinline__ double unit_inv3(const double v[3]) {
  return 1.0 / sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 3.0e-10);
}

// the reference's float32 grid coordinates (numpy linspace: i * step + start, the last sample exactly the end point)
__device__ __forceinline__ double grid_x(const SplatDev& S, int j) {
  const double s = (S.W == 1) ? -1.0 : ((j == S.W - 1) ? 1.0 : (j * S.step_x + -1.0));
  return (double)(float)(s * S.half_w);
}
__device__ __forceinline__ double grid_y(const SplatDev& S, int i) {
  const double s = (S.H == 1) ? 1.0 : ((i == S.H - 1) ? -1.0 : (i * S.step_y + 1.0));
  return (double)(float)(s * S.half_h);
}
__device__ __forceinline__ double sub_shift(const SplatDev& S, int c) {   // linspace(-1, 1, K)_c
  return (c == S.K - 1) ? 1.0 : (c * S.sub_step + -1.0);
}
__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__device__ __forceinline__ double load_z(const SplatDev& S, int b, int pix) {
  return (double)S.pos[(size_t)b * S.pos_vs + (size_t)pix * S.pos_cols + (S.pos_cols == 3 ? 2 : 0)];
}
// camera-space point of splat (i, j) and the direction dP/dZ = (-x/f, -y/f, 1)
__device__ __forceinline__ void splat_point(const SplatDev& S, int b, int i, int j, double P[3], double dPdZ[3]) {
  const double z = load_z(S, b, i * S.W + j);
  const double Z = (z < 0.0) ? z : 0.0;
  const double x = grid_x(S, j), y = grid_y(S, i);
  P[0] = (-Z * x) / S.f; P[1] = (-Z * y) / S.f; P[2] = Z;
  dPdZ[0] = -x / S.f; dPdZ[1] = -y / S.f; dPdZ[2] = 1.0;
}

// Plane fit at splat (i, j): u_k = unit(P_k - P_c) over the 8 neighbours (dy-major), a = sum ux^2, b = sum ux uy,
// d = sum uy^2, r = -(sum ux uz, sum uy uz), (nx, ny) = adj([[a, b], [b, d]]) r / (ad - b^2 + 1e-12), n = unit(nx, ny, 1)
struct PlaneFit {
  double a, b, d, r0, r1, D, nx, ny, s_inv;
};
__device__ inline void plane_fit(const SplatDev& S, int bv, int i, int j, const double Pc[3], PlaneFit& F) {
  double a = 0, b = 0, d = 0, r0 = 0, r1 = 0;
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    if (k == 4) continue;
    double Pk[3], dz[3];
    splat_point(S, bv, reflect_idx(i + k / 3 - 1, S.H), reflect_idx(j + k % 3 - 1, S.W), Pk, dz);
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

// Backward of the plane fit for d loss / d n = g_n: d loss / d Z of the 9 stencil slots (g_direct, d loss / d P of the
// centre from everything else, is folded into slot 4)
__device__ inline void plane_fit_bwd(const SplatDev& S, int bv, int i, int j, const double Pc[3], const PlaneFit& F,
                                     const double g_n[3], const double g_direct[3], double gZ[9]) {
  const double n[3] = {F.nx * F.s_inv, F.ny * F.s_inv, F.s_inv};
  const double proj = (n[0] * g_n[0] + n[1] * g_n[1]) + n[2] * g_n[2];
  const double g_nx = (g_n[0] - n[0] * proj) * F.s_inv, g_ny = (g_n[1] - n[1] * proj) * F.s_inv;
  const double g_r0 = (F.d * g_nx - F.b * g_ny) / F.D, g_r1 = (F.a * g_ny - F.b * g_nx) / F.D;
  const double g_D = -(F.nx * g_nx + F.ny * g_ny) / F.D;
  const double g_a = (F.r1 * g_ny) / F.D + g_D * F.d;
  const double g_d = (F.r0 * g_nx) / F.D + g_D * F.a;
  const double g_b = (-F.r1 * g_nx - F.r0 * g_ny) / F.D - 2.0 * g_D * F.b;
  double gc[3] = {g_direct[0], g_direct[1], g_direct[2]};
  double dPc[3];
  {
    double Pt[3];
    splat_point(S, bv, i, j, Pt, dPc);
  }
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    if (k == 4) continue;
    double Pk[3], dPk[3];
    splat_point(S, bv, reflect_idx(i + k / 3 - 1, S.H), reflect_idx(j + k % 3 - 1, S.W), Pk, dPk);
    const double v[3] = {Pk[0] - Pc[0], Pk[1] - Pc[1], Pk[2] - Pc[2]};
    const double si = unit_inv3(v);
    const double u[3] = {v[0] * si, v[1] * si, v[2] * si};
    const double gu[3] = {2.0 * u[0] * g_a + u[1] * g_b - u[2] * g_r0, 2.0 * u[1] * g_d + u[0] * g_b - u[2] * g_r1,
                          -u[0] * g_r0 - u[1] * g_r1};
    const double pu = (u[0] * gu[0] + u[1] * gu[1]) + u[2] * gu[2];
    double gv[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      gv[m] = (gu[m] - u[m] * pu) * si;
      gc[m] -= gv[m];
    }
    gZ[k] = (gv[0] * dPk[0] + gv[1] * dPk[1]) + gv[2] * dPk[2];
  }
  gZ[4] = (gc[0] * dPc[0] + gc[1] * dPc[1]) + gc[2] * dPc[2];
}

// the view's orthonormal lookat basis R = [x y z] (columns) and eye
__device__ inline void splat_basis(const SplatDev& S, int b, double R[3][3], double e[3]) {
  const float* ep = S.eye + (size_t)b * S.eye_vs;
  e[0] = ep[0]; e[1] = ep[1]; e[2] = ep[2];
  double z[3] = {e[0] - S.at[0], e[1] - S.at[1], e[2] - S.at[2]};
  const double zi = unit_inv3(z);
  z[0] *= zi; z[1] *= zi; z[2] *= zi;
  double x[3] = {S.up[1] * z[2] - S.up[2] * z[1], S.up[2] * z[0] - S.up[0] * z[2], S.up[0] * z[1] - S.up[1] * z[0]};
  const double xi = unit_inv3(x);
  x[0] *= xi; x[1] *= xi; x[2] *= xi;
  const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
#pragma unroll
  for (int k = 0; k < 3; ++k) { R[k][0] = x[k]; R[k][1] = y[k]; R[k][2] = z[k]; }
}

// light l in camera coordinates: R^T (l_xyz - l_w eye)
__device__ __forceinline__ void light_cc(const SplatDev& S, int b, int l, const double R[3][3], const double e[3],
                                         double L[3]) {
  const float* lp = S.lpos + (size_t)b * S.lpos_vs + 4 * (size_t)l;
  const double w = lp[3];
  const double q[3] = {(double)lp[0] - w * e[0], (double)lp[1] - w * e[1], (double)lp[2] - w * e[2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) L[k] = (R[0][k] * q[0] + R[1][k] * q[1]) + R[2][k] * q[2];
}

// kView: the lane's share of d loss / d M for light l, g_v (x) (l_x, l_y, l_z, l_w), added to its twelve running sums
__device__ __forceinline__ void view_light_terms(const SplatDev& S, int b, int l, const double g_v[3], double vM[12]) {
  const float* lp = S.lpos + (size_t)b * S.lpos_vs + 4 * (size_t)l;
#pragma unroll
  for (int k = 0; k < 12; ++k) vM[k] += g_v[k >> 2] * (double)lp[k & 3];
}

struct SplatLight {
  double lh[3], dist, afac, ldn, nd, rd, cl, den, dp;
  bool nz, den_ok;
};
__device__ __forceinline__ void splat_light(const SplatDev& S, int l, const double L[3], const double p[3],
                                            const double n[3], const double cdir[3], double cdotn, SplatLight& T) {
  const double v[3] = {L[0] - p[0], L[1] - p[1], L[2] - p[2]};
  T.dist = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  T.nz = T.dist > 0.0;
  const double inv = T.nz ? 1.0 / T.dist : 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) T.lh[k] = v[k] * inv;
  const double kc = S.latt ? S.latt[3 * l] : 1.0, kl = S.latt ? S.latt[3 * l + 1] : 0.0,
               kq = S.latt ? S.latt[3 * l + 2] : 0.0;
  const double d2 = T.dist * T.dist;
  T.dp = S.use_quartic ? d2 * d2 : d2;
  T.den = (kc + T.dist * kl) + T.dp * kq;
  T.den_ok = fabs(T.den) > 0.0;
  T.afac = T.den_ok ? 1.0 / T.den : 1.0;
  T.ldn = (T.lh[0] * n[0] + T.lh[1] * n[1]) + T.lh[2] * n[2];
  T.cl = (cdir[0] * T.lh[0] + cdir[1] * T.lh[1]) + cdir[2] * T.lh[2];
  T.nd = T.afac * T.ldn;
  T.rd = 2.0 * T.ldn * cdotn - T.cl;
}

// torch.pow: 0^0 = 1
__device__ __forceinline__ double splat_pow(double x, double e) { return (x == 0.0 && e == 0.0) ? 1.0 : pow(x, e); }

struct SplatPixel {          // what the light loops read of one (sub-)pixel
  double p[3], n[3], cdir[3], cdotn, s_inv;
  double alb[3], cf[3], amb[3];
};

__device__ inline void splat_pixel(const SplatDev& S, const double p[3], const double n[3], int m, SplatPixel& X) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { X.p[k] = p[k]; X.n[k] = n[k]; }
  X.s_inv = unit_inv3(p);
#pragma unroll
  for (int k = 0; k < 3; ++k) X.cdir[k] = -p[k] * X.s_inv;
  X.cdotn = (X.cdir[0] * n[0] + X.cdir[1] * n[1]) + X.cdir[2] * n[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    X.alb[k] = S.albedo[3 * m + k];
    X.cf[k] = S.coeffs ? S.coeffs[3 * m + k] : (k == 0 ? 1.0 : 0.0);
    X.amb[k] = S.amb ? S.amb[k] : 0.0;
  }
}

__device__ inline void splat_shade(const SplatDev& S, int b, int pix, const double R[3][3], const double e[3],
                                   const SplatPixel& X, double im[3]) {
  im[0] = im[1] = im[2] = 0.0;
  for (int l = 0; l < S.nlights; ++l) {
    double L[3];
    light_cc(S, b, l, R, e, L);
    SplatLight T;
    splat_light(S, l, L, X.p, X.n, X.cdir, X.cdotn, T);
    const double vis = S.vis ? (double)S.vis[(size_t)b * S.vis_vs + (size_t)l * S.N + pix] : 1.0;
    const double w = X.cf[0] * fmax(T.nd, 0.0) + X.cf[1] * splat_pow(fmax(T.rd, 0.0), X.cf[2]);
    const int ci = clampi(S.lcidx[l], 0, S.ncolors - 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) im[ch] += (w * ((double)S.colors[3 * ci + ch] * X.alb[ch])) * vis + X.amb[ch] * X.alb[ch];
  }
}

// sub-pixel s = c K + r of base pixel (i, j): its point on the splat's plane (P.n / r.n) r, t and the unit ray
__device__ __forceinline__ void sub_point(const SplatDev& S, int i, int j, int c, int r, const double P[3],
                                          const double n[3], double pos[3], double ray[3], double& t, double& rn) {
  const double xx = grid_x(S, j) + (sub_shift(S, c) * S.sub_dx) / 2.0;
  const double yy = grid_y(S, i) + (-sub_shift(S, r) * S.sub_dy) / 2.0;
  const double v[3] = {xx, yy, -S.f};
  const double si = unit_inv3(v);
  ray[0] = xx * si; ray[1] = yy * si; ray[2] = -S.f * si;
  const double d0 = (P[0] * n[0] + P[1] * n[1]) + P[2] * n[2];
  rn = (ray[0] * n[0] + ray[1] * n[1]) + ray[2] * n[2];
  t = d0 / rn;
  pos[0] = t * ray[0]; pos[1] = t * ray[1]; pos[2] = t * ray[2];
}

__device__ __forceinline__ void splat_normal(const SplatDev& S, int b, int i, int j, const double P[3], double n[3]) {
  const int pix = i * S.W + j;
  if (S.estimate) {
    PlaneFit F;
    plane_fit(S, b, i, j, P, F);
    n[0] = F.nx * F.s_inv; n[1] = F.ny * F.s_inv; n[2] = F.s_inv;
  } else {
    const float* q = S.normal + (size_t)b * S.nrm_vs + 3 * (size_t)pix;
    n[0] = q[0]; n[1] = q[1]; n[2] = q[2];
  }
}

// Forward: one lane per base pixel of view blockIdx.y.  Outputs (B, KH, KW, {3, 1, 3, 3}); image only if S.shade.
__global__ __launch_bounds__(256) void k_splat_fwd(SplatDev S, float* __restrict__ image, float* __restrict__ depth,
                                                   float* __restrict__ pos_out, float* __restrict__ normal_out) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (pix >= S.N) return;
  const int i = pix / S.W, j = pix - (pix / S.W) * S.W;
  double P[3], dPdZ[3], n[3];
  splat_point(S, b, i, j, P, dPdZ);
  splat_normal(S, b, i, j, P, n);
  const int m = S.mat ? clampi(S.mat[pix], 0, S.nmat - 1) : 0;
  double R[3][3], e[3];
  if (S.shade) splat_basis(S, b, R, e);
  const int KW = S.K * S.W;
  const size_t view = (size_t)b * S.N * S.K * S.K;
#pragma unroll 1
  for (int c = 0; c < S.K; ++c) {
#pragma unroll 1
    for (int r = 0; r < S.K; ++r) {
      double p[3];
      if (S.K == 1) {
        p[0] = P[0]; p[1] = P[1]; p[2] = P[2];
      } else {
        double ray[3], t, rn;
        sub_point(S, i, j, c, r, P, n, p, ray, t, rn);
      }
      const size_t o = view + (size_t)(i * S.K + c) * KW + (size_t)(j * S.K + r);
      depth[o] = (float)sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) { pos_out[3 * o + k] = (float)p[k]; normal_out[3 * o + k] = (float)n[k]; }
      if (S.shade) {
        SplatPixel X;
        splat_pixel(S, p, n, m, X);
        double im[3];
        splat_shade(S, b, pix, R, e, X, im);
#pragma unroll
        for (int k = 0; k < 3; ++k) image[3 * o + k] = (float)fmax(im[k], 0.0);
      }
    }
  }
}

__device__ __forceinline__ void wave_add(float* dst, double v, bool lane0) {
  const float s = wave_sum((float)v);
  if (lane0 && s != 0.0f) atomicAdd(dst, s);
}

// Backward, pass 1: one lane per base pixel.  Upstream gradients (B, KH, KW, {3, 1, 3, 3}), each may be NULL.
// Writes d loss / d light_vis (B, L, N) and, for given normals, d loss / d normal (B, N, 3) and d loss / d z; for
// estimated normals the 9 stencil-slot gradients d loss / d Z go to ws (B, N, 9) for k_splat_gather.
// kView: also the gradient of the view's world-to-camera matrix, twelve sums per workgroup to view_part
// (srh_view_grad.h); every lane reaches the reduce, the dead ones with zeros.  Without kView the trailing argument is
// unused and the code is what it was without it.
template <bool kView>
__global__ __launch_bounds__(256) void k_splat_bwd(SplatDev S, SplatGradsDev G, const float* __restrict__ g_image,
                                                   const float* __restrict__ g_depth, const float* __restrict__ g_pos,
                                                   const float* __restrict__ g_normal, double* __restrict__ ws,
                                                   double* __restrict__ view_part) {
  const int pix0 = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const bool live = pix0 < S.N;
  const int pix = live ? pix0 : 0;                        // dead lanes run with zero upstream gradients (wave sums)
  const bool lane0 = (threadIdx.x & 63) == 0;
  const int i = pix / S.W, j = pix - (pix / S.W) * S.W;
  double P[3], dPdZ[3], n[3];
  splat_point(S, b, i, j, P, dPdZ);
  splat_normal(S, b, i, j, P, n);
  const int m = S.mat ? clampi(S.mat[pix], 0, S.nmat - 1) : 0;
  double R[3][3], e[3];
  if (S.shade) splat_basis(S, b, R, e);
  const int KW = S.K * S.W;
  const size_t view = (size_t)b * S.N * S.K * S.K;
  double gP[3] = {0, 0, 0}, gN[3] = {0, 0, 0};
  double g_alb[3] = {0, 0, 0}, g_cf[3] = {0, 0, 0}, g_amb[3] = {0, 0, 0};
  double vM[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // kView: this lane's sums of g_v (x) l
#pragma unroll 1
  for (int c = 0; c < S.K; ++c) {
#pragma unroll 1
    for (int r = 0; r < S.K; ++r) {
      const int sub = c * S.K + r;
      double p[3], ray[3] = {0, 0, 0}, t = 0.0, rn = 1.0;
      if (S.K == 1) {
        p[0] = P[0]; p[1] = P[1]; p[2] = P[2];
      } else {
        sub_point(S, i, j, c, r, P, n, p, ray, t, rn);
      }
      const size_t o = view + (size_t)(i * S.K + c) * KW + (size_t)(j * S.K + r);
      double gp[3] = {0, 0, 0};
      if (live && g_pos) { gp[0] = g_pos[3 * o]; gp[1] = g_pos[3 * o + 1]; gp[2] = g_pos[3 * o + 2]; }
      if (live && g_normal) { gN[0] += g_normal[3 * o]; gN[1] += g_normal[3 * o + 1]; gN[2] += g_normal[3 * o + 2]; }
      if (live && g_depth) {
        const double dl = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
        const double gd = g_depth[o];
        if (dl > 0.0) {
#pragma unroll
          for (int k = 0; k < 3; ++k) gp[k] += gd * p[k] / dl;
        }
      }
      if (S.shade) {
        SplatPixel X;
        splat_pixel(S, p, n, m, X);
        double im[3];
        splat_shade(S, b, pix, R, e, X, im);
        double g_im[3] = {0, 0, 0};
        if (live && g_image) {
#pragma unroll
          for (int k = 0; k < 3; ++k) g_im[k] = (im[k] > 0.0) ? (double)g_image[3 * o + k] : 0.0;
        }
        double g_n[3] = {0, 0, 0}, g_cd[3] = {0, 0, 0}, g_cdotn = 0.0;
#pragma unroll 1
        for (int l = 0; l < S.nlights; ++l) {
          double L[3];
          light_cc(S, b, l, R, e, L);
          SplatLight T;
          splat_light(S, l, L, X.p, X.n, X.cdir, X.cdotn, T);
          const size_t vi = (size_t)b * S.vis_vs + (size_t)l * S.N + pix;
          const double vl = S.vis ? (double)S.vis[vi] : 1.0;
          const double ndotl = fmax(T.nd, 0.0), rdotc = fmax(T.rd, 0.0);
          const double Pw = splat_pow(rdotc, X.cf[2]);
          const double w = X.cf[0] * ndotl + X.cf[1] * Pw;
          const int ci = clampi(S.lcidx[l], 0, S.ncolors - 1);
          double g_w = 0.0, g_col[3];
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const double col = S.colors[3 * ci + ch];
            g_w += g_im[ch] * col * X.alb[ch];
            g_alb[ch] += g_im[ch] * (w * col * vl + X.amb[ch]);
            g_col[ch] = g_im[ch] * w * X.alb[ch] * vl;
            g_amb[ch] += g_im[ch] * X.alb[ch];
          }
          if (G.vis && live) {                   // dense (B, L, N), whatever the input's view stride
            const double gv = g_w * w;
            float* dv = G.vis + ((size_t)b * S.nlights + l) * S.N + pix;
            *dv = (sub == 0) ? (float)gv : (float)((double)*dv + gv);
          }
          g_w *= vl;
          g_cf[0] += g_w * ndotl;
          g_cf[1] += g_w * Pw;
          if (rdotc > 0.0) g_cf[2] += (g_w * X.cf[1] * Pw) * log(rdotc);
          const double g_nd = (T.nd > 0.0) ? g_w * X.cf[0] : 0.0;
          const double g_rd = (T.rd > 0.0 && X.cf[2] != 0.0) ? g_w * X.cf[1] * X.cf[2] * pow(rdotc, X.cf[2] - 1.0) : 0.0;
          const double g_ldn = g_rd * 2.0 * X.cdotn + g_nd * T.afac;
          g_cdotn += g_rd * 2.0 * T.ldn;
          const double g_cl = -g_rd;
          const double g_afac = g_nd * T.ldn;
          const double g_den = T.den_ok ? -g_afac * T.afac * T.afac : 0.0;
          const double kl = S.latt ? S.latt[3 * l + 1] : 0.0, kq = S.latt ? S.latt[3 * l + 2] : 0.0;
          const double d2 = T.dist * T.dist;
          const double ddp = S.use_quartic ? 4.0 * d2 * T.dist : 2.0 * T.dist;
          const double g_dist = g_den * (kl + kq * ddp);
          double g_lh[3], g_v[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            g_lh[k] = g_ldn * X.n[k] + g_cl * X.cdir[k];
            g_n[k] += g_ldn * T.lh[k];
            g_cd[k] += g_cl * T.lh[k];
          }
          const double proj = (T.lh[0] * g_lh[0] + T.lh[1] * g_lh[1]) + T.lh[2] * g_lh[2];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            g_v[k] = T.nz ? (g_lh[k] - T.lh[k] * proj) / T.dist + g_dist * T.lh[k] : g_lh[k];
            gp[k] -= g_v[k];
          }
          if (kView) view_light_terms(S, b, l, g_v, vM);
          if (G.lpos) {                          // L = R^T (l_xyz - l_w eye): d/dl_xyz = R g_v, d/dl_w = -eye . R g_v
            double gl[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) gl[k] = (R[k][0] * g_v[0] + R[k][1] * g_v[1]) + R[k][2] * g_v[2];
            float* dst = G.lpos + (size_t)b * S.lpos_vs + 4 * (size_t)l;
#pragma unroll
            for (int k = 0; k < 3; ++k) wave_add(dst + k, gl[k], lane0);
            wave_add(dst + 3, -((e[0] * gl[0] + e[1] * gl[1]) + e[2] * gl[2]), lane0);
          }
          if (G.colors) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) wave_add(G.colors + 3 * ci + ch, g_col[ch], lane0);
          }
          if (G.latt) {
            wave_add(G.latt + 3 * l, g_den, lane0);
            wave_add(G.latt + 3 * l + 1, g_den * T.dist, lane0);
            wave_add(G.latt + 3 * l + 2, g_den * T.dp, lane0);
          }
        }
        // the view direction cdir = -unit(p) and cdotn = cdir . n
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          g_cd[k] += g_cdotn * X.n[k];
          g_n[k] += g_cdotn * X.cdir[k];
        }
        const double pc = (X.p[0] * g_cd[0] + X.p[1] * g_cd[1]) + X.p[2] * g_cd[2];
        const double si = X.s_inv;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          gp[k] -= g_cd[k] * si - X.p[k] * pc * si * si * si;
          gN[k] += g_n[k];
        }
      }
      if (S.K == 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) gP[k] += gp[k];
      } else {                                  // pos = t ray, t = (P . n) / (ray . n)
        const double g_t = (gp[0] * ray[0] + gp[1] * ray[1]) + gp[2] * ray[2];
        const double g_d0 = g_t / rn, g_rn = -g_t * t / rn;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          gN[k] += g_rn * ray[k] + g_d0 * P[k];
          gP[k] += g_d0 * n[k];
        }
      }
    }
  }
  if (S.shade) {
    const int m0 = __builtin_amdgcn_readfirstlane(m);
    const bool uniform = __builtin_amdgcn_ballot_w64(live && m != m0) == 0ull;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (G.amb) wave_add(G.amb + ch, g_amb[ch], lane0);
      if (uniform) {
        if (G.albedo) wave_add(G.albedo + 3 * m0 + ch, g_alb[ch], lane0);
        if (G.coeffs) wave_add(G.coeffs + 3 * m0 + ch, g_cf[ch], lane0);
      } else if (live) {
        if (G.albedo && g_alb[ch] != 0.0) atomicAdd(G.albedo + 3 * m + ch, (float)g_alb[ch]);
        if (G.coeffs && g_cf[ch] != 0.0) atomicAdd(G.coeffs + 3 * m + ch, (float)g_cf[ch]);
      }
    }
  }
  if (kView) view_block_reduce<kViewSums>([&](int k) { return vM[k]; }, view_part);   // once, after both loops
  if (!live) return;
  const double z = load_z(S, b, pix);
  const size_t zo = ((size_t)b * S.N + pix) * S.pos_cols;
  if (S.estimate) {
    if (!ws) return;                            // no z gradient wanted
    PlaneFit F;
    plane_fit(S, b, i, j, P, F);
    double gZ[9];
    plane_fit_bwd(S, b, i, j, P, F, gN, gP, gZ);
    double* dst = ws + ((size_t)b * S.N + pix) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k] = gZ[k];
  } else {
    if (G.normal) {
      float* dst = G.normal + ((size_t)b * S.N + pix) * 3;
      dst[0] = (float)gN[0]; dst[1] = (float)gN[1]; dst[2] = (float)gN[2];
    }
    if (G.pos) {
      const double gZ = (gP[0] * dPdZ[0] + gP[1] * dPdZ[1]) + gP[2] * dPdZ[2];
      for (int k = 0; k < S.pos_cols; ++k) G.pos[zo + k] = 0.0f;
      G.pos[zo + S.pos_cols - 1] = (z < 0.0) ? (float)gZ : 0.0f;
    }
  }
}

// Backward, pass 2 (estimated normals): d loss / d z of splat q = sum of the stencil slots of its neighbours p that
// land on q after reflection, times dZ/dz = [z < 0].
__global__ __launch_bounds__(256) void k_splat_gather(SplatDev S, float* __restrict__ g_pos, const double* __restrict__ ws) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (pix >= S.N) return;
  const int qi = pix / S.W, qj = pix - (pix / S.W) * S.W;
  double g = 0.0;
  for (int pi = qi - 1; pi <= qi + 1; ++pi) {
    if (pi < 0 || pi >= S.H) continue;
    for (int pj = qj - 1; pj <= qj + 1; ++pj) {
      if (pj < 0 || pj >= S.W) continue;
      const double* src = ws + ((size_t)b * S.N + (size_t)pi * S.W + pj) * 9;
      for (int k = 0; k < 9; ++k)
        if (reflect_idx(pi + k / 3 - 1, S.H) == qi && reflect_idx(pj + k % 3 - 1, S.W) == qj) g += src[k];
    }
  }
  const double z = load_z(S, b, pix);
  const size_t zo = ((size_t)b * S.N + pix) * S.pos_cols;
  for (int k = 0; k < S.pos_cols; ++k) g_pos[zo + k] = 0.0f;
  g_pos[zo + S.pos_cols - 1] = (z < 0.0) ? (float)g : 0.0f;
}

}  // namespace srh
