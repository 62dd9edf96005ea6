// The reference's third renderer, render_splats_NDC (diffrend/torch/renderer.py:358-474): one splat per pixel, given by
// its position in normalised device coordinates and a normal; un-projected, shaded where it lies -- no intersection, no
// occlusion, no near / far mask, no tonemap.  Forward and analytic backward, many views per launch (the view is grid
// dimension y).  See DESIGN.md "The NDC splat renderer".
//
//   un-projection  q = (x / m00, y / m11, -w, (z - m22 w) / m23),  P = q.xyz / q.w   (inv_perspective_RH_NO; w = 1 for
//                  three-column positions); m00 .. m23 come from the host in double
//   depth          |P|
//   normal         the given normal, as it is: neither transformed nor normalised
//   shading        the torch backend's Phong with cam_dir = -P, NOT normalised (the along-ray renderer normalises it),
//                  double_sided honoured: sgn = sign(cam_dir . n) multiplies the diffuse and the specular dot before
//                  their relus; lights in camera coordinates as in srh_splat.h; relu over the light sum
// Everything is computed in fp64 and stored as fp32, one lane per splat.  The light and material arithmetic is
// srh_splat.h's (splat_basis, light_cc, splat_light, splat_pow); what differs -- the view direction and its derivative
// with respect to P, double_sided, the four-column un-projection -- is here.
//
// Backward (k_splat_ndc_bwd): d loss / d pos (all pos_cols columns) and d loss / d normal are WRITTEN, each element by
// the lane that owns the splat: no atomics, no zero-fill, no workspace, identical from run to run.  Scene parameters
// (lights, colours, materials) are reduced over the wave and added with fp32 atomics exactly as k_splat_bwd does.
#pragma once
#include "srh_splat.h"

namespace srh {

struct SplatNdcDev {
  SplatDev S;                 // B, W, H, N, pos_cols (3 | 4), shade, use_quartic, the camera, lights and materials
  int double_sided;
  double m00, m11, m22, m23;  // perspective_NO_params(fovy, W / H, near, far)
};

struct SplatNdcPoint {
  double P[3], q3;
};

// NDC -> camera coordinates of splat `pix` of view b
__device__ __forceinline__ void ndc_point(const SplatNdcDev& D, int b, int pix, SplatNdcPoint& U) {
  const float* s = D.S.pos + (size_t)b * D.S.pos_vs + (size_t)pix * D.S.pos_cols;
  const double x = s[0], y = s[1], z = s[2], w = (D.S.pos_cols == 4) ? (double)s[3] : 1.0;
  U.q3 = (z - D.m22 * w) / D.m23;
  U.P[0] = (x / D.m00) / U.q3; U.P[1] = (y / D.m11) / U.q3; U.P[2] = -w / U.q3;
}

// d loss / d (x, y, z, w) from d loss / d P
__device__ __forceinline__ void ndc_point_bwd(const SplatNdcDev& D, const SplatNdcPoint& U, const double gP[3],
                                              double g[4]) {
  const double g_q3 = -((gP[0] * U.P[0] + gP[1] * U.P[1]) + gP[2] * U.P[2]) / U.q3;
  g[0] = (gP[0] / U.q3) / D.m00;
  g[1] = (gP[1] / U.q3) / D.m11;
  g[2] = g_q3 / D.m23;
  g[3] = -(gP[2] / U.q3) - g_q3 * (D.m22 / D.m23);
}

// what the light loops read of one splat: the view direction is -P as it is, sgn its side of the normal
__device__ inline void ndc_pixel(const SplatNdcDev& D, const double p[3], const double n[3], int m, SplatPixel& X,
                                 double& sgn) {
  const SplatDev& S = D.S;
#pragma unroll
  for (int k = 0; k < 3; ++k) { X.p[k] = p[k]; X.n[k] = n[k]; X.cdir[k] = -p[k]; }
  X.s_inv = 1.0;
  X.cdotn = (X.cdir[0] * n[0] + X.cdir[1] * n[1]) + X.cdir[2] * n[2];
  sgn = D.double_sided ? (X.cdotn > 0.0 ? 1.0 : (X.cdotn < 0.0 ? -1.0 : 0.0)) : 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    X.alb[k] = S.albedo[3 * m + k];
    X.cf[k] = S.coeffs ? S.coeffs[3 * m + k] : (k == 0 ? 1.0 : 0.0);
    X.amb[k] = S.amb ? S.amb[k] : 0.0;
  }
}

__device__ inline void ndc_shade(const SplatNdcDev& D, int b, const double R[3][3], const double e[3],
                                 const SplatPixel& X, double sgn, double im[3]) {
  const SplatDev& S = D.S;
  im[0] = im[1] = im[2] = 0.0;
  for (int l = 0; l < S.nlights; ++l) {
    double L[3];
    light_cc(S, b, l, R, e, L);
    SplatLight T;
    splat_light(S, l, L, X.p, X.n, X.cdir, X.cdotn, T);
    const double w = X.cf[0] * fmax(sgn * T.nd, 0.0) + X.cf[1] * splat_pow(fmax(sgn * T.rd, 0.0), X.cf[2]);
    const int ci = clampi(S.lcidx[l], 0, S.ncolors - 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) im[ch] += w * ((double)S.colors[3 * ci + ch] * X.alb[ch]) + X.amb[ch] * X.alb[ch];
  }
}

__device__ __forceinline__ void ndc_normal(const SplatDev& S, int b, int pix, double n[3]) {
  const float* q = S.normal + (size_t)b * S.nrm_vs + 3 * (size_t)pix;
  n[0] = q[0]; n[1] = q[1]; n[2] = q[2];
}

// Forward: one lane per splat of view blockIdx.y.  image (B, N, 3) only if shade; depth (B, N), pos (B, N, 3).
__global__ __launch_bounds__(256) void k_splat_ndc_fwd(SplatNdcDev D, float* __restrict__ image,
                                                       float* __restrict__ depth, float* __restrict__ pos_out) {
  const SplatDev& S = D.S;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (pix >= S.N) return;
  SplatNdcPoint U;
  ndc_point(D, b, pix, U);
  const size_t o = (size_t)b * S.N + pix;
  depth[o] = (float)sqrt((U.P[0] * U.P[0] + U.P[1] * U.P[1]) + U.P[2] * U.P[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) pos_out[3 * o + k] = (float)U.P[k];
  if (!S.shade) return;
  double n[3], R[3][3], e[3], sgn, im[3];
  ndc_normal(S, b, pix, n);
  splat_basis(S, b, R, e);
  const int m = S.mat ? clampi(S.mat[pix], 0, S.nmat - 1) : 0;
  SplatPixel X;
  ndc_pixel(D, U.P, n, m, X, sgn);
  ndc_shade(D, b, R, e, X, sgn, im);
#pragma unroll
  for (int k = 0; k < 3; ++k) image[3 * o + k] = (float)fmax(im[k], 0.0);
}

// Backward: one lane per splat.  Upstream gradients image (B, N, 3), depth (B, N), pos (B, N, 3), each may be NULL.
// Writes G.pos (B, N, pos_cols) and G.normal (B, N, 3); adds the scene parameters' gradients (G.vis is not used).
// kView: also the gradient of the view's world-to-camera matrix, as k_splat_bwd<true> forms it: twelve fp64 sums per
// lane over the lights, one view_block_reduce after the loop (zeros without an image gradient).  Without kView the
// trailing argument is unused and the code is what it was without it.
template <bool kView>
__global__ __launch_bounds__(256) void k_splat_ndc_bwd(SplatNdcDev D, SplatGradsDev G, const float* __restrict__ g_image,
                                                       const float* __restrict__ g_depth,
                                                       const float* __restrict__ g_pos,
                                                       double* __restrict__ view_part) {
  const SplatDev& S = D.S;
  const int pix0 = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const bool live = pix0 < S.N;
  const int pix = live ? pix0 : 0;                        // dead lanes run with zero upstream gradients (wave sums)
  const bool lane0 = (threadIdx.x & 63) == 0;
  SplatNdcPoint U;
  ndc_point(D, b, pix, U);
  const size_t o = (size_t)b * S.N + pix;
  double gp[3] = {0, 0, 0}, gN[3] = {0, 0, 0};
  double vM[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // kView: this lane's sums of g_v (x) l
  if (live && g_pos) { gp[0] = g_pos[3 * o]; gp[1] = g_pos[3 * o + 1]; gp[2] = g_pos[3 * o + 2]; }
  if (live && g_depth) {
    const double dl = sqrt((U.P[0] * U.P[0] + U.P[1] * U.P[1]) + U.P[2] * U.P[2]);
    const double gd = g_depth[o];
    if (dl > 0.0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) gp[k] += gd * U.P[k] / dl;
    }
  }
  if (S.shade && g_image) {                               // without an image gradient nothing of the shading is wanted
    double n[3], R[3][3], e[3], sgn, im[3];
    ndc_normal(S, b, pix, n);
    splat_basis(S, b, R, e);
    const int m = S.mat ? clampi(S.mat[pix], 0, S.nmat - 1) : 0;
    SplatPixel X;
    ndc_pixel(D, U.P, n, m, X, sgn);
    ndc_shade(D, b, R, e, X, sgn, im);
    double g_im[3] = {0, 0, 0};
    if (live) {
#pragma unroll
      for (int k = 0; k < 3; ++k) g_im[k] = (im[k] > 0.0) ? (double)g_image[3 * o + k] : 0.0;
    }
    double g_alb[3] = {0, 0, 0}, g_cf[3] = {0, 0, 0}, g_amb[3] = {0, 0, 0};
    double g_n[3] = {0, 0, 0}, g_cd[3] = {0, 0, 0}, g_cdotn = 0.0;
#pragma unroll 1
    for (int l = 0; l < S.nlights; ++l) {
      double L[3];
      light_cc(S, b, l, R, e, L);
      SplatLight T;
      splat_light(S, l, L, X.p, X.n, X.cdir, X.cdotn, T);
      const double snd = sgn * T.nd, srd = sgn * T.rd;    // the sign itself has no gradient
      const double ndotl = fmax(snd, 0.0), rdotc = fmax(srd, 0.0);
      const double Pw = splat_pow(rdotc, X.cf[2]);
      const double w = X.cf[0] * ndotl + X.cf[1] * Pw;
      const int ci = clampi(S.lcidx[l], 0, S.ncolors - 1);
      double g_w = 0.0, g_col[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double col = S.colors[3 * ci + ch];
        g_w += g_im[ch] * col * X.alb[ch];
        g_alb[ch] += g_im[ch] * (w * col + X.amb[ch]);
        g_col[ch] = g_im[ch] * w * X.alb[ch];
        g_amb[ch] += g_im[ch] * X.alb[ch];
      }
      g_cf[0] += g_w * ndotl;
      g_cf[1] += g_w * Pw;
      if (rdotc > 0.0) g_cf[2] += (g_w * X.cf[1] * Pw) * log(rdotc);
      const double g_nd = (snd > 0.0) ? sgn * (g_w * X.cf[0]) : 0.0;
      const double g_rd = (srd > 0.0 && X.cf[2] != 0.0) ? sgn * (g_w * X.cf[1] * X.cf[2] * pow(rdotc, X.cf[2] - 1.0)) : 0.0;
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
      if (G.lpos) {                              // L = R^T (l_xyz - l_w eye): d/dl_xyz = R g_v, d/dl_w = -eye . R g_v
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
    // the view direction cdir = -P (not normalised) and cdotn = cdir . n
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gp[k] -= g_cd[k] + g_cdotn * X.n[k];
      gN[k] += g_n[k] + g_cdotn * X.cdir[k];
    }
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
  if (kView) view_block_reduce<kViewSums>([&](int k) { return vM[k]; }, view_part);   // once, after the loop
  if (!live) return;
  if (G.normal) {
    float* dst = G.normal + 3 * o;
    dst[0] = (float)gN[0]; dst[1] = (float)gN[1]; dst[2] = (float)gN[2];
  }
  if (G.pos) {
    double g[4];
    ndc_point_bwd(D, U, gp, g);
    float* dst = G.pos + o * S.pos_cols;
    dst[0] = (float)g[0]; dst[1] = (float)g[1]; dst[2] = (float)g[2];
    if (S.pos_cols == 4) dst[3] = (float)g[3];
  }
}

}  // namespace srh
