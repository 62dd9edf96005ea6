// The reference's backward-warp ("pull") re-projection, projection_reverse_renderer (diffrend/torch/
// projection_layer.py:281-333 with project_image_coordinates :45-85 and torch's grid_sample: bilinear, zero padding,
// align_corners = False), forward and analytic backward; many views per launch (the view is grid dimension y).  See
// DESIGN.md "The reverse re-projection layer".
//
// Per view, N = W H pixels q with a target-view surfel o_q (out_pos_wc) and a source-view surfel i_q (in_pos_wc), and the
// source image rgb (D channels per texel).  P(p, cam) = (u, v, z): u = fsx X / nz(Z) + W/2 - 1/2, v likewise, z = -Z,
// with (X, Y, Z) = M [p, 1] -- proj_surfel's coordinates, which are the reference's pixel coordinate minus 1/2, i.e. the
// texel coordinate grid_sample reads at.  S(f, (u, v)) is the bilinear sample of the plane f there, texels outside the
// frame counting 0.
//   c1 = P(o_q, camera1), c2 = P(i_q, camera2)
//   image1 = S(rgb, c1.uv)
//   d = c1.z, d_in = S(d, c2.uv), d_out = S(d_in, c1.uv)
//   mask = !(v1 < 0 | u1 < 0 | v1 >= H - 1 | u1 >= W - 1) (d <= d_out + eps) keep
//   out = mask image1 + (1 - mask) rotated        depth = S(q -> c2.z, c1.uv)
//
// Forward, two launches: k_rproj_depth_in (d_in; the four d it reads are recomputed from out_pos, one row of the view
// matrix each) -> k_rproj_fwd (everything else; the four c2.z likewise).  Nothing is kept for the backward but the mask,
// which is an output.
//
// Backward: k_rproj_pixel_bwd (per pixel: grad rotated, grad out_pos through the sample coordinates of image1 and of
// the new depth, and the planes the texels gather) -> k_rproj_texel_bwd (one lane per source texel walks the lists of
// its four cells in list order: grad rgb and, through the values of the new depth, grad in_pos).  The lists are
// srh_projection.h's: k_proj_keys keys every pixel by its sample cell on the (W + 1) x (H + 1) grid and records (fx, fy),
// the caller orders the keys, k_proj_mark marks each cell's range.  fp64 arithmetic, fp32 results, no float atomic,
// every gradient element written once.
#pragma once
#include "srh_projection.h"

namespace srh {

struct RProjDev {
  int B, W, H, N, D, ncell, nblk;
  double fsx[2], fsy[2], cx0, cy0, eps;    // [0] camera1, [1] camera2
};

// G planes of the backward, channel-major (B, D + 1, N) fp64: the gradient reaching image1 (D channels), then the
// upstream gradient of the new depth.
__host__ __device__ __forceinline__ size_t rproj_plane(const RProjDev& R, int b, int ch, int q) {
  return ((size_t)b * (R.D + 1) + ch) * R.N + q;
}

// the sample cell is texels (ix, iy) .. (ix + 1, iy + 1); live = at least one of them can be in the frame
using RProjPoint = ProjPoint;

__host__ __device__ __forceinline__ double rproj_row(const double* M, int r, const float* p) {
  return ((M[4 * r] * (double)p[0] + M[4 * r + 1] * (double)p[1]) + M[4 * r + 2] * (double)p[2]) + M[4 * r + 3];
}

// proj_surfel's point for camera `cam`
__host__ __device__ __forceinline__ RProjPoint rproj_point(const RProjDev& R, int cam, const double* M, const float* p) {
  return proj_point(R.fsx[cam], R.fsy[cam], R.cx0, R.cy0, R.W, R.H, M, p);
}

// texel k = 2 dx + dy of the cell of S: its index in the frame, or -1
__host__ __device__ __forceinline__ int rproj_texel(const RProjDev& R, const RProjPoint& S, int k) {
  const int x = S.ix + (k >> 1), y = S.iy + (k & 1);
  return (S.live && x >= 0 && x < R.W && y >= 0 && y < R.H) ? y * R.W + x : -1;
}

// Forward 1: d_in (B, N) fp64 = S(d, c2.uv), one lane per pixel; d of a texel t = -(row 2 of view1) . [out_pos_t, 1].
__global__ __launch_bounds__(kProjBlock) void k_rproj_depth_in(RProjDev R, const double* __restrict__ view1,
                                                               const double* __restrict__ view2,
                                                               const float* __restrict__ in_pos,
                                                               const float* __restrict__ out_pos,
                                                               double* __restrict__ d_in) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= R.N) return;
  const size_t base = (size_t)b * R.N;
  double M1[12], M2[12];
  proj_load_view(view1, b, M1);
  proj_load_view(view2, b, M2);
  const RProjPoint S = rproj_point(R, 1, M2, in_pos + 3 * (base + q));
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = rproj_texel(R, S, k);
    if (t >= 0) acc += -rproj_row(M1, 2, out_pos + 3 * (base + t)) * proj_beta(k, S.fx, S.fy);
  }
  d_in[base + q] = acc;
}

// Forward 2: one lane per pixel.  rotated, keep (B, N) and depth may be NULL; out is written only with `rotated`.
__global__ __launch_bounds__(kProjBlock) void k_rproj_fwd(RProjDev R, const double* __restrict__ view1,
                                                          const double* __restrict__ view2,
                                                          const float* __restrict__ rgb, const float* __restrict__ in_pos,
                                                          const float* __restrict__ out_pos,
                                                          const float* __restrict__ rotated,
                                                          const float* __restrict__ keep,
                                                          const double* __restrict__ d_in, float* __restrict__ out,
                                                          float* __restrict__ mask, float* __restrict__ image1,
                                                          float* __restrict__ depth) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= R.N) return;
  const size_t base = (size_t)b * R.N, o = base + q;
  double M1[12], M2[12];
  proj_load_view(view1, b, M1);
  proj_load_view(view2, b, M2);
  const RProjPoint S = rproj_point(R, 0, M1, out_pos + 3 * o);
  double val[kProjMaxD], d_out = 0.0, dep = 0.0;
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) val[c] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = rproj_texel(R, S, k);
    if (t < 0) continue;
    const double wgt = proj_beta(k, S.fx, S.fy);
    const float* e = rgb + (base + t) * R.D;
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c)
      if (c < R.D) val[c] += (double)e[c] * wgt;
    d_out += d_in[base + t] * wgt;
    if (depth) dep += -rproj_row(M2, 2, in_pos + 3 * (base + t)) * wgt;
  }
  // the reference's frame test on pixel coordinate = u + 1/2, literally: a NaN coordinate passes it
  const bool outside = S.v < 0.0 || S.u < 0.0 || S.v >= (double)(R.H - 1) || S.u >= (double)(R.W - 1);
  double m = (!outside && -S.Z <= d_out + R.eps) ? 1.0 : 0.0;
  if (keep) m *= (double)keep[o];
  mask[o] = (float)m;
  if (depth) depth[o] = (float)dep;
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    if (c >= R.D) continue;
    image1[o * R.D + c] = (float)val[c];
    if (rotated) out[o * R.D + c] = (float)(m * val[c] + (1.0 - m) * (double)rotated[o * R.D + c]);
  }
}

// Backward 1: one lane per pixel.  Upstream gradients fp32, NULL = none (g_out only with a rotated image: without one
// `out` is image1).  gpl (G planes), g_out_pos (B, N, 3) and g_rot (B, N, D) may be NULL = not wanted.
// kView: also the gradient of camera 1's matrix, which reaches the results through the sample coordinates alone (d,
// d_in and d_out feed only the mask): g_M1 = sum_q g_cc1 (x) [out_pos_q, 1] with g_cc1 = (g_X, g_Y, g_Z) below, zeros
// for a sample outside the frame.  The lane keeps g_cc1 and the point (vg, vp), and each workgroup stores the sums of
// their 12 products to view_part (srh_view_grad.h).  Without kView the trailing argument is unused and the code is what
// it was without it.
template <bool kView>
__global__ __launch_bounds__(kProjBlock) void k_rproj_pixel_bwd(RProjDev R, const double* __restrict__ view1,
                                                                const double* __restrict__ view2,
                                                                const float* __restrict__ rgb,
                                                                const float* __restrict__ in_pos,
                                                                const float* __restrict__ out_pos,
                                                                const float* __restrict__ mask,
                                                                const float* __restrict__ g_out,
                                                                const float* __restrict__ g_image1,
                                                                const float* __restrict__ g_depth,
                                                                double* __restrict__ gpl, float* __restrict__ g_out_pos,
                                                                float* __restrict__ g_rot,
                                                                double* __restrict__ view_part) {
  const int q = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  double vg[3] = {0.0, 0.0, 0.0}, vp[3] = {0.0, 0.0, 0.0};      // kView: g_cc and the point; zeros bring zeros
  do {                                  // a lane that is done leaves by `break`: with kView every lane reaches the reduce
  if (q >= R.N) break;
  const size_t base = (size_t)b * R.N, o = base + q;
  const double m = (double)mask[o];
  double G[kProjMaxD];
#pragma unroll
  for (int c = 0; c < kProjMaxD; ++c) {
    G[c] = 0.0;
    if (c >= R.D) continue;
    const double go = g_out ? (double)g_out[o * R.D + c] : 0.0;
    G[c] = (g_image1 ? (double)g_image1[o * R.D + c] : 0.0) + m * go;
    if (g_rot) g_rot[o * R.D + c] = (float)((1.0 - m) * go);
    if (gpl) gpl[rproj_plane(R, b, c, q)] = G[c];
  }
  const double gd = g_depth ? (double)g_depth[o] : 0.0;
  if (gpl) gpl[rproj_plane(R, b, R.D, q)] = gd;
  if (!kView && !g_out_pos) break;
  double M1[12], M2[12];
  proj_load_view(view1, b, M1);
  proj_load_view(view2, b, M2);
  const RProjPoint S = rproj_point(R, 0, M1, out_pos + 3 * o);
  double g_u = 0.0, g_v = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = rproj_texel(R, S, k);
    if (t < 0) continue;                       // a texel outside the frame has no coordinate gradient either
    const float* e = rgb + (base + t) * R.D;
    double T = g_depth ? gd * -rproj_row(M2, 2, in_pos + 3 * (base + t)) : 0.0;
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c)
      if (c < R.D) T += G[c] * (double)e[c];
    g_u += T * ((k & 2) ? 1.0 : -1.0) * ((k & 1) ? S.fy : 1.0 - S.fy);
    g_v += T * ((k & 1) ? 1.0 : -1.0) * ((k & 2) ? S.fx : 1.0 - S.fx);
  }
  const double g_X = g_u * R.fsx[0] / S.Zd, g_Y = g_v * R.fsy[0] / S.Zd;
  const double g_Z = S.Z != 0.0 ? -(g_X * S.X + g_Y * S.Y) / S.Zd : 0.0;
  if (kView && S.live) {
    vg[0] = g_X; vg[1] = g_Y; vg[2] = g_Z;
#pragma unroll
    for (int c = 0; c < 3; ++c) vp[c] = (double)out_pos[3 * o + c];
  }
  if (kView && !g_out_pos) break;
#pragma unroll
  for (int j = 0; j < 3; ++j) g_out_pos[3 * o + j] = (float)((M1[j] * g_X + M1[4 + j] * g_Y) + M1[8 + j] * g_Z);
  } while (false);
  if (kView) view_block_reduce<kViewSums>([&](int k) { return view_outer_term(vg, vp, k); }, view_part);
}

constexpr int kRProjView2Sums = 4, kRProjView2First = 8;     // what camera 2 gets: row 2 of the 3 x 4 matrix

// Backward 2: one lane per source texel t walks the lists of its four cells -- t is corner k of the cell at t - (dx, dy)
// -- and accumulates in list order.  rec (B, N, 4) fp64 as k_proj_keys wrote it (fx, fy first), order and range as for
// k_proj_gather.  g_rgb (B, N, D) and g_in_pos (B, N, 3) are written, each element once; either may be NULL.
// kView: also the gradient of camera 2's matrix, which reaches the results through the values of the new depth alone,
// c2.z = -(row 2 of M2) . [in_pos, 1]: row 2 of g_M2 = -sum_t g_z(t) [in_pos_t, 1] with g_z(t) the depth channel
// accumulated below; rows 0 and 1 are exactly 0 (k_view_finish writes them).  The lane's 4 products go to cs, and each
// workgroup stores its sums to view_part (srh_view_grad.h); g_rgb and g_in_pos may then both be NULL.  Without kView
// in_pos and the trailing argument are unused and the code is what it was without them.
template <bool kView>
__global__ __launch_bounds__(kProjBlock) void k_rproj_texel_bwd(RProjDev R, const double* __restrict__ view2,
                                                                const double* __restrict__ rec,
                                                                const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ range,
                                                                const double* __restrict__ gpl,
                                                                float* __restrict__ g_rgb, float* __restrict__ g_in_pos,
                                                                const float* __restrict__ in_pos,
                                                                double* __restrict__ view_part) {
  const int t = blockIdx.x * kProjBlock + threadIdx.x;
  const int b = blockIdx.y;
  double cs[kRProjView2Sums] = {0.0, 0.0, 0.0, 0.0};
  do {                                  // with kView every lane reaches the reduce
  if (t >= R.N) break;
  const int ty = t / R.W, tx = t - ty * R.W;
  const size_t base = (size_t)b * R.N;
  double acc[kProjMaxD + 1];
#pragma unroll
  for (int c = 0; c < kProjMaxD + 1; ++c) acc[c] = 0.0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int cell = (ty - (k & 1) + 1) * (R.W + 1) + (tx - (k >> 1) + 1);
    const int32_t* r = range + ((size_t)b * R.ncell + cell) * 2;
    const int i0 = r[0], i1 = r[1];
    for (int i = i0; i < i1; ++i) {
      const int32_t s = order[base + i];
      if ((uint32_t)s >= (uint32_t)R.N) continue;
      const double* e = rec + 4 * (base + s);
      const double wgt = proj_beta(k, e[0], e[1]);
      const double* g = gpl + rproj_plane(R, b, 0, s);
#pragma unroll
      for (int c = 0; c < kProjMaxD; ++c)
        if (c < R.D) acc[c] += g[(size_t)c * R.N] * wgt;
      acc[kProjMaxD] += g[(size_t)R.D * R.N] * wgt;
    }
  }
  if (g_rgb) {
#pragma unroll
    for (int c = 0; c < kProjMaxD; ++c)
      if (c < R.D) g_rgb[(base + t) * R.D + c] = (float)acc[c];
  }
  if (g_in_pos) {
    const auto* m2 = as_constant(view2) + (size_t)b * 12;
#pragma unroll
    for (int j = 0; j < 3; ++j) g_in_pos[3 * (base + t) + j] = (float)(-m2[8 + j] * acc[kProjMaxD]);
  }
  if (kView) {
    const float* p = in_pos + 3 * (base + t);
#pragma unroll
    for (int c = 0; c < 3; ++c) cs[c] = -acc[kProjMaxD] * (double)p[c];
    cs[3] = -acc[kProjMaxD];
  }
  } while (false);
  if (kView) view_block_reduce<kRProjView2Sums>([&](int k) { return cs[k]; }, view_part);
}
}  // namespace srh
