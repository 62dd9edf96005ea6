// The depth-map-to-surfels front end of the reference's re-projection loops (diffrend/torch/projection_layer.py:749-750:
// cam_to_world_batched(z_to_pcl_CC_batched(-depth, camera), None, camera)['pos'], torch/renderer.py:510-534 and
// torch/utils.py:622-647 with lookat_inv), forward and analytic backward; many views per launch (the view is grid
// dimension y).  See DESIGN.md "The depth lift and the hard projection".
//
// Per view, N = W H pixels q = i W + j with a depth (positive in front of the camera, the reference's -z):
//   d = max(depth, 0)                               torch's relu: a NaN stays a NaN
//   grid   x_j = fp32(linspace(-1, 1, W)_j w / 2),  y_i = fp32(linspace(1, -1, H)_i h / 2)   -- srh_splat.h's grid
//   P_cc = (d x_j / f, d y_i / f, -d)
//   P_wc = R P_cc + eye                             [R | eye] = the view's 3 x 4 camera-to-world matrix, fp64, made by
//                                                   the host
// Backward: g_depth = g_P . dP/dd with dP_cc/dd = (x_j / f, y_i / f, -1), exactly 0 where depth <= 0.
//
// One lane per pixel in both directions; every element written once, no atomic, fp64 arithmetic, one fp32 store per
// element.  Memory-bound: the forward reads 4 B and writes 12 B per lane, and the 12 B of consecutive lanes are
// contiguous.
#pragma once
#include "srh_projection.h"   // proj_load_view
#include "srh_view_grad.h"

namespace srh {

constexpr int kSurfBlock = 256;
constexpr int kSurfFrameCamera = 0, kSurfFrameWorld = 1;

struct SurfDev {
  int B, W, H, N, frame, nblk;
  double f, half_w, half_h, step_x, step_y;
};

// numpy's linspace (i * step + start, the last sample exactly the end point, a single sample the start point) times the
// half extent, rounded once to fp32: the arithmetic of srh_splat.h's grid_x / grid_y, so both place the same points
__host__ __device__ __forceinline__ double surf_grid_x(const SurfDev& S, int j) {
  const double s = (S.W == 1) ? -1.0 : ((j == S.W - 1) ? 1.0 : (j * S.step_x + -1.0));
  return (double)(float)(s * S.half_w);
}
__host__ __device__ __forceinline__ double surf_grid_y(const SurfDev& S, int i) {
  const double s = (S.H == 1) ? 1.0 : ((i == S.H - 1) ? -1.0 : (i * S.step_y + 1.0));
  return (double)(float)(s * S.half_h);
}

// dP_cc / dd of pixel q
__host__ __device__ __forceinline__ void surf_dir(const SurfDev& S, int q, double dir[3]) {
  const int i = q / S.W, j = q - i * S.W;
  dir[0] = surf_grid_x(S, j); dir[1] = surf_grid_y(S, i); dir[2] = -1.0;
}

// depth (B, N) fp32 -> out (B, N, 3) fp32; view (B, 12) fp64 is read only for the world frame
__global__ __launch_bounds__(kSurfBlock) void k_surfels_fwd(SurfDev S, const double* __restrict__ view,
                                                            const float* __restrict__ depth, float* __restrict__ out) {
  const int q = blockIdx.x * kSurfBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= S.N) return;
  const size_t o = (size_t)b * S.N + q;
  const double z = (double)depth[o];
  const double d = (z <= 0.0) ? 0.0 : z;
  double dir[3];
  surf_dir(S, q, dir);
  double P[3] = {(d * dir[0]) / S.f, (d * dir[1]) / S.f, -d};
  if (S.frame == kSurfFrameWorld) {
    double M[12];
    proj_load_view(view, b, M);
    const double X = P[0], Y = P[1], Z = P[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r] = ((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) out[3 * o + r] = (float)P[r];
}

// g_out (B, N, 3) fp32 -> g_depth (B, N) fp32, every element written.
// kView (world frame only): also the gradient of the view's matrix M = [R | eye].  P_wc = R P_cc + eye, so columns 0-2
// are sum_q g_P (x) P_cc and column 3 is sum_q g_P; a pixel with depth <= 0 has P_cc = 0 and still moves with the eye.
// Each workgroup stores its 12 sums to view_part (srh_view_grad.h); g_depth may then be NULL = not wanted.  Without
// kView the trailing argument is unused and the code is what it was without it.
template <bool kView>
__global__ __launch_bounds__(kSurfBlock) void k_surfels_bwd(SurfDev S, const double* __restrict__ view,
                                                            const float* __restrict__ depth,
                                                            const float* __restrict__ g_out,
                                                            float* __restrict__ g_depth,
                                                            double* __restrict__ view_part) {
  const int q = blockIdx.x * kSurfBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (!kView) {
    if (q >= S.N) return;
    const size_t o = (size_t)b * S.N + q;
    if ((double)depth[o] <= 0.0) {
      g_depth[o] = 0.0f;
      return;
    }
    double G[3] = {(double)g_out[3 * o], (double)g_out[3 * o + 1], (double)g_out[3 * o + 2]};
    if (S.frame == kSurfFrameWorld) {            // R^T g
      double M[12];
      proj_load_view(view, b, M);
      const double gx = G[0], gy = G[1], gz = G[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) G[c] = (M[c] * gx + M[4 + c] * gy) + M[8 + c] * gz;
    }
    double dir[3];
    surf_dir(S, q, dir);
    g_depth[o] = (float)((G[0] * (dir[0] / S.f) + G[1] * (dir[1] / S.f)) - G[2]);
  } else {
    double g[3] = {0.0, 0.0, 0.0}, P[3] = {0.0, 0.0, 0.0};      // a lane past N brings zeros
    if (q < S.N) {
      const size_t o = (size_t)b * S.N + q;
      const double z = (double)depth[o];
      const double d = (z <= 0.0) ? 0.0 : z;
#pragma unroll
      for (int r = 0; r < 3; ++r) g[r] = (double)g_out[3 * o + r];
      double dir[3];
      surf_dir(S, q, dir);
      P[0] = (d * dir[0]) / S.f; P[1] = (d * dir[1]) / S.f; P[2] = -d;      // the forward's P_cc
      if (g_depth) {
        double M[12], G[3];
        proj_load_view(view, b, M);
#pragma unroll
        for (int c = 0; c < 3; ++c) G[c] = (M[c] * g[0] + M[4 + c] * g[1]) + M[8 + c] * g[2];
        g_depth[o] = (z <= 0.0) ? 0.0f : (float)((G[0] * (dir[0] / S.f) + G[1] * (dir[1] / S.f)) - G[2]);
      }
    }
    view_block_reduce<kViewSums>([&](int k) { return view_outer_term(g, P, k); }, view_part);
  }
}
}  // namespace srh
