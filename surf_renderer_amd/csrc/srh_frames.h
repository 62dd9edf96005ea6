// The reference's frame transforms and point projection as layers of their own (diffrend/torch/utils.py:539-647:
// world_to_cam, world_to_cam_batched, cam_to_world, cam_to_world_batched; torch/projection_layer.py:19-85:
// project_surfels, project_image_coordinates), forward and analytic backward; many views per launch (the view is grid
// dimension y).  See DESIGN.md "The frame transforms and the point projection".
//
// Frame transform.  Per view, n_pos points p = (x, y, z[, w]) (w = 1 for three columns) and n_normal normals
// n = (n0, n1, n2[, ignored]), the two counts independent, with two 3 x 4 fp64 tables made by the host:
//   out_pos[r]    = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3] w,  r = 0..2;  out_pos[3] = w       P = view_pos
//   out_normal[j] = (n0 A[0][j] + n1 A[1][j]) + n2 A[2][j],             j = 0..2                        A = view_normal
// The direction is the host's choice of tables: world to camera pairs P = lookat with A = lookat_inv, camera to world
// the other way round, as the reference pairs them.  Column 3 of A is not read.  Nothing is normalised.
// Backward, g the upstream gradients (out_pos has four columns, so g_pos has):
//   grad_pos[c]    = (g0 P[0][c] + g1 P[1][c]) + g2 P[2][c],  c = 0..2;  column 3 (four-column input) the same + g3
//   grad_normal[i] = (g0 A[i][0] + g1 A[i][1]) + g2 A[i][2],  i = 0..2;  column 3 (four-column input) exactly 0
//   kView: d loss / dP[r][c] = sum g_r [p, w]_c,  d loss / dA[i][j] = sum n_i g_j (column 3 exactly 0)
//
// Projection.  Per view, N points (three or four columns as above), M = the view's world-to-camera table:
//   (X, Y, Z) = the position transform above,  Zd = Z != 0 ? Z : 1                      nonzero_divide
//   plane    = (f (X / Zd), f (Y / Zd), -Z)                                             project_surfels
//   px_coord = (plane_x sx + W / 2, plane_y sy + H / 2, -Z),  sx = -(W - 1) / w, sy = (H - 1) / h
//   px_idx   = hproj_key(fsx (X / Zd) + cx0, fsy (Y / Zd) + cy0): the hard projection's key (srh_hard_projection.h),
//              same function, same operands for a three-column point; W H = the dump slot
// Backward, g_plane and g_coord the upstream gradients (either may be absent):
//   gx = g_plane_x + g_coord_x sx,  gy = g_plane_y + g_coord_y sy,  gz = g_plane_z + g_coord_z
//   dX = gx f / Zd,  dY = gy f / Zd,  dZ = -gz - (Z != 0 ? ((gx f) X + (gy f) Y) / (Zd Zd) : 0)
//   grad_surfels[c] = (dX M[0][c] + dY M[1][c]) + dZ M[2][c];   kView: d loss / dM = sum (dX, dY, dZ) (x) [p, w]
// At Z == 0 the x and y outputs have exactly zero gradient with respect to Z.
//
// One lane per point in both directions; fp32 loads, fp64 arithmetic in the order written above, one fp32 store per
// element, every element written once, no atomic.  Memory-bound: 12-16 B in and 12-16 B out per lane, and the bytes of
// consecutive lanes are contiguous.  The kView variants hand each lane's terms to view_block_reduce (srh_view_grad.h);
// a lane past a count brings zeros.
#pragma once
#include "srh_hard_projection.h"   // hproj_key
#include "srh_projection.h"        // proj_load_view
#include "srh_view_grad.h"

namespace srh {

constexpr int kFrameBlock = 256;

struct FramesDev {
  int B, n_pos, n_normal, pos_cols, normal_cols, nblk;      // nblk covers max(n_pos, n_normal)
};

struct PCoordDev {
  int B, N, cols, W, H, nblk;
  double f, sx, sy, hx, hy;           // px_coord = plane * (sx, sy) + (hx, hy)
  double fsx, fsy, cx0, cy0;          // the hard projection's u, v (pixel_scales)
};

// p = (x, y, z, w) of a point with `cols` columns
__device__ __forceinline__ void frame_load_point(const float* __restrict__ p, int cols, double v[4]) {
  v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2];
  v[3] = cols == 4 ? (double)p[3] : 1.0;
}

// rows 0-2 of M [p, w]
__device__ __forceinline__ void frame_apply(const double M[12], const double v[4], double out[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    out[r] = ((M[4 * r] * v[0] + M[4 * r + 1] * v[1]) + M[4 * r + 2] * v[2]) + M[4 * r + 3] * v[3];
}

// column c of g^T M: (g0 M[0][c] + g1 M[1][c]) + g2 M[2][c]
__device__ __forceinline__ double frame_apply_t(const double M[12], const double g[3], int c) {
  return (g[0] * M[c] + g[1] * M[4 + c]) + g[2] * M[8 + c];
}

// term k = 4 r + c of g (x) [p, w]
__device__ __forceinline__ double frame_outer_term(const double g[3], const double v[4], int k) {
  return g[k >> 2] * v[k & 3];
}

// pos (B, n_pos, pos_cols), normal (B, n_normal, normal_cols) fp32 -> out_pos (B, n_pos, 4), out_normal (B, n_normal, 3)
__global__ __launch_bounds__(kFrameBlock) void k_frames_fwd(FramesDev F, const double* __restrict__ view_pos,
                                                            const double* __restrict__ view_normal,
                                                            const float* __restrict__ pos,
                                                            const float* __restrict__ normal,
                                                            float* __restrict__ out_pos,
                                                            float* __restrict__ out_normal) {
  const int q = blockIdx.x * kFrameBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q < F.n_pos) {
    const size_t o = (size_t)b * F.n_pos + q;
    double M[12], v[4], P[3];
    proj_load_view(view_pos, b, M);
    frame_load_point(pos + o * F.pos_cols, F.pos_cols, v);
    frame_apply(M, v, P);
#pragma unroll
    for (int r = 0; r < 3; ++r) out_pos[4 * o + r] = (float)P[r];
    out_pos[4 * o + 3] = (float)v[3];
  }
  if (q < F.n_normal) {
    const size_t o = (size_t)b * F.n_normal + q;
    double A[12];
    proj_load_view(view_normal, b, A);
    const float* n = normal + o * F.normal_cols;
    const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) out_normal[3 * o + j] = (float)((n0 * A[j] + n1 * A[4 + j]) + n2 * A[8 + j]);
  }
}

// g_pos (B, n_pos, 4), g_normal (B, n_normal, 3) fp32 -> grad_pos (B, n_pos, pos_cols), grad_normal (B, n_normal,
// normal_cols) fp32, every element written; a NULL gradient is not wanted.  An absent half (count 0) is skipped.
// kView: also the two tables' gradients, 12 sums each per workgroup: part_pos and part_normal (srh_view_grad.h), either
// NULL = not wanted.
template <bool kView>
__global__ __launch_bounds__(kFrameBlock) void k_frames_bwd(FramesDev F, const double* __restrict__ view_pos,
                                                            const double* __restrict__ view_normal,
                                                            const float* __restrict__ pos,
                                                            const float* __restrict__ normal,
                                                            const float* __restrict__ g_pos,
                                                            const float* __restrict__ g_normal,
                                                            float* __restrict__ grad_pos,
                                                            float* __restrict__ grad_normal,
                                                            double* __restrict__ part_pos,
                                                            double* __restrict__ part_normal) {
  const int q = blockIdx.x * kFrameBlock + threadIdx.x;
  const int b = blockIdx.y;
  double g[3] = {0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};      // a lane past n_pos brings zeros
  if (q < F.n_pos) {
    const size_t o = (size_t)b * F.n_pos + q;
#pragma unroll
    for (int r = 0; r < 3; ++r) g[r] = (double)g_pos[4 * o + r];
    if (kView && part_pos) frame_load_point(pos + o * F.pos_cols, F.pos_cols, v);
    if (grad_pos) {
      double M[12];
      proj_load_view(view_pos, b, M);
      float* out = grad_pos + o * F.pos_cols;
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] = (float)frame_apply_t(M, g, c);
      if (F.pos_cols == 4) out[3] = (float)(frame_apply_t(M, g, 3) + (double)g_pos[4 * o + 3]);
    }
  }
  if (kView && part_pos)      // uniform over the launch: every thread of the workgroup calls the reduce
    view_block_reduce<kViewSums>([&](int k) { return frame_outer_term(g, v, k); }, part_pos);

  double h[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};           // a lane past n_normal brings zeros
  if (q < F.n_normal) {
    const size_t o = (size_t)b * F.n_normal + q;
#pragma unroll
    for (int j = 0; j < 3; ++j) h[j] = (double)g_normal[3 * o + j];
    if (kView && part_normal) {
      const float* in = normal + o * F.normal_cols;
      n[0] = (double)in[0]; n[1] = (double)in[1]; n[2] = (double)in[2];
    }
    if (grad_normal) {
      double A[12];
      proj_load_view(view_normal, b, A);
      float* out = grad_normal + o * F.normal_cols;
#pragma unroll
      for (int i = 0; i < 3; ++i) out[i] = (float)((h[0] * A[4 * i] + h[1] * A[4 * i + 1]) + h[2] * A[4 * i + 2]);
      if (F.normal_cols == 4) out[3] = 0.0f;
    }
  }
  if (kView && part_normal)
    view_block_reduce<kViewSums>([&](int k) { return (k & 3) == 3 ? 0.0 : n[k >> 2] * h[k & 3]; }, part_normal);
}

// what both directions of the projection compute of a point
struct PCoordPoint {
  double v[4], X, Y, Z, Zd;
};

__device__ __forceinline__ PCoordPoint pcoord_point(const PCoordDev& P, const double M[12],
                                                    const float* __restrict__ p) {
  PCoordPoint S;
  frame_load_point(p, P.cols, S.v);
  double cc[3];
  frame_apply(M, S.v, cc);
  S.X = cc[0]; S.Y = cc[1]; S.Z = cc[2];
  S.Zd = S.Z != 0.0 ? S.Z : 1.0;                       // nonzero_divide
  return S;
}

// surfels (B, N, cols) fp32 -> plane (B, N, 3), px_coord (B, N, 3) fp32 and px_idx (B, N) int32, each NULL = not wanted
__global__ __launch_bounds__(kFrameBlock) void k_project_fwd(PCoordDev P, const double* __restrict__ view,
                                                             const float* __restrict__ surfels,
                                                             float* __restrict__ plane, float* __restrict__ px_coord,
                                                             int32_t* __restrict__ px_idx) {
  const int q = blockIdx.x * kFrameBlock + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= P.N) return;
  const size_t o = (size_t)b * P.N + q;
  double M[12];
  proj_load_view(view, b, M);
  const PCoordPoint S = pcoord_point(P, M, surfels + o * P.cols);
  const double rx = S.X / S.Zd, ry = S.Y / S.Zd;
  const double x = P.f * rx, y = P.f * ry, z = -S.Z;
  if (plane) {
    plane[3 * o] = (float)x; plane[3 * o + 1] = (float)y; plane[3 * o + 2] = (float)z;
  }
  if (px_coord) {
    px_coord[3 * o] = (float)(x * P.sx + P.hx);
    px_coord[3 * o + 1] = (float)(y * P.sy + P.hy);
    px_coord[3 * o + 2] = (float)z;
  }
  if (px_idx) px_idx[o] = hproj_key(P.W, P.H, P.W * P.H, P.fsx * rx + P.cx0, P.fsy * ry + P.cy0);
}

// g_plane, g_coord (B, N, 3) fp32, either NULL = no such upstream -> grad_surfels (B, N, cols) fp32, every element
// written (column 3 of a four-column input included); kView: NULL = not wanted, and the table's 12 sums per workgroup
// go to view_part.
template <bool kView>
__global__ __launch_bounds__(kFrameBlock) void k_project_bwd(PCoordDev P, const double* __restrict__ view,
                                                             const float* __restrict__ surfels,
                                                             const float* __restrict__ g_plane,
                                                             const float* __restrict__ g_coord,
                                                             float* __restrict__ grad_surfels,
                                                             double* __restrict__ view_part) {
  const int q = blockIdx.x * kFrameBlock + threadIdx.x;
  const int b = blockIdx.y;
  double d[3] = {0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};      // a lane past N brings zeros
  if (q < P.N) {
    const size_t o = (size_t)b * P.N + q;
    double M[12];
    proj_load_view(view, b, M);
    const PCoordPoint S = pcoord_point(P, M, surfels + o * P.cols);
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (g_plane) {
      gx = (double)g_plane[3 * o]; gy = (double)g_plane[3 * o + 1]; gz = (double)g_plane[3 * o + 2];
    }
    if (g_coord) {
      gx = gx + (double)g_coord[3 * o] * P.sx;
      gy = gy + (double)g_coord[3 * o + 1] * P.sy;
      gz = gz + (double)g_coord[3 * o + 2];
    }
    const double fx = gx * P.f, fy = gy * P.f;
    d[0] = fx / S.Zd;
    d[1] = fy / S.Zd;
    d[2] = -gz - (S.Z != 0.0 ? (fx * S.X + fy * S.Y) / (S.Zd * S.Zd) : 0.0);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = S.v[c];
    if (grad_surfels) {
      float* out = grad_surfels + o * P.cols;
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] = (float)frame_apply_t(M, d, c);
      if (P.cols == 4) out[3] = (float)frame_apply_t(M, d, 3);
    }
  }
  if (kView) view_block_reduce<kViewSums>([&](int k) { return frame_outer_term(d, v, k); }, view_part);
}
}  // namespace srh
