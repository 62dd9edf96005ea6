// Nearest points between two point sets, per view: the building block of the reference's hausdorff(u, v)
// (diffrend/torch/ops.py:112-125) and of a Chamfer loss, forward and backward; many views per launch (the view is grid
// dimension y, the direction grid dimension z).  See DESIGN.md "Point-set distances".
//
// Per view, u (N, D) and v (M, D) fp32, D in 1..4:
//   d2(i, j)  = sum over c, ascending, of (u_i[c] - v_j[c])^2            fp64: the differences, the first square, then FMAs
//   idx_u[i]  = the j whose d2(i, j) is smallest, dist_u[i] = sqrt(d2(i, idx_u[i]))  (d2 itself under `squared`)
//   idx_v[j], dist_v[j] likewise with the roles swapped
// The winner rule: the running best starts at +inf with index 0, the candidates are visited in ascending index, and one
// replaces the best only when its d2 is STRICTLY smaller.  So an exact tie goes to the lowest index, a candidate whose
// d2 is NaN or +inf never wins, and a query without a finite candidate gets dist = +inf, idx = 0.  (The reference forms
// the (N, M, D) difference tensor, and one NaN target poisons every query through torch.min.)
//
// Forward, k_ps_nearest<D>: one wave per kPsQueries queries of one direction, kPsQ of them per lane with their
// coordinates in fp64 registers.  The other set streams past every lane in ascending index through SCALAR loads from
// wave-uniform addresses, kPsUnroll targets per round (their fp32 coordinates arrive in SGPRs, one v_cvt_f64_f32 per
// coordinate and wave, shared by the lane's kPsQ queries); the ragged tail runs target by target, bounded, never
// padded.  No LDS, no barrier, no atomic, no buffer that grows with N M.
//
// Backward, k_ps_bwd<D>: one lane per point of the side whose gradient is written.  With dir(p, o) = (p - o) / |p - o|
// (2 (p - o) under `squared`), exactly 0 where the fp64 distance is 0 or not finite:
//   grad_p[i] = g_own[i] dir(p_i, o_idx_own[i])  +  sum over { j : idx_other[j] = i }, ascending j, of g_other[j] dir(p_i, o_j)
// The second part is a scatter in the reference; here the caller orders idx_other (stable, ascending), and the lane
// finds its run in that order by binary search and sums it in fp64 (as k_hproj_gather does).  One fp32 store per
// element, every element written once: values and gradients are identical from run to run, and a view's result does
// not depend on its batch.
#pragma once
#include "srh_device.h"       // as_constant

namespace srh {

constexpr int kPsBlock = 64;                      // k_ps_nearest: one wave
constexpr int kPsQ = 4;                           //   queries per lane
constexpr int kPsQueries = kPsBlock * kPsQ;       //   queries per workgroup
constexpr int kPsUnroll = 8;                      //   targets per round of the stream
constexpr int kPsBwdBlock = 256;                  // k_ps_bwd
constexpr int kPsMaxD = 4;

struct PsDev {
  int B, N, M, D, squared;
};

// d2 of a query q (fp64) and a target t (fp64), components ascending
template <int D>
__device__ __forceinline__ double ps_d2(const double (&q)[D], const double (&t)[D]) {
  const double d0 = q[0] - t[0];
  double s = d0 * d0;
#pragma unroll
  for (int c = 1; c < D; ++c) {
    const double d = q[c] - t[c];
    s = __builtin_fma(d, d, s);
  }
  return s;
}

// One target against the lane's kPsQ queries: strictly smaller wins (a NaN d2 fails the comparison)
template <int D>
__device__ __forceinline__ void ps_visit(const double (&q)[kPsQ][D], const double (&t)[D], int j, double (&best)[kPsQ],
                                         int32_t (&arg)[kPsQ]) {
#pragma unroll
  for (int k = 0; k < kPsQ; ++k) {
    const double s = ps_d2<D>(q[k], t);
    const bool win = s < best[k];
    best[k] = win ? s : best[k];
    arg[k] = win ? j : arg[k];
  }
}

// blockIdx.x = the block of kPsQueries queries, blockIdx.y = the view, blockIdx.z = the direction: 0 asks for every u_i
// its nearest v (dist_u, idx_u), 1 for every v_j its nearest u.  With one direction wanted the grid has one z and
// `first_dir` names it.  dist_* (B, n) fp32, idx_* (B, n) int32.
template <int D>
__global__ __launch_bounds__(kPsBlock) void k_ps_nearest(PsDev P, int first_dir, const float* __restrict__ u,
                                                         const float* __restrict__ v, float* __restrict__ dist_u,
                                                         int32_t* __restrict__ idx_u, float* __restrict__ dist_v,
                                                         int32_t* __restrict__ idx_v) {
  const int dir = first_dir + (int)blockIdx.z, b = blockIdx.y;
  const int nq = dir ? P.M : P.N, nt = dir ? P.N : P.M;
  const int q0 = blockIdx.x * kPsQueries + threadIdx.x;
  if ((int)blockIdx.x * kPsQueries >= nq) return;             // the grid is sized for the larger set
  const float* qs = (dir ? v : u) + (size_t)b * nq * D;
  // the targets are an input no kernel here writes, read at wave-uniform addresses: scalar loads
  const auto ts = as_constant((dir ? u : v) + (size_t)b * nt * D);

  double q[kPsQ][D], best[kPsQ];
  int32_t arg[kPsQ];
#pragma unroll
  for (int k = 0; k < kPsQ; ++k) {
    const int i = min(q0 + k * kPsBlock, nq - 1);             // a lane past the end repeats the last query, stores nothing
#pragma unroll
    for (int c = 0; c < D; ++c) q[k][c] = (double)qs[(size_t)i * D + c];
    best[k] = __builtin_inf();
    arg[k] = 0;
  }

  int j = 0;
  for (; j + kPsUnroll <= nt; j += kPsUnroll) {
    float raw[kPsUnroll * D];
#pragma unroll
    for (int e = 0; e < kPsUnroll * D; ++e) raw[e] = ts[(size_t)j * D + e];
#pragma unroll
    for (int r = 0; r < kPsUnroll; ++r) {
      double t[D];
#pragma unroll
      for (int c = 0; c < D; ++c) t[c] = (double)raw[r * D + c];
      ps_visit<D>(q, t, j + r, best, arg);
    }
  }
  for (; j < nt; ++j) {                                       // the ragged tail: bounded, not padded
    double t[D];
#pragma unroll
    for (int c = 0; c < D; ++c) t[c] = (double)ts[(size_t)j * D + c];
    ps_visit<D>(q, t, j, best, arg);
  }

  float* dist = (dir ? dist_v : dist_u) + (size_t)b * nq;
  int32_t* idx = (dir ? idx_v : idx_u) + (size_t)b * nq;
#pragma unroll
  for (int k = 0; k < kPsQ; ++k) {
    const int i = q0 + k * kPsBlock;
    if (i >= nq) continue;
    dist[i] = (float)(P.squared ? best[k] : sqrt(best[k]));   // sqrt(+inf) = +inf
    idx[i] = arg[k];
  }
}

// acc += g dir(p, o): the direction recomputed from the points, exactly 0 where the fp64 distance is 0 or not finite
template <int D>
__device__ __forceinline__ void ps_add_dir(bool squared, const double (&p)[D], const float* __restrict__ o, double g,
                                           double (&acc)[D]) {
  double t[D], d[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    t[c] = (double)o[c];
    d[c] = p[c] - t[c];
  }
  const double s = ps_d2<D>(p, t);
  if (!(s > 0.0 && s < __builtin_inf())) return;              // 0, +inf and NaN
  const double w = squared ? 2.0 * g : g / sqrt(s);
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] += w * d[c];
}

// blockIdx.x = the block of points, blockIdx.y = the view, blockIdx.z + first_side = the side: 0 writes grad_u (B, N, D),
// 1 grad_v (B, M, D).  For side 0 the own term reads idx_u and g_dist_u, the fan-in idx_v, order_v and g_dist_v; side 1
// the other way round.  order_* (B, n) int32: per view a stable ascending permutation of idx_*.  g_dist_* (B, n) are
// fp64: two upstream gradients that meet in one distance (hausdorff's sym and uv) are summed by the caller, and that sum
// must not round before it multiplies a direction that another term may cancel.  A NULL g_dist_* is a zero upstream
// gradient: its terms are skipped, and idx_* / order_* of that half are not read.  An index outside its
// range is skipped.
template <int D>
__global__ __launch_bounds__(kPsBwdBlock) void k_ps_bwd(PsDev P, int first_side, const float* __restrict__ u,
                                                        const float* __restrict__ v, const int32_t* __restrict__ idx_u,
                                                        const int32_t* __restrict__ idx_v,
                                                        const int32_t* __restrict__ order_u,
                                                        const int32_t* __restrict__ order_v,
                                                        const double* __restrict__ g_dist_u,
                                                        const double* __restrict__ g_dist_v, float* __restrict__ grad_u,
                                                        float* __restrict__ grad_v) {
  const int side = first_side + (int)blockIdx.z, b = blockIdx.y;
  const int np = side ? P.M : P.N, no = side ? P.N : P.M;
  const int i = blockIdx.x * kPsBwdBlock + threadIdx.x;
  if (i >= np) return;
  const float* ps = (side ? v : u) + (size_t)b * np * D;
  const float* os = (side ? u : v) + (size_t)b * no * D;
  const int32_t* idx_own = side ? idx_v : idx_u;
  const double* g_own = side ? g_dist_v : g_dist_u;
  const int32_t* idx_other = side ? idx_u : idx_v;
  const int32_t* order_other = side ? order_u : order_v;
  const double* g_other = side ? g_dist_u : g_dist_v;
  float* grad = (side ? grad_v : grad_u) + (size_t)b * np * D;
  const bool squared = P.squared != 0;

  double p[D], acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    p[c] = (double)ps[(size_t)i * D + c];
    acc[c] = 0.0;
  }
  if (g_own) {
    const int32_t j = idx_own[(size_t)b * np + i];
    if ((uint32_t)j < (uint32_t)no) ps_add_dir<D>(squared, p, os + (size_t)j * D, g_own[(size_t)b * np + i], acc);
  }
  if (g_other) {
    const size_t base = (size_t)b * no;
    int lo = 0, hi = no;                // the first position of the order whose index is >= i
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      const int32_t j = order_other[base + mid];
      const int32_t k = (uint32_t)j < (uint32_t)no ? idx_other[base + j] : np;
      if (k < i) lo = mid + 1;
      else hi = mid;
    }
    for (int at = lo; at < no; ++at) {  // the run, in ascending original index (the order is stable)
      const int32_t j = order_other[base + at];
      if ((uint32_t)j >= (uint32_t)no) continue;
      if (idx_other[base + j] != i) break;
      ps_add_dir<D>(squared, p, os + (size_t)j * D, g_other[base + j], acc);
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) grad[(size_t)i * D + c] = (float)acc[c];
}

}  // namespace srh
