// The camera gradient of the depth lift, of the three surfel warps and of the world-frame normals (srh_surfels.h,
// srh_projection.h, srh_reverse_projection.h, srh_dense_projection.h, srh_normals.h), up to the per-view 3 x 4 matrix the layer is handed: the kView variants of the layers'
// backward kernels form, per lane, the products that sum to d loss / d matrix, and this header holds the one copy of
// the reduction.  The chain from the matrix to eye / at / up is the host's.  See DESIGN.md "Differentiable cameras for
// the depth lift and the two warps".
//
//   view_block_reduce   every lane of a 256-thread workgroup brings K terms (zeros for a lane past N): butterfly sum
//                       within each wave, the four waves added in wave order through LDS, K plain stores to
//                       part[b][workgroup][K].  A workgroup with no lane in range stores zeros.  The lane hands its
//                       terms over as a function of k, so that the 12 products of an outer product g (x) [p, 1] are
//                       formed one at a time from 6 values and never live together (view_outer_term).
//   view_wave_reduce    the same for a workgroup that is one wave (the dense projection's surfel kernel): the butterfly
//                       alone, no LDS and no barrier; lane k keeps sum k and K lanes store.
//   k_view_finish       one workgroup per view adds the view's partials: row j of kViewRows takes the workgroups j,
//                       j + kViewRows, ... in that order, then the rows are halved log2(kViewRows) times through LDS.
//                       The order depends only on the number of workgroups, i.e. on N.
// No atomic anywhere, so the result is identical from run to run, and a view of a batch gets the bits of the same view
// alone (the view is grid dimension y in both kernels).
#pragma once
#include <hip/hip_runtime.h>

namespace srh {

constexpr int kViewBlock = 256;     // the workgroup of the layers' backward kernels (kProjBlock, kSurfBlock)
constexpr int kViewSums = 12;       // a 3 x 4 matrix, row-major
constexpr int kViewRows = 64;       // k_view_finish: 64 rows x 12 sums = 768 threads

// all 64 lanes get the same bits: the butterfly adds the same pairs in every lane
__device__ __forceinline__ double view_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// term k = 4 r + c of g (x) [p, 1]: g[r] p[c], and g[r] itself in column 3
__device__ __forceinline__ double view_outer_term(const double g[3], const double p[3], int k) {
  return (k & 3) == 3 ? g[k >> 2] : g[k >> 2] * p[k & 3];
}

// Called by EVERY thread of a one-dimensional 256-thread workgroup; term(k) is the lane's k-th term, k a constant after
// unrolling.  part: this launch's partials, (gridDim.y, gridDim.x, K) fp64, every element written.
template <int K, class Term>
__device__ __forceinline__ void view_block_reduce(Term term, double* __restrict__ part) {
  static_assert(K >= 1 && K <= kViewSums, "at most a 3 x 4 matrix");
  __shared__ double lds[kViewBlock / 64][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double sum = view_wave_sum(term(k));
    if (lane == 0) lds[wave][k] = sum;
  }
  __syncthreads();
  if (threadIdx.x < K)
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * K + threadIdx.x] =
        ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
}

// The one-wave form: called by EVERY lane of a one-dimensional 64-thread workgroup.  Every lane gets every sum (the
// butterfly), lane k keeps the k-th, and lanes 0 .. K - 1 store them: part (gridDim.y, gridDim.x, K) fp64 as above.
template <int K, class Term>
__device__ __forceinline__ void view_wave_reduce(Term term, double* __restrict__ part) {
  static_assert(K >= 1 && K <= kViewSums, "at most a 3 x 4 matrix");
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double sum = view_wave_sum(term(k));
    if ((int)threadIdx.x == k) mine = sum;
  }
  if (threadIdx.x < K) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * K + threadIdx.x] = mine;
}

// part (B, ngroups, K) fp64 -> grad_view (B, 12) fp64, every element written: entries [first, first + K) get the sums,
// the others exactly 0.  grid (1, B), block kViewRows * kViewSums.
__global__ __launch_bounds__(kViewRows * kViewSums) void k_view_finish(int ngroups, int K, int first,
                                                                       const double* __restrict__ part,
                                                                       double* __restrict__ grad_view) {
  __shared__ double rows[kViewRows][kViewSums];
  const int b = blockIdx.y;
  const int j = threadIdx.x / kViewSums, k = threadIdx.x % kViewSums;
  const double* p = part + (size_t)b * ngroups * K;
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
  if (j == 0) grad_view[(size_t)b * kViewSums + k] = (k >= first && k < first + K) ? rows[0][k - first] : 0.0;
}
}  // namespace srh
