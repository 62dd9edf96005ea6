// Uniform surface samples of a triangle mesh, per view: the reference's uniform_sample_mesh
// (diffrend/utils/sample_generator.py:157-194, over triangle_double_area, compute_face_normal and backface_culling),
// forward and backward; many views per launch.  See DESIGN.md "Mesh sampling".
//
// Per view, v (V, 3) fp32, f (F, 3) int32 (one list for every view, or one per view), optionally eye (3) fp64, and per
// sample three uniforms (r0, s, t) fp64 in [0, 1).  With p0, p1, p2 = v[f[i, 0..2]] in fp64:
//   c      = (p1 - p0) x (p2 - p0),  n = c / |c|  (the divisor 1 where |c| = 0)
//   area2  = sqrt((d0^2 + d1^2) + d2^2), d* the 2 x 2 determinants of r = p0 - p2 and s = p1 - p2 (the reference's order)
//   weight = area2 where it is finite and positive, the face's indices are inside [0, V) and, with an eye,
//            n . (eye - p0) >= 0; else 0
//   cdf[i] = (the largest prefix sum of the weights over the positive-weight faces j <= i) / (that of the last face)
//   face   = the number of faces with cdf <= r0, by binary search over [0, F - 1]
//   q = sqrt(s), bary = (1 - q, (1 - t) q, t q), pos = (b0 p0 + b1 p1) + b2 p2, normal = n of the face
// A view whose weights are all 0 gets face = -1 and NaN pos, normal and bary.
//
// Forward, three launches:
//   k_mesh_faces   a lane per face: the weight (the cull is folded into it; the normal is recomputed from the three
//                  gathered vertices by the sample pass, which holds them in registers anyway)
//   k_mesh_scan    ONE workgroup per view walks the faces in tiles of kMeshScanTile: a lane adds its kMeshScanItems
//                  consecutive weights serially, the lane totals are scanned across the wave by shuffles, the wave
//                  totals go through LDS, and a carry runs from tile to tile.  The order of every addition depends on
//                  F alone.  Prefix sums formed by different association trees are not monotone to the last bit, so the
//                  same pass takes the running MAXIMUM of the prefix sums of the positive-weight faces, which is exact:
//                  a zero-weight face has exactly its predecessor's value and is never chosen, and the last value is the
//                  total, so the last positive-weight face and everything behind it has cdf = 1 > r0 exactly.  It runs in
//                  place over the weights; a second walk by the same lanes divides by the total.
//   k_mesh_sample  a lane per sample: binary search, gather, one fp32 store per element.
// One workgroup per view scans 1024 faces per round of two barriers: some microseconds for the meshes of a few thousand
// to a few hundred thousand faces this serves; past about a million faces in a single view a decoupled multi-workgroup
// scan would be the better shape.
//
// Backward, two gathers (no atomic):
//   k_mesh_bwd_faces     a lane per face: its run in the caller's stable order of `face` by binary search, summed in
//                        ascending sample index -- A[c] = sum b_c g_pos (3 x 3, bary recomputed in fp64 from the
//                        uniforms) and gn = sum g_normal; gn goes through c / |c| (exactly 0 where |c| is 0 or not finite)
//                        and the cross product; nine fp64 per face, one per corner coordinate
//   k_mesh_bwd_vertices  a lane per vertex: its incident corners in the caller's stable order of the flattened f, summed
//                        in ascending corner index; one fp32 store per element, exactly 0 for an unreferenced vertex.
#pragma once
#include "srh_device.h"

namespace srh {

constexpr int kMeshBlock = 256;                                   // k_mesh_faces, k_mesh_sample, k_mesh_bwd_*
constexpr int kMeshScanBlock = 256;                               // k_mesh_scan: four waves
constexpr int kMeshScanWaves = kMeshScanBlock / 64;
constexpr int kMeshScanItems = 4;                                 //   consecutive faces per lane and tile
constexpr int kMeshScanTile = kMeshScanBlock * kMeshScanItems;    //   faces per round of the workgroup

struct MeshDev {
  int B, V, F, S, f_per_view, eye_per_view;
};

__device__ __forceinline__ const int32_t* mesh_faces_of(const MeshDev& P, const int32_t* f, int b) {
  return f + (P.f_per_view ? (size_t)b * P.F * 3 : (size_t)0);
}

// The three vertices of face i in fp64.  False where an index is outside [0, V): vertex 0 stands in, nothing is read
// out of bounds.
__device__ __forceinline__ bool mesh_load_tri(const MeshDev& P, const float* __restrict__ vb,
                                              const int32_t* __restrict__ fb, int i, double (&p)[3][3]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int32_t k = fb[(size_t)i * 3 + c];
    const bool in = (uint32_t)k < (uint32_t)P.V;
    ok = ok && in;
    k = in ? k : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[c][a] = (double)vb[(size_t)k * 3 + a];
  }
  return ok;
}

// e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2 in numpy.cross's order; returns |c| = sqrt((c0^2 + c1^2) + c2^2)
__device__ __forceinline__ double mesh_cross(const double (&p)[3][3], double (&e1)[3], double (&e2)[3], double (&c)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    e1[a] = p[1][a] - p[0][a];
    e2[a] = p[2][a] - p[0][a];
  }
  c[0] = e1[1] * e2[2] - e1[2] * e2[1];
  c[1] = e1[2] * e2[0] - e1[0] * e2[2];
  c[2] = e1[0] * e2[1] - e1[1] * e2[0];
  return sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
}

// weight (B, F) fp64.  eye NULL = no cull.
__global__ __launch_bounds__(kMeshBlock) void k_mesh_faces(MeshDev P, const float* __restrict__ v,
                                                           const int32_t* __restrict__ f,
                                                           const double* __restrict__ eye, double* __restrict__ weight) {
  const int i = blockIdx.x * kMeshBlock + threadIdx.x, b = blockIdx.y;
  if (i >= P.F) return;
  double p[3][3];
  bool ok = mesh_load_tri(P, v + (size_t)b * P.V * 3, mesh_faces_of(P, f, b), i, p);
  double r[3], s[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r[a] = p[0][a] - p[2][a];
    s[a] = p[1][a] - p[2][a];
  }
  const double d0 = r[1] * s[2] - r[2] * s[1];
  const double d1 = r[2] * s[0] - r[0] * s[2];
  const double d2 = r[0] * s[1] - r[1] * s[0];
  const double w = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  if (eye) {
    const double* e = eye + (P.eye_per_view ? (size_t)b * 3 : (size_t)0);
    double e1[3], e2[3], c[3];
    const double len = mesh_cross(p, e1, e2, c);
    const double den = len == 0.0 ? 1.0 : len;
    const double facing = ((c[0] / den) * (e[0] - p[0][0]) + (c[1] / den) * (e[1] - p[0][1])) +
                          (c[2] / den) * (e[2] - p[0][2]);
    ok = ok && facing >= 0.0;                                  // a NaN fails
  }
  weight[(size_t)b * P.F + i] = (ok && w > 0.0 && w < __builtin_inf()) ? w : 0.0;
}

// inclusive scans across the wave, Hillis-Steele: the earlier lanes' value is the left operand
__device__ __forceinline__ double mesh_wave_scan_add(double x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double y = __shfl_up(x, d, 64);
    if (lane >= d) x = y + x;
  }
  return x;
}
__device__ __forceinline__ double mesh_wave_scan_max(double x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double y = __shfl_up(x, d, 64);
    if (lane >= d) x = y > x ? y : x;
  }
  return x;
}

// blockIdx.x = the view.  cdf (B, F) fp64 holds the weights (finite, >= 0) on entry and the cdf on exit; total (B) gets
// the view's total weight, 0 for a view without a positive weight (its cdf is then all 0 and not used).
__global__ __launch_bounds__(kMeshScanBlock) void k_mesh_scan(MeshDev P, double* __restrict__ cdf,
                                                              double* __restrict__ total) {
  __shared__ double wave_sum[kMeshScanWaves], wave_max[kMeshScanWaves];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double* w = cdf + (size_t)b * P.F;
  double carry = 0.0, carry_max = 0.0;
  for (int base = 0; base < P.F; base += kMeshScanTile) {
    const int i0 = base + t * kMeshScanItems;
    double x[kMeshScanItems], s[kMeshScanItems];
#pragma unroll
    for (int k = 0; k < kMeshScanItems; ++k) x[k] = i0 + k < P.F ? w[i0 + k] : 0.0;
    s[0] = x[0];
#pragma unroll
    for (int k = 1; k < kMeshScanItems; ++k) s[k] = s[k - 1] + x[k];
    const double inc = mesh_wave_scan_add(s[kMeshScanItems - 1], lane);
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.0;
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    double tile = 0.0, woff = 0.0;
#pragma unroll
    for (int j = 0; j < kMeshScanWaves; ++j) {
      if (j == wave) woff = tile;
      tile = tile + wave_sum[j];
    }
    const double before = carry + (woff + exc);
    // the running maximum of the prefix sums of the positive-weight faces; 0 is neutral, every prefix sum is >= 0
    double m[kMeshScanItems], top = 0.0;
#pragma unroll
    for (int k = 0; k < kMeshScanItems; ++k) {
      const double prefix = x[k] > 0.0 ? before + s[k] : 0.0;
      top = prefix > top ? prefix : top;
      m[k] = top;
    }
    const double inc_max = mesh_wave_scan_max(m[kMeshScanItems - 1], lane);
    double exc_max = __shfl_up(inc_max, 1, 64);
    if (lane == 0) exc_max = 0.0;
    if (lane == 63) wave_max[wave] = inc_max;
    __syncthreads();
    double tile_max = 0.0, woff_max = 0.0;
#pragma unroll
    for (int j = 0; j < kMeshScanWaves; ++j) {
      if (j == wave) woff_max = tile_max;
      tile_max = wave_max[j] > tile_max ? wave_max[j] : tile_max;
    }
    double floor_max = carry_max > woff_max ? carry_max : woff_max;
    floor_max = exc_max > floor_max ? exc_max : floor_max;
#pragma unroll
    for (int k = 0; k < kMeshScanItems; ++k)
      if (i0 + k < P.F) w[i0 + k] = m[k] > floor_max ? m[k] : floor_max;
    carry = carry + tile;
    carry_max = tile_max > carry_max ? tile_max : carry_max;
  }
  if (t == 0) total[b] = carry_max;
  if (!(carry_max > 0.0)) return;
  // every lane divides what it stored itself
  for (int base = 0; base < P.F; base += kMeshScanTile) {
    const int i0 = base + t * kMeshScanItems;
#pragma unroll
    for (int k = 0; k < kMeshScanItems; ++k)
      if (i0 + k < P.F) w[i0 + k] = w[i0 + k] / carry_max;
  }
}

// bary of a sample's (s, t): the forward and the backward compute it alike
__device__ __forceinline__ void mesh_bary(double s, double t, double (&bc)[3]) {
  const double q = sqrt(s);
  bc[0] = 1.0 - q;
  bc[1] = (1.0 - t) * q;
  bc[2] = t * q;
}

// uniforms (B, S, 3) fp64; pos, normal, bary (B, S, 3) fp32, face (B, S) int32
__global__ __launch_bounds__(kMeshBlock) void k_mesh_sample(MeshDev P, const float* __restrict__ v,
                                                            const int32_t* __restrict__ f,
                                                            const double* __restrict__ uniforms,
                                                            const double* __restrict__ cdf,
                                                            const double* __restrict__ total, float* __restrict__ pos,
                                                            float* __restrict__ normal, int32_t* __restrict__ face,
                                                            float* __restrict__ bary) {
  const int i = blockIdx.x * kMeshBlock + threadIdx.x, b = blockIdx.y;
  if (i >= P.S) return;
  const size_t o = (size_t)b * P.S + i;
  const double r0 = uniforms[o * 3], tot = total[b];
  double p[3][3];
  int lo = 0;
  bool ok = tot > 0.0 && tot < __builtin_inf();
  if (ok) {
    const double* cv = cdf + (size_t)b * P.F;
    int hi = P.F - 1;                   // cdf[F - 1] = 1 > r0: the count of values <= r0 is at most F - 1
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (cv[mid] <= r0) lo = mid + 1;
      else hi = mid;
    }
    ok = mesh_load_tri(P, v + (size_t)b * P.V * 3, mesh_faces_of(P, f, b), lo, p);
  }
  if (!ok) {
    face[o] = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[o * 3 + a] = normal[o * 3 + a] = bary[o * 3 + a] = __builtin_nanf("");
    return;
  }
  double bc[3], e1[3], e2[3], c[3];
  mesh_bary(uniforms[o * 3 + 1], uniforms[o * 3 + 2], bc);
  const double len = mesh_cross(p, e1, e2, c);
  const double den = len == 0.0 ? 1.0 : len;
  face[o] = lo;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pos[o * 3 + a] = (float)((bc[0] * p[0][a] + bc[1] * p[1][a]) + bc[2] * p[2][a]);
    normal[o * 3 + a] = (float)(c[a] / den);
    bary[o * 3 + a] = (float)bc[a];
  }
}

// face (B, S) int32 and order (B, S) int32, per view a stable ascending permutation of face; g_pos, g_normal (B, S, 3)
// fp32, either NULL = a zero upstream gradient (its buffer is not read).  corner (B, F, 3, 3) fp64 is written, every
// element once: the gradient of each face's corners.  An order entry outside [0, S) is skipped.
__global__ __launch_bounds__(kMeshBlock) void k_mesh_bwd_faces(MeshDev P, const float* __restrict__ v,
                                                               const int32_t* __restrict__ f,
                                                               const double* __restrict__ uniforms,
                                                               const int32_t* __restrict__ face,
                                                               const int32_t* __restrict__ order,
                                                               const float* __restrict__ g_pos,
                                                               const float* __restrict__ g_normal,
                                                               double* __restrict__ corner) {
  const int i = blockIdx.x * kMeshBlock + threadIdx.x, b = blockIdx.y;
  if (i >= P.F) return;
  const size_t base = (size_t)b * P.S;
  int lo = 0, hi = P.S;                 // the first position of the order whose face is >= i
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int32_t j = order[base + mid];
    const int32_t k = (uint32_t)j < (uint32_t)P.S ? face[base + j] : P.F;
    if (k < i) lo = mid + 1;
    else hi = mid;
  }
  double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, gn[3] = {0.0, 0.0, 0.0};
  bool any = false;
  for (int at = lo; at < P.S; ++at) {   // the run, in ascending sample index (the order is stable)
    const int32_t j = order[base + at];
    if ((uint32_t)j >= (uint32_t)P.S) continue;
    if (face[base + j] != i) break;
    any = true;
    const size_t o = base + j;
    if (g_pos) {
      double bc[3];
      mesh_bary(uniforms[o * 3 + 1], uniforms[o * 3 + 2], bc);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) A[c][a] += bc[c] * (double)g_pos[o * 3 + a];
    }
    if (g_normal) {
#pragma unroll
      for (int a = 0; a < 3; ++a) gn[a] += (double)g_normal[o * 3 + a];
    }
  }
  if (any && g_normal) {
    double p[3][3], e1[3], e2[3], c[3];
    const bool ok = mesh_load_tri(P, v + (size_t)b * P.V * 3, mesh_faces_of(P, f, b), i, p);
    const double len = mesh_cross(p, e1, e2, c);
    if (ok && len > 0.0 && len < __builtin_inf()) {
      // n = c / |c|: dc = (gn - n (n . gn)) / |c|; c = e1 x e2: d e1 = e2 x dc, d e2 = dc x e1
      double n[3], dc[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) n[a] = c[a] / len;
      const double dot = (n[0] * gn[0] + n[1] * gn[1]) + n[2] * gn[2];
#pragma unroll
      for (int a = 0; a < 3; ++a) dc[a] = (gn[a] - n[a] * dot) / len;
      const double g1[3] = {e2[1] * dc[2] - e2[2] * dc[1], e2[2] * dc[0] - e2[0] * dc[2], e2[0] * dc[1] - e2[1] * dc[0]};
      const double g2[3] = {dc[1] * e1[2] - dc[2] * e1[1], dc[2] * e1[0] - dc[0] * e1[2], dc[0] * e1[1] - dc[1] * e1[0]};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        A[0][a] -= g1[a] + g2[a];
        A[1][a] += g1[a];
        A[2][a] += g2[a];
      }
    }
  }
  double* out = corner + ((size_t)b * P.F + i) * 9;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int a = 0; a < 3; ++a) out[c * 3 + a] = A[c][a];
}

// corner_order (3 F) int32, or (B, 3 F) with per-view faces: a stable ascending permutation of the flattened f, so
// that the corners of a vertex are a run of it in ascending corner index 3 face + c.  grad_v (B, V, 3) fp32 is
// written, every element once.  An order entry outside [0, 3 F) is skipped.
__global__ __launch_bounds__(kMeshBlock) void k_mesh_bwd_vertices(MeshDev P, const int32_t* __restrict__ f,
                                                                  const int32_t* __restrict__ corner_order,
                                                                  const double* __restrict__ corner,
                                                                  float* __restrict__ grad_v) {
  const int i = blockIdx.x * kMeshBlock + threadIdx.x, b = blockIdx.y;
  if (i >= P.V) return;
  const int n = 3 * P.F;
  const int32_t* fb = mesh_faces_of(P, f, b);
  const int32_t* ob = corner_order + (P.f_per_view ? (size_t)b * n : (size_t)0);
  const double* cb = corner + (size_t)b * P.F * 9;
  int lo = 0, hi = n;                   // the first position of the order whose vertex is >= i
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int32_t j = ob[mid];
    const int32_t k = (uint32_t)j < (uint32_t)n ? fb[j] : P.V;
    if (k < i) lo = mid + 1;
    else hi = mid;
  }
  double acc[3] = {0.0, 0.0, 0.0};
  for (int at = lo; at < n; ++at) {     // the run, in ascending corner index (the order is stable)
    const int32_t j = ob[at];
    if ((uint32_t)j >= (uint32_t)n) continue;
    if (fb[j] != i) break;
#pragma unroll
    for (int a = 0; a < 3; ++a) acc[a] += cb[(size_t)j * 3 + a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) grad_v[((size_t)b * P.V + i) * 3 + a] = (float)acc[a];
}

}  // namespace srh
