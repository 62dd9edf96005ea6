// Analytic backward of the render path (gfx950): one thread per pixel, fp64 chain rule, fp32 atomic accumulation.
//
// What is differentiated is exactly what the forward computes for a hit pixel with winner m
// (reference numpy/renderer.py:204-263; gradient semantics = autograd through the reference's torch backend,
// torch/renderer.py:136-355 + torch/utils.py:238-366 -- selection and masks are piecewise constant):
//     planar m:  n^ = n/|n|, t = n^.(q - o) / (n^.d), q = pos | face[0]          p = o + t d
//     sphere m:  t = (-b -/+ sqrt(b^2 - 4a(|oc|^2 - r^2))) / 2a, n^ = (p - c)/|p - c|
//     shading:   im_c = sum_i (n^ . l^_i) C_ic A_c,  l^_i = (L_i - p)/|L_i - p|;  clip at 0;  out_c = im_c ^ gamma
// Accumulation: every sum is reduced over the wave before it goes out as fp32 atomics -- light / colour gradients over
// all 64 lanes (every pixel contributes to the same few addresses), albedo gradients too when the whole wave shades
// with one material, per-primitive gradients over the runs of adjacent pixels won by the same primitive (RunReduce).
#pragma once
#include "srh_device.h"

namespace srh {

struct GradsDev {
  float* pos[SRH_MAX_SEGMENTS];
  float* normal[SRH_MAX_SEGMENTS];
  float* radius[SRH_MAX_SEGMENTS];
  float* face[SRH_MAX_SEGMENTS];
  float* lights_pos;
  float* colors;
  float* albedo;
  float* coeffs;        // torch shading only
  float* attenuation;   // torch shading only
  float* ambient;       // torch shading only
};

// gamma * x^(gamma - 1) for x > 0, the tonemap's derivative, the way tonemap_f32 evaluates the tonemap itself: hardware
// log2 / exp2 in fp32 (1.1e-6 relative while |(gamma - 1) log2 x| <= 12; the gradients leave as fp32 sums and are checked
// to 2e-4 of their largest entry), the fp64 library pow outside that range.  The library call is ~250 fp64
// instructions per channel: a third of the numpy-shading backward kernel.
__device__ __forceinline__ double tonemap_slope(double x, double gamma) {
  const float xf = (float)x, e = (float)(gamma - 1.0);
  const float y = e * __builtin_amdgcn_logf(xf);
  if (xf >= 1.0e-30f && xf <= 1.0e30f && fabsf(y) <= 12.0f) return gamma * (double)__builtin_amdgcn_exp2f(y);
  return gamma * pow(x, gamma - 1.0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ void add3(float* dst, const double g[3]) {
  if (g[0] != 0.0) atomicAdd(dst + 0, (float)g[0]);
  if (g[1] != 0.0) atomicAdd(dst + 1, (float)g[1]);
  if (g[2] != 0.0) atomicAdd(dst + 2, (float)g[2]);
}

__device__ __forceinline__ void add3(float* dst, const float g[3]) {
  if (g[0] != 0.0f) atomicAdd(dst + 0, g[0]);
  if (g[1] != 0.0f) atomicAdd(dst + 1, g[1]);
  if (g[2] != 0.0f) atomicAdd(dst + 2, g[2]);
}

// Per-primitive gradients, reduced by key over the wave before they go out as atomics.  A wave is 64 consecutive
// pixels of one image row, so pixels won by the same primitive form RUNS of adjacent lanes: a segmented inclusive scan
// over the runs (six shuffle steps) leaves each run's sum in its last lane, and only that lane issues the atomics --
// one set per (wave, run) instead of one per pixel.  A plane that fills the frame sends 6 atomics per wave to its six
// addresses instead of 384; a primitive that re-appears after a gap in the same row simply forms
// two runs.  All 64 lanes must call this (lanes without a hit pass key -1 and zeros).
struct RunReduce {
  int lane, start;      // this lane, first lane of its run
  bool tail;            // last lane of its run: holds the run's sums after reduce()
  __device__ __forceinline__ RunReduce(int key, int lane_) : lane(lane_) {
    const int prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __builtin_amdgcn_ballot_w64(head);
    const unsigned long long upto = heads & (~0ull >> (63 - lane));          // heads at lanes <= this one (lane 0 is one)
    start = 63 - __builtin_clzll(upto);
    tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  }
  __device__ __forceinline__ float reduce(float v) const {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float t = __shfl_up(v, off);
      if (lane - off >= start) v += t;
    }
    return v;
  }
};

// Run-reduce one pixel's primitive gradients over the wave and add the run sums: gA -> pos (disc / plane / sphere) or
// face vertex 0 (triangle), gB -> normal (planar types), g_r -> radius (sphere).  key = winner's global index, -1 = none.
__device__ __forceinline__ void scatter_primitive_grads(const GradsDev& G, int key, int lane, int s, int type, int li,
                                                        const double gA[3], const double gB[3], double g_r) {
  const RunReduce run(key, lane);
  float v[7];
#pragma unroll
  for (int k = 0; k < 3; ++k) { v[k] = run.reduce((float)gA[k]); v[3 + k] = run.reduce((float)gB[k]); }
  v[6] = run.reduce((float)g_r);
  // Second level, for primitives larger than a wave's 64 pixels: when each of the workgroup's four waves (four image
  // rows) is ONE run of the same primitive, wave 0 adds the four sums and issues the only atomics of the workgroup.
  // (All 256 threads reach this barrier: a workgroup leaves the backward kernels only as a whole, at their top.)
  __shared__ float wsum[4][8];
  __shared__ int wkey[4];
  const int wave = threadIdx.y;
  const bool whole = run.start == 0 && lane == 63;          // this lane closes a run that spans the whole wave
  if (lane == 63) {
    wkey[wave] = (run.start == 0) ? key : -2;
#pragma unroll
    for (int k = 0; k < 7; ++k) wsum[wave][k] = v[k];
  }
  __syncthreads();
  const bool merged = wkey[0] >= 0 && wkey[0] == wkey[1] && wkey[0] == wkey[2] && wkey[0] == wkey[3];
  if (merged) {
    if (!(whole && wave == 0)) return;
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = (wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]);
  } else if (!run.tail || key < 0) {
    return;
  }
  float* dstA = nullptr;
  float* dstB = nullptr;
  float* dstR = nullptr;
#pragma unroll
  for (int i = 0; i < SRH_MAX_SEGMENTS; ++i)
    if (s == i) {
      dstA = type == SRH_PRIM_TRIANGLE ? (G.face[i] ? G.face[i] + 12 * (size_t)li : nullptr)
                                       : (G.pos[i] ? G.pos[i] + 4 * (size_t)li : nullptr);
      dstB = (type != SRH_PRIM_SPHERE && G.normal[i]) ? G.normal[i] + 4 * (size_t)li : nullptr;
      dstR = (type == SRH_PRIM_SPHERE && G.radius[i]) ? G.radius[i] + li : nullptr;
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (dstA && v[k] != 0.0f) atomicAdd(dstA + k, v[k]);
    if (dstB && v[3 + k] != 0.0f) atomicAdd(dstB + k, v[3 + k]);
  }
  if (dstR && v[6] != 0.0f) atomicAdd(dstR, v[6]);
}

// The body of k_render_bwd and k_render_bwd_views: one frame F with its gradient destinations G.
__device__ __forceinline__ void render_bwd_body(const FrameDev& F, const GradsDev& G, const float* grad_image,
                                                const float* grad_depth,
                                                const int32_t* nearest,
                                                const float* depth) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int r = F.row0 + blockIdx.y * 4 + threadIdx.y;
  const int lane = threadIdx.x;
  const bool live = (c < F.W) && (r < F.row1);
  const size_t row = live ? (size_t)(r - F.row0) : 0;
  const int cc = live ? c : 0;
  // background pixels (depth = +inf) and pixels outside the slab take part in the wave reductions with zeros
  const bool hit = live && isfinite(depth[row * F.depth_stride + cc]);
  // a workgroup (4 rows x 64 pixels) without a single hit pixel contributes nothing: it leaves together, before the
  // reductions below (whose barriers every thread of a workgroup that stays still reaches) -- a mesh that covers a fifth
  // of the frame then runs a fifth of the workgroups through the fp64 chain rule
  if (!__syncthreads_or(hit ? 1 : 0)) return;

  double g_out[3] = {0, 0, 0}, g_dep = 0.0;
  int win = 0;
  if (hit) {
    const float* gi = grad_image + row * F.img_stride + 3 * (size_t)cc;
    g_out[0] = gi[0]; g_out[1] = gi[1]; g_out[2] = gi[2];
    if (grad_depth) g_dep = grad_depth[row * F.depth_stride + cc];
    win = nearest[row * F.near_stride + cc];
  }
  int s = 0;
#pragma unroll
  for (int i = 1; i < SRH_MAX_SEGMENTS; ++i)
    if (i < F.nseg && win >= F.seg[i].first) s = i;
  // type, local index and record are selected here; the other per-batch pointers where they are used (seg_ptr), as in
  // render_bwd_tch_body.  (Eight fields selected in one chain: behind a reference to F hipcc turns the chain into
  // reads at per-lane addresses inside F, which for a by-value kernel argument means a copy of F.seg in scratch.)
  int type = F.seg[0].type, first = F.seg[0].first;
  const double* rec_base = F.seg[0].rec64;
#pragma unroll
  for (int i = 1; i < SRH_MAX_SEGMENTS; ++i)
    if (s == i) { type = F.seg[i].type; first = F.seg[i].first; rec_base = F.seg[i].rec64; }
  const int li = win - first;
  auto seg_ptr = [&](auto field) {
    auto ptr = field(F.seg[0]);
#pragma unroll
    for (int i = 1; i < SRH_MAX_SEGMENTS; ++i)
      if (s == i) ptr = field(F.seg[i]);
    return ptr;
  };

  double d[3] = {0, 0, -1};
  pixel_ray(F, live ? c : 0, live ? r : F.row0, d);

  // ---- forward quantities of this pixel ---------------------------------------------------------------------
  double t = 0.0, n[3] = {0, 0, 0}, p[3] = {0, 0, 0};
  double sph_v[3] = {0, 0, 0}, sph_inv = 0.0;          // sphere: p - c and 1/|p - c|
  bool sph_ok = false;
  const double* R = rec_base + (size_t)li * kRec64Stride[type];
  if (hit) {
    t = hit_any64(type, R, F.o, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = F.o[k] + t * d[k];
    if (type == SRH_PRIM_SPHERE) {
      const float* cp = seg_ptr([](const SegDev& S) { return S.pos; }) + 4 * (size_t)li;
#pragma unroll
      for (int k = 0; k < 3; ++k) sph_v[k] = p[k] - (double)cp[k];
      const double len2 = (sph_v[0] * sph_v[0] + sph_v[1] * sph_v[1]) + sph_v[2] * sph_v[2];
      (void)hit_sphere64(R, d, &sph_ok);
      sph_inv = (len2 > 0.0 && sph_ok) ? 1.0 / sqrt(len2) : 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) n[k] = sph_v[k] * sph_inv;
    } else {
      n[0] = R[0]; n[1] = R[1]; n[2] = R[2];
    }
  }
  const int m = hit ? clampi(seg_ptr([](const SegDev& S) { return S.mat; })[li], 0, F.nmat - 1) : 0;
  double alb[3] = {0, 0, 0};
  if (hit) { alb[0] = F.albedo[3 * m]; alb[1] = F.albedo[3 * m + 1]; alb[2] = F.albedo[3 * m + 2]; }

  // first pass over the lights: the image value, needed for the clip / tonemap derivative
  double im[3] = {0, 0, 0};
  for (int l = 0; l < F.nlights; ++l) {
    const float* lp = F.lpos + 4 * l;
    const double v[3] = {(double)lp[0] - p[0], (double)lp[1] - p[1], (double)lp[2] - p[2]};
    const double len2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double inv = (len2 > 0.0) ? rsqrt_newton(len2) : 1.0;     // ~1e-15 relative: far inside the fp32 sums
    const double sdot = ((n[0] * v[0] + n[1] * v[1]) + n[2] * v[2]) * inv;
    const int ci = clampi(F.lcidx[l], 0, F.ncolors - 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) im[ch] += (sdot * (double)F.colors[3 * ci + ch]) * alb[ch];
  }
  // d out / d im: clip passes im >= 0; gamma: gamma * im^(gamma-1) for im > 0
  double g_im[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double w = 0.0;
    if (hit) {
      if (F.tonemap) w = (im[ch] > 0.0) ? tonemap_slope(im[ch], F.gamma) : 0.0;
      else w = (im[ch] >= 0.0) ? 1.0 : 0.0;
    }
    g_im[ch] = g_out[ch] * w;
  }

  // second pass: gradients through the shading
  double g_n[3] = {0, 0, 0}, g_p[3] = {0, 0, 0}, g_alb[3] = {0, 0, 0};
  for (int l = 0; l < F.nlights; ++l) {
    const float* lp = F.lpos + 4 * l;
    const double v[3] = {(double)lp[0] - p[0], (double)lp[1] - p[1], (double)lp[2] - p[2]};
    const double len2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const bool nz = len2 > 0.0;
    const double inv = nz ? rsqrt_newton(len2) : 1.0;
    const double lh[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
    const double sdot = (n[0] * lh[0] + n[1] * lh[1]) + n[2] * lh[2];
    const int ci = clampi(F.lcidx[l], 0, F.ncolors - 1);
    double g_s = 0.0, g_col[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double col = (double)F.colors[3 * ci + ch];
      g_s += g_im[ch] * col * alb[ch];
      g_alb[ch] += g_im[ch] * sdot * col;
      g_col[ch] = g_im[ch] * sdot * alb[ch];
    }
    // l^ = v/|v| (|v| = 0 -> divided by 1: l^ = v, Q7): g_v = (g_lh - l^ (l^.g_lh)) / |v|, or g_lh itself
    const double g_lh[3] = {g_s * n[0], g_s * n[1], g_s * n[2]};
    const double proj = (lh[0] * g_lh[0] + lh[1] * g_lh[1]) + lh[2] * g_lh[2];
    double g_v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g_v[k] = nz ? (g_lh[k] - lh[k] * proj) * inv : g_lh[k];
      g_n[k] += g_s * lh[k];
      g_p[k] -= g_v[k];
    }
    // light position and light colour: every pixel of the wave adds to the same address -> reduce first
    if (G.lights_pos) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float sum = wave_sum((float)g_v[k]);
        if (lane == 0 && sum != 0.0f) atomicAdd(G.lights_pos + 4 * l + k, sum);
      }
    }
    if (G.colors) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float sum = wave_sum((float)g_col[ch]);
        if (lane == 0 && sum != 0.0f) atomicAdd(G.colors + 3 * ci + ch, sum);
      }
    }
  }
  if (G.albedo) {
    // one material for the whole wave (the common case) -> one atomic per channel; otherwise per lane
    const int m0 = __builtin_amdgcn_readfirstlane(m);
    const bool uniform = __builtin_amdgcn_ballot_w64(hit && m != m0) == 0ull;
    if (uniform) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float sum = wave_sum((float)g_alb[ch]);
        if (lane == 0 && sum != 0.0f) atomicAdd(G.albedo + 3 * m0 + ch, sum);
      }
    } else if (hit) {
      add3(G.albedo + 3 * m, g_alb);
    }
  }
  // ---- geometry: every lane takes part (run reduction below); lanes without a hit carry zeros -------------------------
  double gA[3] = {0, 0, 0};        // d/d pos (disc, plane, sphere) or d/d face vertex 0 (triangle)
  double gB[3] = {0, 0, 0};        // d/d normal (planar types)
  double g_r = 0.0;                // d/d radius (sphere)
  if (hit && type == SRH_PRIM_SPHERE) {
    // n^ = v/|v| with v = p - c (zero gradient where the line misses the sphere: n^ is the constant 0 there)
    const double proj = (n[0] * g_n[0] + n[1] * g_n[1]) + n[2] * g_n[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double g_v = (g_n[k] - n[k] * proj) * sph_inv;
      g_p[k] += g_v;
      gA[k] = -g_v;
    }
    const double g_t = ((g_p[0] * d[0] + g_p[1] * d[1]) + g_p[2] * d[2]) + g_dep;
    // t = (-b -/+ root)/(2a) unless it is one of the reference's constants (1.0 for a bad root, 0 for a miss)
    const double a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const double b = 2.0 * dot3(R, d);
    const double disc = b * b - 4.0 * a * R[3];
    if (disc > 0.0) {
      const double root = sqrt(disc), inv2a = 1.0 / (2.0 * a);
      const double t1 = (-b - root) * inv2a, t2 = (-b + root) * inv2a;
      const double t1v = (t1 >= 0.0) ? t1 : 1.0, t2v = (t2 >= 0.0) ? t2 : 1.0;
      const bool use1 = t1v <= t2v;
      const bool constant = use1 ? !(t1 >= 0.0) : !(t2 >= 0.0);
      if (!constant) {
        const double sgn = use1 ? -1.0 : 1.0;
        double g_b = -g_t * inv2a;
        const double g_disc = sgn * g_t * inv2a / (2.0 * root);
        g_b += 2.0 * b * g_disc;
        const double g_cc = -4.0 * a * g_disc;
        g_r = -2.0 * (double)seg_ptr([](const SegDev& S) { return S.radius; })[li] * g_cc;
#pragma unroll
        for (int k = 0; k < 3; ++k) gA[k] -= 2.0 * R[k] * g_cc + 2.0 * d[k] * g_b;   // oc = o - c
      }
    }
  } else if (hit) {
    // planar: t = k/den, k = n^.(q - o), den = n^.d
    const double g_t = ((g_p[0] * d[0] + g_p[1] * d[1]) + g_p[2] * d[2]) + g_dep;
    const double den = dot3(R, d);
    const double g_k = g_t / den, g_den = -g_t * t / den;
    const float* qp = (type == SRH_PRIM_TRIANGLE) ? seg_ptr([](const SegDev& S) { return S.face; }) + 12 * (size_t)li
                                                  : seg_ptr([](const SegDev& S) { return S.pos; }) + 4 * (size_t)li;
    double g_nh[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gA[k] = g_k * n[k];
      g_nh[k] = g_n[k] + g_k * ((double)qp[k] - F.o[k]) + g_den * d[k];
    }
    // n^ = nin/|nin| (4-D norm with w = 0; a zero normal stays zero and gets the gradient divided by 1)
    const float* np_ = seg_ptr([](const SegDev& S) { return S.normal; }) + 4 * (size_t)li;
    const double nin2 = (((double)np_[0] * np_[0] + (double)np_[1] * np_[1]) + (double)np_[2] * np_[2]) + (double)np_[3] * np_[3];
    const double ninv = (nin2 > 0.0) ? 1.0 / sqrt(nin2) : 1.0;
    const double proj = (nin2 > 0.0) ? (n[0] * g_nh[0] + n[1] * g_nh[1]) + n[2] * g_nh[2] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) gB[k] = (g_nh[k] - n[k] * proj) * ninv;
  }
  scatter_primitive_grads(G, hit ? win : -1, lane, s, type, li, gA, gB, g_r);
}

__global__ __launch_bounds__(256) void k_render_bwd(FrameDev F, GradsDev G, const float* __restrict__ grad_image,
                                                     const float* __restrict__ grad_depth,
                                                     const int32_t* __restrict__ nearest,
                                                     const float* __restrict__ depth) {
  render_bwd_body(F, G, grad_image, grad_depth, nearest, depth);
}

// A batch of views per launch (srh_render_views_bwd): grid (pixel_grid.x, pixel_grid.y, n_views), view v = blockIdx.z
// works on Fs[v] and adds into Gs[v]; the stacked per-view arrays are offset as srh_render_views offsets its outputs.
// Fs and Gs were written by a copy in front of the launch and nothing in the kernel writes them: they are read in
// their constant-address-space form (as_constant), so a view's descriptors arrive by scalar loads where they are used,
// as a by-value kernel argument's fields do, and never occupy vector registers.
__global__ __launch_bounds__(256) void k_render_bwd_views(const FrameDev* __restrict__ Fs, const GradsDev* __restrict__ Gs,
                                                           const float* __restrict__ grad_images,
                                                           const float* __restrict__ grad_depths,
                                                           const int32_t* __restrict__ nearests,
                                                           const float* __restrict__ depths,
                                                           const uint64_t* __restrict__ visibility) {
  const size_t v = blockIdx.z;
  const FrameDev& F = *(const FrameDev*)(as_constant(Fs) + v);
  const GradsDev& G = *(const GradsDev*)(as_constant(Gs) + v);
  const size_t rows = (size_t)(F.row1 - F.row0);
  (void)visibility;                                       // the numpy backend has no shadow rays
  render_bwd_body(F, G, grad_images + v * rows * F.img_stride,
                  grad_depths ? grad_depths + v * rows * F.depth_stride : nullptr,
                  nearests + v * rows * F.near_stride, depths + v * rows * F.depth_stride);
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward of the torch backend's semantics (SRH_SHADING_TORCH; reference torch/renderer.py:82-125,136-355):
//     n^ = n / sqrt(|n|^2 + 3e-10)  (sphere: (p - c) likewise),   c^ = (o - p) / sqrt(|o - p|^2 + 3e-10)
//     per light i:  l = L_i - p, dist = |l|, l^ = l / dist,  afac = 1 / (kc + kl dist + kq dist^pw)   (pw = 2 | 4)
//                   ndotl = relu(sgn afac (l^ . n^)),  rdotc = relu(sgn (2 (l^ . n^)(c^ . n^) - c^ . l^))
//                   im_c += (c0 ndotl + c1 rdotc^c2) C_ic A_c + amb_c A_c
//     out_c = relu(im_c) ^ gamma
// sgn = sign(c^ . n^) with double_sided, else 1 -- a constant, like the relus (threshold_backward selects, it does not
// multiply) and the nearest-hit selection.  torch.pow: 0^0 = 1, d/d exponent = 0 at base 0, d/d base = 0 at exponent 0.
// Misses and the far + 1 background carry no gradient.
// ---------------------------------------------------------------------------------------------------------------------
// Two compile-time variants (srh_render_bwd_aux):
//   kAux    the upstream gradients of the extra outputs normal = n^ (un-flipped: double_sided flips only inside the
//           shading) and pos = origin + t d enter at hit pixels, added to d/d n^ and d/d p before the geometry chain.
//           grad_normal / grad_pos are dense (rows,W,3) like the forward's normal_out / pos_out; either may be NULL.
//   kImage  grad_image is read and the shading differentiated.  Without it both light loops and every light /
//           material / colour accumulation drop out: a geometry-only backward for losses on normal / pos / depth.
//   kCam    camera gradients (srh_render_bwd_camera): every hit pixel also forms the gradients of its ray origin and ray
//           direction, maps them to the camera basis (end of the kernel) and the workgroup stores its twelve fp64 partial sums
//           to cam_part[workgroup][12] with plain stores; k_camera_finish adds the workgroups up in a fixed order.  A
//           workgroup that leaves at the top stores zeros, so the scratch needs no clearing launch and never holds a
//           stale partial.  Without kCam the trailing argument is unused and the code is what it was without it.
// <false, true> is srh_render_bwd's kernel (the trailing arguments are unused there).
constexpr int kBwdTchWaves = 3;
constexpr int kCamSums = 12;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// The body of k_render_bwd_tch and k_render_bwd_tch_views: one frame F with its gradient destinations G.
template <bool kAux, bool kImage, bool kCam>
__device__ __forceinline__ void render_bwd_tch_body(const FrameDev& F, const GradsDev& G, const float* grad_image,
                                                    const float* grad_depth,
                                                    const int32_t* nearest,
                                                    const float* depth,
                                                    const uint64_t* visibility,
                                                    const float* grad_normal,
                                                    const float* grad_pos,
                                                    double* cam_part) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int r = F.row0 + blockIdx.y * 4 + threadIdx.y;
  const int lane = threadIdx.x;
  const bool live = (c < F.W) && (r < F.row1);
  const size_t row = live ? (size_t)(r - F.row0) : 0;
  const int cc = live ? c : 0;
  const bool hit = live && ((double)depth[row * F.depth_stride + cc] <= F.far_clip);
  // a workgroup (4 rows x 64 pixels) without a single hit pixel contributes nothing: it leaves together, before the
  // reductions below (whose barriers every thread of a workgroup that stays still reaches) -- a mesh that covers a fifth
  // of the frame then runs a fifth of the workgroups through the fp64 chain rule
  if (!__syncthreads_or(hit ? 1 : 0)) {
    if (kCam && threadIdx.y == 0 && lane < kCamSums)       // its slot of the camera partials: zeros, never a stale frame's
      cam_part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kCamSums + lane] = 0.0;
    return;
  }

  float g_out[3] = {0, 0, 0}, g_dep = 0.0f;               // upstream gradients are fp32
  int win = 0;
  if (hit) {
    if (kImage) {
      const float* gi = grad_image + row * F.img_stride + 3 * (size_t)cc;
      g_out[0] = gi[0]; g_out[1] = gi[1]; g_out[2] = gi[2];
    }
    if (grad_depth) g_dep = grad_depth[row * F.depth_stride + cc];
    win = nearest[row * F.near_stride + cc];
  }
  int s = 0;
#pragma unroll
  for (int i = 1; i < SRH_MAX_SEGMENTS; ++i)
    if (i < F.nseg && win >= F.seg[i].first) s = i;
  // only what the whole kernel needs stays in registers (type, local index, record); the other per-segment pointers are
  // selected again where they are used -- six 64-bit pointers held across both light loops cost 12 registers
  int type = F.seg[0].type, first = F.seg[0].first;
  const double* rec_base = F.seg[0].rec64;
#pragma unroll
  for (int i = 1; i < SRH_MAX_SEGMENTS; ++i)
    if (s == i) { type = F.seg[i].type; first = F.seg[i].first; rec_base = F.seg[i].rec64; }
  const int li = win - first;
  auto seg_ptr = [&](auto field) {
    auto ptr = field(F.seg[0]);
#pragma unroll
    for (int i = 1; i < SRH_MAX_SEGMENTS; ++i)
      if (s == i) ptr = field(F.seg[i]);
    return ptr;
  };
  // light visibility of the forward pass (shadow rays): a constant 0 / 1 factor on each light's colour x albedo term
  const uint64_t vis = (kImage && visibility && hit) ? visibility[row * (size_t)F.W + cc] : ~0ull;

  // the pixel's ray: from the eye (perspective), or from its own origin eye + q0 on the image plane with the one
  // direction -z of the camera basis (orthographic, torch/utils.py:461-468); org is what the reference calls ray_orig
  const int pc = live ? c : 0, pr = live ? r : F.row0;
  double d[3], q0[3], org[3];
  const double* R = rec_base + (size_t)li * kRec64Stride[type];
  const double t = primary_hit(F, pc, pr, type, R, d, q0, org, hit);

  // ---- forward quantities of this pixel ---------------------------------------------------------------------
  double n[3] = {0, 0, 0}, p[3] = {0, 0, 0};
  double sph_inv = 0.0;                                    // sphere: 1 / sqrt(|p - c|^2 + 3e-10)
  if (hit) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = org[k] + t * d[k];
    if (type == SRH_PRIM_SPHERE) {
      const float* cp = seg_ptr([](const SegDev& S) { return S.pos; }) + 4 * (size_t)li;
      double v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = p[k] - (double)cp[k];
      sph_inv = 1.0 / sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 3.0e-10);
#pragma unroll
      for (int k = 0; k < 3; ++k) n[k] = v[k] * sph_inv;
    } else {
      n[0] = R[0]; n[1] = R[1]; n[2] = R[2];
    }
  }
  const int m = hit ? clampi(seg_ptr([](const SegDev& S) { return S.mat; })[li], 0, F.nmat - 1) : 0;
  float alb[3] = {0, 0, 0}, cf[3] = {1.0f, 0.0f, 0.0f}, amb[3] = {0, 0, 0};    // inputs are fp32: kept as such, widened at use
  if (hit) {
    alb[0] = F.albedo[3 * m]; alb[1] = F.albedo[3 * m + 1]; alb[2] = F.albedo[3 * m + 2];
    if (F.coeffs) { cf[0] = F.coeffs[3 * m]; cf[1] = F.coeffs[3 * m + 1]; cf[2] = F.coeffs[3 * m + 2]; }
    if (F.ambient) { amb[0] = F.ambient[0]; amb[1] = F.ambient[1]; amb[2] = F.ambient[2]; }
  }
  // view direction
  const double u[3] = {F.o[0] - p[0], F.o[1] - p[1], F.o[2] - p[2]};
  const double sc_inv = 1.0 / sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + 3.0e-10);
  const double cdir[3] = {u[0] * sc_inv, u[1] * sc_inv, u[2] * sc_inv};
  const double cdotn = (cdir[0] * n[0] + cdir[1] * n[1]) + cdir[2] * n[2];
  const double sgn = F.double_sided ? ((cdotn > 0.0) ? 1.0 : ((cdotn < 0.0) ? -1.0 : 0.0)) : 1.0;
  const int pw = F.use_quartic ? 4 : 2;
  const int nlights = kImage ? F.nlights : 0;              // geometry-only variant: no light loop at all

  // per-light forward terms, evaluated twice (image first: its value gates the clip / tonemap derivative).
  // The light loops run in fp32: the hit point, the normal and the view direction come out of the fp64 geometry above and
  // are rounded once; everything a light contributes is then a few dozen fp32 operations whose sums leave as fp32
  // atomics anyway.  With these terms in fp64 the kernel held 168 registers (three waves per SIMD, 9 of them spilled).
  const float nf[3] = {(float)n[0], (float)n[1], (float)n[2]};
  const float cdf[3] = {(float)cdir[0], (float)cdir[1], (float)cdir[2]};
  const float cdotnf = (float)cdotn, sgnf = (float)sgn;
  struct LightTerms {
    float lh[3], dist, afac, ldn, nd, rd, cl;
    bool nz, den_ok;
  };
  auto light_terms = [&](int l, LightTerms& T) {
    const float* lp = F.lpos + 4 * l;
    // the difference is formed in fp64 (light and fragment may be far from the origin and close to each other)
    const double vd[3] = {(double)lp[0] - p[0], (double)lp[1] - p[1], (double)lp[2] - p[2]};
    const float v[3] = {(float)vd[0], (float)vd[1], (float)vd[2]};
    T.dist = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    T.nz = T.dist > 0.0f;
    const float inv = T.nz ? 1.0f / T.dist : 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) T.lh[k] = v[k] * inv;
    const float kc = F.latt ? F.latt[3 * l] : 1.0f, kl = F.latt ? F.latt[3 * l + 1] : 0.0f, kq = F.latt ? F.latt[3 * l + 2] : 0.0f;
    const float dp = (pw == 4) ? (T.dist * T.dist) * (T.dist * T.dist) : T.dist * T.dist;
    const float den = (kc + T.dist * kl) + dp * kq;
    T.den_ok = fabsf(den) > 0.0f;
    T.afac = T.den_ok ? 1.0f / den : 1.0f;
    T.ldn = (T.lh[0] * nf[0] + T.lh[1] * nf[1]) + T.lh[2] * nf[2];
    T.cl = (cdf[0] * T.lh[0] + cdf[1] * T.lh[1]) + cdf[2] * T.lh[2];
    T.nd = sgnf * (T.afac * T.ldn);
    // The lobe's base is the exception: r.c = 2 (l^.n)(c^.n) - c^.l^ cancels to 0 at the lobe's edge, where rdotc ** (n - 1)
    // of an exponent below 1 is unbounded, and comes within 1e-6 of 1 at the highlight's centre, where an exponent of
    // 1000 multiplies every error of the base by 1000.  In fp32 it carries ~1e-7 ABSOLUTE either way; formed in fp64, as
    // the forward pass forms it, and rounded once, it is good to 6e-8 RELATIVE at 3e-8 as well.
    const double len2 = (vd[0] * vd[0] + vd[1] * vd[1]) + vd[2] * vd[2];
    const double invd = (len2 > 0.0) ? rsqrt_newton(len2) : 1.0;
    const double ldn = ((vd[0] * n[0] + vd[1] * n[1]) + vd[2] * n[2]) * invd;
    const double cl = ((vd[0] * cdir[0] + vd[1] * cdir[1]) + vd[2] * cdir[2]) * invd;
    T.rd = (float)(sgn * (2.0 * ldn * cdotn - cl));
  };
  // the forward pass evaluates the lobe in fp32 too (spec_pow_f32)
  auto spec_pow = [&](float rdotc) { return (rdotc == 0.0f && cf[2] == 0.0f) ? 1.0f : powf(rdotc, cf[2]); };

  float im[3] = {0, 0, 0};
  for (int l = 0; l < nlights; ++l) {
    LightTerms T;
    light_terms(l, T);
    const float w = (cf[0] * fmaxf(T.nd, 0.0f) + cf[1] * spec_pow(fmaxf(T.rd, 0.0f))) * (float)((vis >> l) & 1ull);
    const int ci = clampi(F.lcidx[l], 0, F.ncolors - 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) im[ch] += w * (F.colors[3 * ci + ch] * alb[ch]) + amb[ch] * alb[ch];
  }
  float g_im[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float w = 0.0f;
    if (hit && im[ch] > 0.0f) w = F.tonemap ? (float)F.gamma * powf(im[ch], (float)(F.gamma - 1.0)) : 1.0f;
    g_im[ch] = g_out[ch] * w;
  }

  float g_nf[3] = {0, 0, 0}, g_pf[3] = {0, 0, 0};
  float g_alb[3] = {0, 0, 0}, g_cf[3] = {0, 0, 0}, g_amb[3] = {0, 0, 0};     // leave as fp32 atomics: summed in fp32
  float g_cdf[3] = {0, 0, 0}, g_cdotnf = 0.0f;
  for (int l = 0; l < nlights; ++l) {
    LightTerms T;
    light_terms(l, T);
    const float ndotl = fmaxf(T.nd, 0.0f), rdotc = fmaxf(T.rd, 0.0f);
    const float P = spec_pow(rdotc);
    const float vl = (float)((vis >> l) & 1ull);
    const float w = (cf[0] * ndotl + cf[1] * P) * vl;          // the visible light's weight
    const int ci = clampi(F.lcidx[l], 0, F.ncolors - 1);
    float g_w = 0.0f, g_col[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float col = F.colors[3 * ci + ch];
      g_w += g_im[ch] * col * alb[ch];
      g_alb[ch] += g_im[ch] * (w * col + amb[ch]);
      g_col[ch] = g_im[ch] * w * alb[ch];
      g_amb[ch] += g_im[ch] * alb[ch];
    }
    g_w *= vl;                                                  // d im / d (unshadowed weight)
    g_cf[0] += g_w * ndotl;
    g_cf[1] += g_w * P;
    if (rdotc > 0.0f) g_cf[2] += (g_w * cf[1] * P) * logf(rdotc);
    const float g_nd = (T.nd > 0.0f) ? g_w * cf[0] : 0.0f;
    const float g_rd = (T.rd > 0.0f && cf[2] != 0.0f) ? g_w * cf[1] * cf[2] * powf(rdotc, cf[2] - 1.0f) : 0.0f;
    const float g_ldn = g_rd * sgnf * 2.0f * cdotnf + g_nd * sgnf * T.afac;
    g_cdotnf += g_rd * sgnf * 2.0f * T.ldn;
    const float g_cl = -g_rd * sgnf;
    const float g_afac = g_nd * sgnf * T.ldn;
    const float g_den = T.den_ok ? -g_afac * T.afac * T.afac : 0.0f;
    const float kl = F.latt ? F.latt[3 * l + 1] : 0.0f, kq = F.latt ? F.latt[3 * l + 2] : 0.0f;
    const float d2 = T.dist * T.dist;
    const float dp = (pw == 4) ? d2 * d2 : d2;
    const float ddp = (pw == 4) ? 4.0f * d2 * T.dist : 2.0f * T.dist;
    const float g_dist = g_den * (kl + kq * ddp);
    float g_lh[3], g_v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g_lh[k] = g_ldn * nf[k] + g_cl * cdf[k];
      g_nf[k] += g_ldn * T.lh[k];
      g_cdf[k] += g_cl * T.lh[k];
    }
    const float proj = (T.lh[0] * g_lh[0] + T.lh[1] * g_lh[1]) + T.lh[2] * g_lh[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g_v[k] = T.nz ? (g_lh[k] - T.lh[k] * proj) / T.dist + g_dist * T.lh[k] : g_lh[k];
      g_pf[k] -= g_v[k];
    }
    if (G.lights_pos) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float sum = wave_sum(g_v[k]);
        if (lane == 0 && sum != 0.0f) atomicAdd(G.lights_pos + 4 * l + k, sum);
      }
    }
    if (G.colors) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float sum = wave_sum(g_col[ch]);
        if (lane == 0 && sum != 0.0f) atomicAdd(G.colors + 3 * ci + ch, sum);
      }
    }
    if (G.attenuation) {
      const float ga[3] = {g_den, g_den * T.dist, g_den * dp};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float sum = wave_sum(ga[k]);
        if (lane == 0 && sum != 0.0f) atomicAdd(G.attenuation + 3 * l + k, sum);
      }
    }
  }
  // back to fp64 for the geometry chain below
  double g_n[3] = {(double)g_nf[0], (double)g_nf[1], (double)g_nf[2]}, g_p[3] = {(double)g_pf[0], (double)g_pf[1], (double)g_pf[2]};
  double g_cdir[3] = {(double)g_cdf[0], (double)g_cdf[1], (double)g_cdf[2]};
  const double g_cdotn = (double)g_cdotnf;
  // the extra outputs' upstream gradients, read here rather than at the top: nothing holds them across the light loops
  if (kAux && hit) {
    const size_t a = (row * (size_t)F.W + (size_t)cc) * 3;
    if (grad_normal) {
#pragma unroll
      for (int k = 0; k < 3; ++k) g_n[k] += (double)grad_normal[a + k];
    }
    if (grad_pos) {
#pragma unroll
      for (int k = 0; k < 3; ++k) g_p[k] += (double)grad_pos[a + k];
    }
  }
  if (kImage && G.ambient) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float sum = wave_sum((float)g_amb[ch]);
      if (lane == 0 && sum != 0.0f) atomicAdd(G.ambient + ch, sum);
    }
  }
  if (kImage) {
    // one material for the whole wave (the common case) -> one atomic per component; otherwise per lane
    const int m0 = __builtin_amdgcn_readfirstlane(m);
    const bool uniform = __builtin_amdgcn_ballot_w64(hit && m != m0) == 0ull;
    if (G.albedo) {
      if (uniform) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float sum = wave_sum((float)g_alb[ch]);
          if (lane == 0 && sum != 0.0f) atomicAdd(G.albedo + 3 * m0 + ch, sum);
        }
      } else if (hit) {
        add3(G.albedo + 3 * m, g_alb);
      }
    }
    if (G.coeffs) {
      if (uniform) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float sum = wave_sum((float)g_cf[k]);
          if (lane == 0 && sum != 0.0f) atomicAdd(G.coeffs + 3 * m0 + k, sum);
        }
      } else if (hit) {
        add3(G.coeffs + 3 * m, g_cf);
      }
    }
  }
  // ---- view direction and geometry: every lane takes part (run reduction below); lanes without a hit carry zeros ------
  double gA[3] = {0, 0, 0}, gB[3] = {0, 0, 0}, g_r = 0.0;
  // kCam: d/d eye through the view direction, d/d ray origin and d/d ray direction (zeros at pixels without a hit)
  double g_eye[3] = {0, 0, 0}, g_org[3] = {0, 0, 0}, g_d[3] = {0, 0, 0};
  if (kImage && hit) {
    // c^ . n^ and c^ = u / sqrt(|u|^2 + eps), u = o - p
#pragma unroll
    for (int k = 0; k < 3; ++k) { g_cdir[k] += g_cdotn * n[k]; g_n[k] += g_cdotn * cdir[k]; }
    const double projc = (cdir[0] * g_cdir[0] + cdir[1] * g_cdir[1]) + cdir[2] * g_cdir[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double g_u = (g_cdir[k] - cdir[k] * projc) * sc_inv;
      g_p[k] -= g_u;
      if (kCam) g_eye[k] = g_u;                            // u = eye - p: the eye itself, not the ray origin
    }
  }
  if (hit && type == SRH_PRIM_SPHERE) {
    const double proj = (n[0] * g_n[0] + n[1] * g_n[1]) + n[2] * g_n[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double g_v = (g_n[k] - n[k] * proj) * sph_inv;
      g_p[k] += g_v;
      gA[k] = -g_v;
    }
    const double g_t = ((g_p[0] * d[0] + g_p[1] * d[1]) + g_p[2] * d[2]) + g_dep;
    // oc = ray origin - centre: the record's eye-relative oc shifted by q0 (zero for perspective rays)
    const double oc[3] = {R[0] + q0[0], R[1] + q0[1], R[2] + q0[2]};
    const double cq = (R[3] + 2.0 * dot3(R, q0)) + dot3(q0, q0);
    const double a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const double b = 2.0 * dot3(oc, d);
    const double disc = b * b - 4.0 * a * cq;
    if (disc > 0.0) {
      const double root = sqrt(disc), inv2a = 1.0 / (2.0 * a);
      const double t1 = (-b - root) * inv2a;
      const double sg = (t1 >= 0.0) ? -1.0 : 1.0;       // the smaller non-negative root
      double g_b = -g_t * inv2a;
      const double g_disc = sg * g_t * inv2a / (2.0 * root);
      g_b += 2.0 * b * g_disc;
      const double g_cc = -4.0 * a * g_disc;
      g_r = -2.0 * (double)seg_ptr([](const SegDev& S) { return S.radius; })[li] * g_cc;
#pragma unroll
      for (int k = 0; k < 3; ++k) gA[k] -= 2.0 * oc[k] * g_cc + 2.0 * d[k] * g_b;  // oc = origin - c
      if (kCam) {
        // the origin enters through oc as the centre does, with the other sign; the direction through b = 2 oc.d and
        // a = d.d (t = (-b -/+ root) / 2a: d t / d a = -t / a - 4 cq d t / d disc)
        const double g_a = -g_t * t / a - 4.0 * cq * g_disc;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          g_org[k] = 2.0 * oc[k] * g_cc + 2.0 * d[k] * g_b;
          g_d[k] = 2.0 * oc[k] * g_b + 2.0 * d[k] * g_a;
        }
      }
    }
    if (kCam) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { g_org[k] += g_p[k]; g_d[k] += t * g_p[k]; }     // p = origin + t d
    }
  } else if (hit) {
    // planar: t = k/den, k = n^.(q - origin), den = n^.d
    const double g_t = ((g_p[0] * d[0] + g_p[1] * d[1]) + g_p[2] * d[2]) + g_dep;
    const double den = dot3(R, d);
    const double g_k = g_t / den, g_den = -g_t * t / den;
    const float* qp = (type == SRH_PRIM_TRIANGLE) ? seg_ptr([](const SegDev& S) { return S.face; }) + 12 * (size_t)li
                                                  : seg_ptr([](const SegDev& S) { return S.pos; }) + 4 * (size_t)li;
    double g_nh[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gA[k] = g_k * n[k];
      g_nh[k] = g_n[k] + g_k * ((double)qp[k] - org[k]) + g_den * d[k];
      if (kCam) { g_org[k] = g_p[k] - g_k * n[k]; g_d[k] = t * g_p[k] + g_den * n[k]; }   // p = origin + t d, k, den
    }
    // n^ = nin / sqrt(|nin|^2 + 3e-10) over xyz
    const float* np_ = seg_ptr([](const SegDev& S) { return S.normal; }) + 4 * (size_t)li;
    const double nin2 = (((double)np_[0] * np_[0] + 1e-10) + ((double)np_[1] * np_[1] + 1e-10)) + ((double)np_[2] * np_[2] + 1e-10);
    const double ninv = 1.0 / sqrt(nin2);
    const double proj = (n[0] * g_nh[0] + n[1] * g_nh[1]) + n[2] * g_nh[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) gB[k] = (g_nh[k] - n[k] * proj) * ninv;
  }
  if (kCam) {
    // Camera sums of this pixel: [0..2] d/d eye, [3..5] d/d bx, [6..8] d/d by, [9..11] the sum that gives
    // d/d bz.  Perspective: d = v / |v| with v = bx X + by Y - bz f and |v| = sqrt(X^2 + Y^2 + f^2) (orthonormal basis),
    // g_v = (g_d - d (d . g_d)) / |v|; the sums are g_org, X g_v, Y g_v, g_v.  Orthographic: origin = eye + bx X + by Y,
    // d = -bz; the sums are g_org, X g_org, Y g_org, g_d.
    double X, Y;
    pixel_plane_xy(F, pc, pr, X, Y);
    double cs[kCamSums];
    if (F.ortho) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { cs[k] = g_org[k] + g_eye[k]; cs[3 + k] = X * g_org[k]; cs[6 + k] = Y * g_org[k]; cs[9 + k] = g_d[k]; }
    } else {
      const double vinv = 1.0 / sqrt((X * X + Y * Y) + F.focal * F.focal);
      const double dg = (d[0] * g_d[0] + d[1] * g_d[1]) + d[2] * g_d[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double g_v = (g_d[k] - d[k] * dg) * vinv;
        cs[k] = g_org[k] + g_eye[k]; cs[3 + k] = X * g_v; cs[6 + k] = Y * g_v; cs[9 + k] = g_v;
      }
    }
    // wave sum, then the four waves through LDS in a fixed order, then ONE plain store per sum and workgroup: no atomics,
    // so the frame's result does not depend on the order in which workgroups finish
    __shared__ double cam_lds[4][kCamSums];
#pragma unroll
    for (int k = 0; k < kCamSums; ++k) {
      const double sum = wave_sum(cs[k]);
      if (lane == 0) cam_lds[threadIdx.y][k] = sum;
    }
    __syncthreads();
    if (threadIdx.y == 0 && lane < kCamSums)
      cam_part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kCamSums + lane] =
          (cam_lds[0][lane] + cam_lds[1][lane]) + (cam_lds[2][lane] + cam_lds[3][lane]);
  }
  scatter_primitive_grads(G, hit ? win : -1, lane, s, type, li, gA, gB, g_r);
}

template <bool kAux, bool kImage, bool kCam = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kBwdTchWaves))) void k_render_bwd_tch(FrameDev F, GradsDev G, const float* __restrict__ grad_image,
                                                         const float* __restrict__ grad_depth,
                                                         const int32_t* __restrict__ nearest,
                                                         const float* __restrict__ depth,
                                                         const uint64_t* __restrict__ visibility,
                                                         const float* __restrict__ grad_normal,
                                                         const float* __restrict__ grad_pos,
                                                         double* __restrict__ cam_part = nullptr) {
  render_bwd_tch_body<kAux, kImage, kCam>(F, G, grad_image, grad_depth, nearest, depth, visibility, grad_normal, grad_pos,
                                          cam_part);
}

// k_render_bwd_views for the torch backend's semantics: the body's variants with the view as grid dimension z.
// <false, true, false> (image plus optional depth gradient, no aux outputs, no camera) is srh_render_views_bwd's kernel;
// the kAux variants are srh_render_views_bwd_camera's.  `visibility` is the stacked (n_views, rows, W) bit field of the
// views' shadow passes, or NULL; `grad_normals` / `grad_poses` are the stacked dense (n_views, rows, W, 3) upstream
// gradients of the aux outputs, either NULL, offset per view like the image gradient; view v's camera partials start
// v * groups * kCamSums doubles into `cam_part` (groups = workgroups of one view: gridDim.x * gridDim.y).
template <bool kAux, bool kImage, bool kCam>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kBwdTchWaves))) void k_render_bwd_tch_views(
    const FrameDev* __restrict__ Fs, const GradsDev* __restrict__ Gs, const float* __restrict__ grad_images,
    const float* __restrict__ grad_depths, const int32_t* __restrict__ nearests, const float* __restrict__ depths,
    const uint64_t* __restrict__ visibility, const float* __restrict__ grad_normals,
    const float* __restrict__ grad_poses, double* __restrict__ cam_part) {
  const size_t v = blockIdx.z;
  const FrameDev& F = *(const FrameDev*)(as_constant(Fs) + v);
  const GradsDev& G = *(const GradsDev*)(as_constant(Gs) + v);
  const size_t rows = (size_t)(F.row1 - F.row0);
  const size_t aux_off = kAux ? v * rows * (size_t)F.W * 3 : 0;
  render_bwd_tch_body<kAux, kImage, kCam>(F, G, kImage ? grad_images + v * rows * F.img_stride : nullptr,
                                          grad_depths ? grad_depths + v * rows * F.depth_stride : nullptr,
                                          nearests + v * rows * F.near_stride, depths + v * rows * F.depth_stride,
                                          visibility ? visibility + v * rows * (size_t)F.W : nullptr,
                                          (kAux && grad_normals) ? grad_normals + aux_off : nullptr,
                                          (kAux && grad_poses) ? grad_poses + aux_off : nullptr,
                                          kCam ? cam_part + v * ((size_t)gridDim.x * gridDim.y) * kCamSums : nullptr);
}

// The frame's camera gradients from the workgroups' partial sums (one workgroup).  Thread (j, k) adds sum k of workgroups
// j, j + kCamFinishRows, ... in that order, the rows are added in order through LDS, and thread 0 applies the chain rule
// of the look-at basis in fp64 -- every addition has a fixed place, so two runs give the same bits.
//     z = unit(eye - at), u^ = unit(up), x = unit(cross(u^, z)), y = cross(z, x)          (torch/utils.py:402-427), unit
//     the reference's v / sqrt(sum(v_i^2 + 1e-10)) as camera_to_frame builds them: with `up` a fraction of a degree from
//     the view direction |cross(u^, z)|^2 is 1e-5 or less, the 3e-10 is 1e-5 of it, and the chain rule divides by that
//     length twice (tests/test_hip_grad_fuzz.py::test_up_a_tenth_of_a_degree_from_the_view_direction)
// persp: g_x = S1, g_y = S2, g_z = -f S3;  ortho: g_x = S1, g_y = S2, g_z = -S3;  g_eye = S0 + chain, g_at = -chain.
struct CamFinish {
  double eye[3], at[3], up[3], focal;
  int32_t ortho, ngroups;
  float* g_eye;
  float* g_at;
  float* g_up;
};
constexpr int kCamFinishRows = 85;                        // 85 x 12 = 1020 threads

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// g_v for u = v / len given g_u:  (g_u - u (u . g_u)) / len  -- exact for len = |v| and for len = eps_len(v) (srh_device.h) alike
// (d(v / n) = dv / n - v (v . dv) / n^3 with n^2 = |v|^2 + 3e-10)
__device__ __forceinline__ void unit_bwd(const double u[3], double len, const double g_u[3], double g_v[3]) {
  const double pr = dot3(u, g_u);
#pragma unroll
  for (int k = 0; k < 3; ++k) g_v[k] = (g_u[k] - u[k] * pr) / len;
}

// The body of k_camera_finish and k_camera_finish_views: one frame's finish P over its workgroups' partial sums.
// (A template over the kernel it serves: each instantiation has LDS arrays of its own, so each kernel's LDS layout is
// that of a kernel that declares them itself.)
template <bool kViews>
__device__ __forceinline__ void camera_finish_body(const CamFinish& P, const double* __restrict__ cam_part) {
  __shared__ double part[kCamFinishRows][kCamSums];
  __shared__ double S[kCamSums];
  const int tid = threadIdx.x;
  if (tid < kCamFinishRows * kCamSums) {
    const int j = tid / kCamSums, k = tid % kCamSums;
    double acc = 0.0;
    for (int g = j; g < P.ngroups; g += kCamFinishRows) acc += cam_part[(size_t)g * kCamSums + k];
    part[j][k] = acc;
  }
  __syncthreads();
  if (tid < kCamSums) {
    double acc = 0.0;
    for (int j = 0; j < kCamFinishRows; ++j) acc += part[j][tid];
    S[tid] = acc;
  }
  __syncthreads();
  if (tid != 0) return;
  double w[3], z[3], uh[3], cx[3], x[3];
  for (int k = 0; k < 3; ++k) w[k] = P.eye[k] - P.at[k];
  const double wl = eps_len(w), ul = eps_len(P.up);
  for (int k = 0; k < 3; ++k) { z[k] = w[k] / wl; uh[k] = P.up[k] / ul; }
  cross3(uh, z, cx);
  const double cl = eps_len(cx);
  for (int k = 0; k < 3; ++k) x[k] = cx[k] / cl;
  double g_x[3], g_y[3], g_z[3];
  for (int k = 0; k < 3; ++k) { g_x[k] = S[3 + k]; g_y[k] = S[6 + k]; g_z[k] = -(P.ortho ? 1.0 : P.focal) * S[9 + k]; }
  // y = cross(z, x)
  double t0[3], t1[3];
  cross3(x, g_y, t0);
  cross3(g_y, z, t1);
  for (int k = 0; k < 3; ++k) { g_z[k] += t0[k]; g_x[k] += t1[k]; }
  // x = cx / |cx|, cx = cross(u^, z)
  double g_cx[3], g_uh[3], g_up[3], g_w[3];
  unit_bwd(x, cl, g_x, g_cx);
  cross3(z, g_cx, g_uh);
  cross3(g_cx, uh, t0);
  for (int k = 0; k < 3; ++k) g_z[k] += t0[k];
  unit_bwd(uh, ul, g_uh, g_up);
  unit_bwd(z, wl, g_z, g_w);
  for (int k = 0; k < 3; ++k) {
    if (P.g_eye) P.g_eye[k] = (float)(S[k] + g_w[k]);
    if (P.g_at) P.g_at[k] = (float)(-g_w[k]);
    if (P.g_up) P.g_up[k] = (float)g_up[k];
  }
  if (P.g_eye) P.g_eye[3] = 0.0f;
  if (P.g_at) P.g_at[3] = 0.0f;
  if (P.g_up) P.g_up[3] = 0.0f;
}

__global__ __launch_bounds__(1024) void k_camera_finish(CamFinish P, const double* __restrict__ cam_part) {
  camera_finish_body<false>(P, cam_part);
}

// A batch of views per launch (srh_render_views_bwd_camera): one workgroup per view, view v = blockIdx.x finishes Ps[v]
// over its own slice of the partial sums, which starts v * ngroups * kCamSums doubles into `cam_part` (every view of a
// batch has the same ngroups).  Ps was written by a copy in front of the launch and is read as k_render_bwd_tch_views
// reads Fs.  A view that wants no camera gradient (three NULL destinations) leaves as a whole before the first barrier.
__global__ __launch_bounds__(1024) void k_camera_finish_views(const CamFinish* __restrict__ Ps,
                                                              const double* __restrict__ cam_part) {
  const size_t v = blockIdx.x;
  const CamFinish& P = *(const CamFinish*)(as_constant(Ps) + v);
  if (!P.g_eye && !P.g_at && !P.g_up) return;
  camera_finish_body<true>(P, cam_part + v * (size_t)P.ngroups * kCamSums);
}

}  // namespace srh
