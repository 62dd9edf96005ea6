// k_prep: the per-frame primitive records of the render backend (gfx950), and the binning of the primitives.
//
// One thread per primitive: the fp64 record (unit normal, plane offset, eye-relative centre, ...; layouts in
// srh_device.h), the fp32 reject record of the FAST and BINNED modes (srh_reject.h), and -- for a binned frame -- the
// primitive's tile box and its place in the bins (srh_binned.h).
#pragma once
#include "srh_binned.h"

namespace srh {

__device__ __forceinline__ void prep_record64(const SegDev& S, int type, int i, const double o[3], bool tch, double* R) {
  double nh[3] = {0, 0, 0};
  if (type != SRH_PRIM_SPHERE) {
    // ops.normalize: divide by the 4-D length, by 1 if that is zero (numpy/ops.py:18-26)
    const float* q = S.normal + 4 * (size_t)i;
    const double v[4] = {(double)q[0], (double)q[1], (double)q[2], (double)q[3]};
    double len = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
    // the torch backend normalises xyz only, with an eps inside the sum (torch/utils.py:131-135, :289)
    if (tch) len = eps_len(v);
    if (!(fabs(len) > 0.0)) len = 1.0;
    nh[0] = v[0] / len; nh[1] = v[1] / len; nh[2] = v[2] / len;
  }
  if (type == SRH_PRIM_SPHERE) {
    const float* c = S.pos + 4 * (size_t)i;
    const double r = (double)S.radius[i];
    const double oc[3] = {o[0] - (double)c[0], o[1] - (double)c[1], o[2] - (double)c[2]};
    R[0] = oc[0]; R[1] = oc[1]; R[2] = oc[2];
    R[3] = ((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - r * r;     // numpy/renderer.py:22
    return;
  }
  // point on the plane: pos, or vertex 0 of the triangle (numpy/renderer.py:107)
  const float* pp = (type == SRH_PRIM_TRIANGLE) ? S.face + 12 * (size_t)i : S.pos + 4 * (size_t)i;
  const double p[3] = {(double)pp[0], (double)pp[1], (double)pp[2]};
  // dist - n^.eye (numpy/renderer.py:62,69)
  const double dist = (p[0] * nh[0] + p[1] * nh[1]) + p[2] * nh[2];
  const double neye = (nh[0] * o[0] + nh[1] * o[1]) + nh[2] * o[2];
  R[0] = nh[0]; R[1] = nh[1]; R[2] = nh[2];
  R[3] = dist - neye;
  if (type == SRH_PRIM_DISK) {
    const double r = (double)S.radius[i];
    R[4] = p[0]; R[5] = p[1]; R[6] = p[2];
    R[7] = r * r;
  } else if (type == SRH_PRIM_TRIANGLE) {
    const float* f = S.face + 12 * (size_t)i;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const int w = (v + 1) % 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        R[4 + 3 * v + k] = (double)f[4 * v + k];
        R[13 + 3 * v + k] = (double)f[4 * w + k] - (double)f[4 * v + k];
      }
    }
    R[22] = 0.0; R[23] = 0.0;
  }
}

// Can no pixel of rows [row0, row1) see anything of the ball (centre x relative to the eye, radius rho)?  The ball's
// points have a in a0 +- rho |m_a| and g in g0 +- rho |m_g| (Cauchy-Schwarz) and lie on image row g / a; rays exist
// only through integer rows, hence the half-row slack.  A ball that reaches the eye plane (a <= 0) is kept.
__device__ inline bool ball_misses_slab(const FrameDev& F, const double x[3], double rho) {
  const double a0 = dot3(F.slab_ma, x), g0 = dot3(F.slab_mg, x);
  const double a_lo = a0 - rho * F.slab_na, a_hi = a0 + rho * F.slab_na;
  const double g_lo = g0 - rho * F.slab_ng, g_hi = g0 + rho * F.slab_ng;
  // fp64 side: a0 and g0 carry 2^-52 of their absolute terms.  The cull is used only while a_lo keeps 1e-6 of them
  // (relative error of a below 2^-32, of the rows below 1e-6 of a row: inside the half-row slack); a ball that far off
  // axis, or that cancelled (centre ~1e20 away, radius to match), is simply kept
  if (!(a_lo > 1.0e-6 * (abs_dot3(F.slab_ma, x) + rho * F.slab_na)) || !isfinite(a_hi + g_lo + g_hi)) return false;
  const double r_lo = g_lo / (g_lo >= 0.0 ? a_hi : a_lo), r_hi = g_hi / (g_hi >= 0.0 ? a_lo : a_hi);
  return r_hi < (double)F.row0 - 0.5 || r_lo > (double)F.row1 - 0.5;
}

// multi-GPU row slabs: most primitives project outside a rank's rows; they are recognised from their bounding ball
// before any of the per-frame records is computed, and are simply not binned (no list refers to their records)
__device__ inline bool primitive_misses_slab(const FrameDev& F, const SegDev& S, int i) {
  double x[3], rho;
  // numpy semantics, near <= 0: a sphere whose line a ray MISSES yields the valid distance 0 (Q2) -- on every pixel
  // of the image, wherever the sphere projects; it can never be culled
  if (S.type == SRH_PRIM_SPHERE && !(F.near_clip > 0.0)) return false;
  if (S.type == SRH_PRIM_DISK || S.type == SRH_PRIM_SPHERE) {
    const float* c = S.pos + 4 * (size_t)i;
    for (int k = 0; k < 3; ++k) x[k] = (double)c[k] - F.o[k];
    rho = fabs((double)S.radius[i]);
  } else if (S.type == SRH_PRIM_TRIANGLE) {
    const float* f = S.face + 12 * (size_t)i;
    double cen[3];
    for (int k = 0; k < 3; ++k) cen[k] = ((double)f[k] + (double)f[4 + k] + (double)f[8 + k]) / 3.0;
    rho = 0.0;
    for (int v = 0; v < 3; ++v) {
      const double w[3] = {(double)f[4 * v] - cen[0], (double)f[4 * v + 1] - cen[1], (double)f[4 * v + 2] - cen[2]};
      rho = fmax(rho, sqrt(dot3(w, w)));
    }
    rho *= 1.0000001;
    for (int k = 0; k < 3; ++k) x[k] = cen[k] - F.o[k];
  } else {
    return false;
  }
  return ball_misses_slab(F, x, rho);
}

// TYPE = the batch's primitive type (the host launches the matching instantiation): the fp64 record and the reject
// record are built in REGISTERS, stored once, and the tile box and the bin placement work from the register copies --
// a thread never waits for its own stores to come back (measured: the kernel was 76 % s_waitcnt).
template <int TYPE>
__device__ __forceinline__ void prep_body(const FrameDev& F, int s, double* rec64, float* rec32) {
  const SegDev& S = F.seg[s];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.count) return;
  // which set of frame-wide list lengths this frame counts into (srh_device.h: kLargeNext); stable for the whole binning
  // (the same word for every lane: kept in a scalar register, the vector ones are all taken while the record is built)
  const uint32_t set = F.tilerange ? ((uint32_t)__builtin_amdgcn_readfirstlane((int)F.counters[kLargeNext]) & 1u) : 0u;
  if (s == 0 && i == 0) {
    if (F.tilerange) F.counters[kLargeNow] = set;          // ... and the render kernel reads the same one
    // per-frame fp64 copy of the lights for the fragment stage: position, colour looked up through color_idx
    double* L = const_cast<double*>(F.lights64);
    for (int l = 0; l < F.nlights; ++l) {
      const int ci = clampi(F.lcidx[l], 0, F.ncolors - 1);
      for (int k = 0; k < 3; ++k) {
        L[6 * l + k] = (double)F.lpos[4 * l + k];
        L[6 * l + 3 + k] = (double)F.colors[3 * ci + k];
      }
    }
  }
  if (F.tilerange && F.slab_cull && primitive_misses_slab(F, S, i)) {
    uint16_t* tr = F.tilerange + 4 * (size_t)(S.first + i);
    tr[0] = 1; tr[1] = 0; tr[2] = 0; tr[3] = 0;                   // not binned
    return;
  }
  constexpr int N64 = kRec64Stride[TYPE], N32 = kRec32Stride[TYPE];
  double R[N64];
  prep_record64(S, TYPE, i, F.o, F.shading != 0, R);
  // screen-space reject record of the FAST / binned modes, from the fp64 record
  float Q[N32];
  const PixelBasis B = pixel_basis(F);
  const bool near_pos = F.near_clip > 0.0;
  ConicExtent conic = no_extent();
  // (a disc's STORED word [10] is the occlusion cull's V; Q[10] stays hi_u for bin_place below: srh_reject.h, layouts)
  float stored10 = 0.0f;
  if (TYPE == SRH_PRIM_DISK) disk_reject_record(R, F.o, B, F.W, F.H, F.near_clip, F.far_clip, Q, &conic, &stored10);
  else if (TYPE == SRH_PRIM_SPHERE) sphere_reject_record(R, B, F.W, F.H, near_pos, F.shading != 0, Q, &conic);
  else if (TYPE == SRH_PRIM_TRIANGLE) triangle_reject_record(R, F.o, B, F.W, F.H, near_pos, Q);
  else plane_reject_record(R, B, F.W, F.H, Q);
  {
    double2* r2 = reinterpret_cast<double2*>(rec64 + (size_t)i * N64);      // records are 16-byte aligned (strides 4, 8, 24)
#pragma unroll
    for (int k = 0; k < N64 / 2; ++k) r2[k] = make_double2(R[2 * k], R[2 * k + 1]);
    float4* q4 = reinterpret_cast<float4*>(rec32 + (size_t)i * N32);
#pragma unroll
    for (int k = 0; k < N32 / 4; ++k) {
      const float w2 = (TYPE == SRH_PRIM_DISK && k == 2) ? stored10 : Q[4 * k + 2];
      q4[k] = make_float4(Q[4 * k], Q[4 * k + 1], w2, Q[4 * k + 3]);
    }
  }
  if (F.tilerange) {
    // light views: a primitive that comes within near_ball of the eye can block a shadow ray from BEHIND the light
    // (the reference accepts hits up to 0.1 beyond it); its screen-space shape says nothing about that, so every
    // query tests it
    bool near_eye = false;
    if (F.near_ball > 0.0) {
      // distance from the light to the nearest point the primitive can have, as a difference of two lengths -- which
      // cancels for a primitive as large as it is far (centre 1e20 away, radius 1e20): 2^-46 of the lengths' sum,
      // 64x their rounding, comes off
      double dmin = 0.0, mag = 0.0;
      if (TYPE == SRH_PRIM_DISK) {
        const double oc[3] = {F.o[0] - R[4], F.o[1] - R[5], F.o[2] - R[6]};
        const double dc = sqrt(dot3(oc, oc)), rr = sqrt(fabs(R[7]));
        dmin = dc - rr; mag = dc + rr;
      }
      else if (TYPE == SRH_PRIM_SPHERE) {
        // (the radius itself: |oc|^2 - (|oc|^2 - r^2) gives r^2 back only to 2^-52 |oc|^2)
        const double dc = sqrt(dot3(R, R)), rr = fabs((double)S.radius[i]);
        dmin = dc - rr; mag = dc + rr;
      }
      else if (TYPE == SRH_PRIM_TRIANGLE) {
        double far2 = 0.0, near2 = 1.0e300;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const double w[3] = {R[4 + 3 * v] - F.o[0], R[5 + 3 * v] - F.o[1], R[6 + 3 * v] - F.o[2]};
          near2 = fmin(near2, dot3(w, w));
          const double e[3] = {R[13 + 3 * v], R[14 + 3 * v], R[15 + 3 * v]};
          far2 = fmax(far2, dot3(e, e));
        }
        dmin = sqrt(near2) - sqrt(far2);                        // every point is within one edge length of a vertex
        mag = sqrt(near2) + sqrt(far2);
      }
      dmin -= 1.4210854715202004e-14 * mag;
      near_eye = !(dmin > F.near_ball);                         // NaN -> large
      // what the shadow pass skips candidates by: no point of the primitive is closer to the light than this (rounded
      // DOWN to fp32; 0 = unknown: planes, non-finite geometry)
      const float nd = (TYPE != SRH_PRIM_PLANE && dmin > 0.0 && dmin < 1.0e30) ? (float)dmin * 0.999999f : 0.0f;
      F.neardist[S.first + i] = nd;
    }
    const TileBox box = bin_primitive(F, s, TYPE, Q, conic, S.first + i, set, near_eye);
    if (box.tx0 <= box.tx1) bin_place(F, s, TYPE, S.first, Q, S.first + i, box.tx0, box.ty0, box.tx1, box.ty1, set);
  }
}

// Four waves per SIMD (at most 128 VGPRs), asked for explicitly: left alone hipcc takes what it likes -- 150 registers for
// the disc instantiation once the fp64 trust terms of srh_reject.h went in, three waves per SIMD -- and the prep waves of
// the frames in flight then hold their slots longer beside the render waves: config 5 went from 0.078 to 0.093 ms per
// frame on that alone.  At 128 the compiler needs no spills.
// The prep waves run at the render waves' issue priority.  Raised (s_setprio 1 or 3 as the kernels' first instruction) they
// are 13 us shorter beside the render waves, which get 3-4 us longer each: the steady state loses 1 % (DESIGN Part II).
constexpr int kPrepWaves = 4;
template <int TYPE>
__global__ __launch_bounds__(kBinBlock) __attribute__((amdgpu_waves_per_eu(kPrepWaves))) void k_prep(FrameDev F, int s, double* rec64, float* rec32) {
  // the frame's constants into the workspace, where the render kernel reads them (FrameDev::self; srh_binned.h)
  if (F.self && s == 0 && blockIdx.x == 0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&F);
    uint32_t* dst = reinterpret_cast<uint32_t*>(F.self);
    for (unsigned i = threadIdx.x; i < sizeof(FrameDev) / 4; i += kBinBlock) dst[i] = src[i];
  }
  prep_body<TYPE>(F, s, rec64, rec32);
}

template <int TYPE>
__global__ __launch_bounds__(kBinBlock) __attribute__((amdgpu_waves_per_eu(kPrepWaves))) void k_prep_views(const FrameDev* __restrict__ Fs, int s) {
  const FrameDev& F = Fs[blockIdx.y];
  prep_body<TYPE>(F, s, const_cast<double*>(F.seg[s].rec64), const_cast<float*>(F.seg[s].rec32));
}

}  // namespace srh
