// Screen-space reject records of the FAST / BINNED render modes (gfx950).
//
// For a pinhole camera the set of pixels whose ray *line* meets a disc (or a sphere) is the interior of
// a conic in pixel coordinates, the inside of a triangle is the intersection of three half planes, and
// n^.D is affine in the pixel coordinates.  k_prep derives those screen-space shapes per primitive and per
// frame in fp64, inflates them by a margin that covers every fp32 rounding on the evaluation side, and
// stores them as fp32 "reject records".  The render kernels evaluate the cheap fp32 tests per
// (pixel, primitive) pair and send only the survivors to the fp64 intersection of srh_device.h.  A pair
// that fails a reject test is provably not the winner of the fp64 path, so every mode's output is
// bit-identical to the all-pairs fp64 mode.
//
// Pixel coordinates are (c, r) = (column, row) indices of the full image; the un-normalised ray
// direction is affine in them:  D(c, r) = D0 + c*Dc + r*Dr   (numpy/renderer.py:152-164).
//
// rec32 layouts (floats)
//   disc (12)      [0] c0 [1] r0 [2] A11 [3] 2*A12 [4] A22 : candidate iff
//                  dc*(A11*dc + 2A12*dr) + A22*dr*dr - 1 <= 0,  dc = c - c0, dr = r - r0
//                  (A = 0: "always a candidate" -- the disc's image is not an ellipse, etc.)
//                  [5..7] u0 u1 u2 [9] lo_u [10] hi_u : depth estimate, see plane_estimate_record
//                  [8] U [11] s_in : occlusion fields, see disk_reject_record
//                  The STORED word [10] is V, the occlusion cull's lower bound of 1 / t (disk_reject_record), not hi_u:
//                  hi_u is read by k_prep alone (RectTest, on the thread's register copy of the record), and no kernel
//                  reads word [10] of a stored disc record -- the binned sweeps, slow path and re-sweep evaluate
//                  [0..7] (pair_bounds), the sort [8], the sorted sweep [10] as V and [11], the fast mode [0..4]; the
//                  shadow pass takes the light views' bins and the fp64 records, the backward pass no reject record at
//                  all; a render-only call (SRH_STAGE_RENDER) runs the same render kernels on the stored records.
//   sphere (12)   [0..4] as the disc; [5] upper bound of 1 / t for the whole sphere (1e30: none)
//   triangle (16)  {a_i, b_i, g_i} at [4i..4i+2], i < 3: candidate iff min_i(a_i*c + b_i*r + g_i) >= 0
//                  [3] u0 [7] u1 [11] u2 [13] lo_u [14] hi_u
//   plane (8)      [0..2] u0 u1 u2 [4] lo_u [5] hi_u; candidate iff den > hi_u
//
// Depth estimate of a planar primitive (disc, triangle, plane): the ray distance is
//   t = k |D| / (n^.D),   n^.D = v0 + c*v1 + r*v2   with v_j = n^.{D0, Dc, Dr}   (affine in the pixel coordinates)
#pragma once
#include "srh_device.h"

namespace srh {

constexpr int kRec32Stride[4] = {12, 8, 12, 16};

struct PixelBasis {   // D(c,r) = D0 + c*Dc + r*Dr
  double D0[3], Dc[3], Dr[3];
};

__device__ __host__ inline PixelBasis pixel_basis(const FrameDev& F) {
  PixelBasis B;
  for (int i = 0; i < 3; ++i) {
    B.D0[i] = (-F.half_w * F.bx[i] + F.half_h * F.by[i]) - F.focal * F.bz[i];
    B.Dc[i] = (F.step_x * F.half_w) * F.bx[i];
    B.Dr[i] = (F.step_y * F.half_h) * F.by[i];
  }
  return B;
}

__device__ inline double abs_dot3(const double* a, const double* b) {
  return fabs(a[0] * b[0]) + fabs(a[1] * b[1]) + fabs(a[2] * b[2]);
}

__device__ inline void rec_zero(float* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = 0.0f;
}

// ---- cheap reciprocals and roots ---------------------------------------------------------------------
// An IEEE fp64 division costs k_prep about 11 vector instructions and a square root about 15; rcp_newton and
// rsqrt_newton (srh_device.h) cost 3 and 5.  Nothing below needs a correctly rounded result: the values feed fp32 records
// whose margins are 2^-22 and wider.  kFastEps = 2^-44 is the relative error every comment below grants ONE of these
// operations, the product formed with it included.  tools/ubench_newton.hip measures them against the IEEE results
// over the whole exponent range (profiles/prep_div_ubench.txt): the largest error found is 2^-47.7, a factor of 13
// inside kFastEps, and each margin cited below covers kFastEps itself with room to spare.
// Outside the positive normal range the refined value is NaN where the IEEE one is 0 or inf (x = 0, inf, a result that
// over- or underflows).  Where the surrounding code already sends a NaN down its "no record" branch (every test there
// is written !(x > ...)) the bare functions are used; the *_fast forms below return the hardware seed's IEEE special
// value instead.
__device__ __forceinline__ double rcp_fast(double x) {          // 1 / x
  const double y = rcp_newton(x);
  return (y == y) ? y : __builtin_amdgcn_rcp(x);
}
__device__ __forceinline__ double rsqrt_fast(double x) {        // 1 / sqrt(x)
  const double y = rsqrt_newton(x);
  return (y == y) ? y : __builtin_amdgcn_rsq(x);
}
__device__ __forceinline__ double sqrt_fast(double x) {         // sqrt(x); +-0 and +inf come back as they are
  const double y = x * rsqrt_newton(x);
  return __builtin_amdgcn_class(x, 0x260) ? x : y;
}

// Depth-estimate fields of a planar primitive with unit normal n and plane offset k (see the file header):
//   u_j = w_j / K  with  w0 = s v0 + E, w1 = s v1, w2 = s v2,  s = sign(k),  K = |k| (1 - 2^-20),  and lo_u, hi_u.
// The kernel evaluates den = u0 + c u1 + r u2 = (s (n^.D) + E) / K up to an fp32 error below E / K, where
//   E = 2^-19 (|v0| + W |v1| + H |v2|)  covers the three rounded coefficients and the two fmas of the vector path
// (5 x 2^-24) and, with 2x slack, the matrix-core sweep that was measured and dropped (DESIGN.md Part II A.2; the
// margin still covers it): the constant moved to the tile origin by two more fmas, every coefficient split into three
// bfloat16 parts (2^-24 of itself left over) and nine exact products summed in fp32 (at most 16 x 2^-24 together) --
// so s (n^.D) / K <= den always.  A valid hit with near > 0 has s (n^.D) > 0 and ray distance
//   t = |k| |D| / (s n^.D) >= |D| / ((1 - 2^-20) max(den, lo_u))      for ANY lo_u > 0
// (the 2^-20 absorbs the roundings of |D|, the reciprocal and the product).  The kernel uses exactly that,
//   lower bound = |D| rcp(max(den, lo_u)),   lo_u = 1025 E / K:
// clamping at lo_u keeps the bound finite and positive where the plane is seen edge-on (it is then simply weak).
//   den <= hi_u = -1023 E / K   provably t < 0: never a valid hit when near > 0 (used to cull tiles, and per pixel
//                               for planes, whose every pixel is otherwise a candidate)
// An estimate that cannot be represented (plane through the eye, overflow) is WITHDRAWN: u0 = 1e30, u1 = u2 = 0
// make den huge everywhere, i.e. "as near as can be", which ranks the candidate first -- it is then confirmed,
// not trusted.
__device__ inline void plane_estimate_record(const double n[3], double k, const PixelBasis& B, int W, int H,
                                             float* u0, float* u1, float* u2, float* unused, float* lo_u,
                                             float* hi_u) {
  const double a = dot3(n, B.D0), b = dot3(n, B.Dc), c = dot3(n, B.Dr);
  const double sg = (k > 0.0) ? 1.0 : ((k < 0.0) ? -1.0 : 0.0);
  // fp64 side: a, b, c carry 2^-52 of the ABSOLUTE terms they were summed from, and so does the n^.d the exact path
  // divides k by (hit_*64) -- where the plane is seen edge-on over the whole image these exceed 2^-21 of the values
  // themselves, so the slack also holds 2^-48 of the absolute terms (32x the rounding of either side)
  const double e = 1.9073486328125e-6 * (fabs(a) + fabs(b) * W + fabs(c) * H) +
                   3.552713678800501e-15 * (abs_dot3(n, B.D0) + abs_dot3(n, B.Dc) * W + abs_dot3(n, B.Dr) * H);
  const double K = fabs(k) * (1.0 - 9.5367431640625e-7);
  // ONE reciprocal of K for the six quotients (kFastEps each; K = 0, denormal or inf makes it NaN or inf and the
  // estimate is withdrawn below, as with the division).  u0, u1, u2: together they move den by at most
  // kFastEps (|w0| + W |w1| + H |w2|) / K < 2^-24 E / K, and E = 32 x 2^-24 (...) spends 5 of its 32 units on the
  // vector path.  lo_u may be ANY positive number; hi_u has 1023 units of E / K where it needs 2.
  const double iK = rcp_newton(K);
  const double big = (fabs(a) + e + fabs(b) * W + fabs(c) * H) * iK, lo = 1025.0 * e * iK;
  *unused = 0.0f;
  if (!(K > 0.0) || !isfinite(big) || !(big < 1.0e30) || !(lo > 1.0e-30)) {
    *u0 = 1.0e30f;
    *u1 = *u2 = 0.0f;
    *lo_u = 3.0e38f;
    *hi_u = -3.0e38f;
    return;
  }
  *u0 = (float)((sg * a + e) * iK); *u1 = (float)(sg * b * iK); *u2 = (float)(sg * c * iK);
  *lo_u = (float)lo * 1.0000002f;
  *hi_u = (float)(-1023.0 * e * iK) * 1.0000002f;
}

// Conic x^T T x <= 0, x = (1, c, r)  ->  inflated, normalised ellipse record out[0..4] (out[11] = 0: the quadratic form
//   dc (A11 dc + 2A12 dr) + A22 dr^2 - 1 <= 0,  dc = c - c0, dr = r - r0).
// Returns false (record = "always a candidate") when the conic is not a
// well-conditioned ellipse: not positive definite, centre or size beyond 2^20 pixels, or axis ratio > 512
// (a disc seen edge-on; its parameters are then numerical noise).
//
// ONE form for every ellipse (until round 3 elongated ones were stored in a principal-axes form).  The record is
// evaluated in two ways, and the inflation `thr` covers both:
//   vector path   centre-relative in fp32 (pair_bounds, ellipse_reject): three rounded coefficients and five rounded
//                 operations on terms up to Tm near the boundary;
//   matrix path   (measured and dropped, DESIGN.md Part II A.2; the inflation still covers it) as the polynomial
//                 a0 + a1 x + a2 y + a3 x^2 + a4 x y + a5 y^2 in TILE-LOCAL pixel coordinates x, y in [0, 15]: coefficients moved to the tile origin in fp32 (six rounded operations),
//                 each split into two float16 parts (2^-22 of itself left over), twelve exact products summed in fp32.
//                 Its terms reach the form's value, with absolute values, 15 pixels beyond the tile origin; a binned
//                 tile starts at most 17 pixels outside the ellipse's box.
// Tm = A11 X^2 + 2|A12| X Y + A22 Y^2 + 1 with X = hc + 34, Y = hr + 34 (hc, hr = half extents of the box) bounds the
// sum of the absolute terms of either evaluation; each commits at most 2.6 * 2^-20 Tm, `rel` is 2^-18 Tm.  A point
// inside the true ellipse has A d.d <= 1, hence value <= 1 / thr - 1 <= -rel / (1 + rel) after the inflation.
//
// `sure_in` (optional) receives the INWARD counterpart: an fp32 value q < sure_in of the kernel's evaluation (with its
// -1.00000024, pair_bounds) proves that the pixel lies inside the ellipse with room to spare -- the value carries at most
// rel + 2^-22 of evaluation error, the centre moves by at most delta, and what is left shrinks the radius by another
// (grow - 1) + 2^-10 of itself for the fp64 path's own roundings (twice the position slack the outward margin grants
// them, plus 2^-10).  -1e30 when nothing is provably inside.
// Half extents, in pixels, of the box of a stored ellipse record around its centre (rec[0], rec[1]); hc < 0: the record
// is "always a candidate", no box.  conic_record has them at hand, conic_bbox makes the box of them.  (fp32, rounded
// up: they wait in registers while the rest of the record is built, and k_prep has none to spare.)
struct ConicExtent { float hc, hr; };
__device__ inline ConicExtent no_extent() { return ConicExtent{-1.0f, -1.0f}; }

// n / d from id = rcp_newton(d): one residual step on the quotient leaves 2^-52 (kFastEps^2 and one rounding), so
// several quotients share one reciprocal and still carry no more than an IEEE division and one further rounding
__device__ __forceinline__ double quot_refined(double n, double d, double id) {
  const double q = n * id;
  return __builtin_fma(__builtin_fma(-d, q, n), id, q);
}

// `ext` receives the half extents of the stored record's box (none when there is no record): see the end.
__device__ inline bool conic_record(double T00, double T01, double T02, double T11, double T12, double T22,
                                    int W, int H, float* out, ConicExtent* ext, double* sure_in = nullptr) {
  if (sure_in) *sure_in = -1.0e30;
  rec_zero(out, 5);
  out[11] = 0.0f;
  *ext = no_extent();
  const double det = T11 * T22 - T12 * T12;
  if (!(T11 > 0.0) || !(det > 0.0) || !isfinite(T00 + T01 + T02 + T11 + T12 + T22)) return false;
  // Centre: F0 below is first-order sensitive to it, so the two quotients keep 2^-52 (quot_refined) -- one rounding more
  // than the products of F0 commit on the same terms.  det denormal or inf: NaN, no record.
  const double idet = rcp_newton(det);
  const double c0 = quot_refined(-(T22 * T01 - T12 * T02), det, idet);
  const double r0 = quot_refined(-(T11 * T02 - T12 * T01), det, idet);
  const double F0 = T00 + T01 * c0 + T02 * r0;                 // value at the centre, < 0 inside
  if (!(F0 < 0.0)) return false;
  // iF and `it` below scale the whole form: kFastEps each, against the 1.4 x 2^-20 Tm that rel keeps spare (see above)
  const double iF = -rcp_newton(F0);
  const double A11 = T11 * iF, A12 = T12 * iF, A22 = T22 * iF;
  // IEEE root: lmin cancels, and the two limits below decide whether the disc keeps this record
  const double mean = 0.5 * (A11 + A22), dev = sqrt(0.25 * (A11 - A22) * (A11 - A22) + A12 * A12);
  const double lmax = mean + dev, lmin = mean - dev;
  if (!(lmin > 0.0) || !isfinite(lmax)) return false;
  // semi-axes smin = 1 / sqrt(lmax) <= smax = 1 / sqrt(lmin): the limits smax < 2^20 and smax <= 512 smin are taken
  // on the eigenvalues themselves (powers of two: exact), no root and no quotient
  const double far_lim = 1048576.0;
  if (!(fabs(c0) < far_lim) || !(fabs(r0) < far_lim) || !(lmin > 9.094947017729282e-13)) return false;
  if (!(lmax <= 262144.0 * lmin)) return false;
  const double dA = A11 * A22 - A12 * A12;
  if (!(dA > 0.0)) return false;
  // half extents of the un-inflated ellipse: kFastEps on each of idA and the two roots, 2^-42 of Tm together -- rel's
  // spare again.  (An underflowing operand gives NaN, thr is then NaN too: no record.)
  const double idA = rcp_newton(dA);
  const double hx2 = A22 * idA, hy2 = A11 * idA;
  const double hx = hx2 * rsqrt_newton(hx2), hy = hy2 * rsqrt_newton(hy2);
  const double X = hx + 34.0, Y = hy + 34.0;
  const double Tm = A11 * X * X + 2.0 * fabs(A12) * X * Y + A22 * Y * Y + 1.0;
  // Position: c0, r0 are rounded to fp32 (2^-24 |c0|) and so is c - c0 (2^-24 (W + |c0|)), together
  // < 2^-23 (|c0| + |r0| + W + H) pixels; delta doubles that and adds 2^-12 px.
  const double pos_err = 2.384185791015625e-7 * (fabs(c0) + fabs(r0) + W + H);
  const double delta = 0.000244140625 + pos_err;
  const double rel = 3.814697265625e-6 * Tm;
  // 1 / smin = sqrt(lmax), lmax in [2^-40, inf): kFastEps of grow - 1, which holds twice the position error it needs
  const double grow = 1.0 + delta * (lmax * rsqrt_newton(lmax));
  const double thr = grow * grow * (1.0 + rel);
  // (a convention, not a bound: a form inflated a million-fold rejects nothing worth its test, and the record is
  // conservative on either side of the limit -- thr's own kFastEps needs no cover here)
  if (!(thr < 1.0e6)) return false;
  const double it = rcp_newton(thr);
  out[0] = (float)c0;
  out[1] = (float)r0;
  out[2] = (float)(A11 * it);
  out[3] = (float)(2.0 * A12 * it);
  out[4] = (float)(A22 * it);
  const double shrink = 1.0 - 2.0 * (grow - 1.0) - 9.765625e-4;
  if (sure_in && shrink > 0.0) *sure_in = shrink * shrink * it - 1.0 - rel - 4.76837158203125e-7;
  // Box of the STORED form, from the half extents at hand: those of the inflated fp64 form are sqrt(thr) (hx, hy).  The
  // stored coefficients are that form's rounded to fp32 (2^-24 each; they are normal numbers: lmin / thr > 2^-60), so
  // with p = A11 A22, q = A12^2 the stored determinant is at least (p - q) (1 - x), x = 2.0000002 x 2^-24 (p + q) / (p - q),
  // and its half extents are at most sqrt((1 + 2^-24) / (1 - x)) <= (1 + 2^-24) (1 + x) times those (x <= 0.6;
  // here (p + q) / (p - q) <= 2 lmax / lmin <= 2^19, x <= 2^-4).  The factor below holds x with 1.001 for the 2^-33 that
  // dA's own cancellation and idA leave on it, and 2^-22 for the 2^-24, the three kFastEps and every fp64 rounding on
  // either side: the extents are at least those of the stored coefficients (what conic_bbox computed from the record
  // until they were handed over), whose box contains every pixel the record can pass.  Round ellipses pay 2^-21 of
  // their size.  (A12 alone may round to a denormal fp32: 2^-150 absolute, nothing against p - q > 2^-120.)
  const double x = 1.1933e-7 * ((A11 * A22 + A12 * A12) * idA);
  const double widen = (thr * rsqrt_newton(thr)) * (1.0 + 2.384185791015625e-7 + x);
  const double hc = hx * widen, hr = hy * widen;
  if (hc < 1.0e30 && hr < 1.0e30) *ext = ConicExtent{(float)hc * 1.0000002f, (float)hr * 1.0000002f};
  return true;
}

// Upper bound of 1 / t for every hit inside the ball of radius r around the point at eye-relative position -oc:
// t >= |oc| - r (the ball's nearest point).  1e30 ("no estimate") when the eye is inside or on the ball.
// fp64 side: |oc| - r cancels when the eye is close to the ball's surface relative to its size, and the exact path's
// own distance (q = oc + t d against r^2, or the sphere's root -b - sqrt(b^2 - 4 a c)) is then off by up to
// 2^-24 (|oc| + r) (square root of 2^-51 of the squared terms): the bound gives up 2^-22 (|oc| + r), four times that.
// l = |oc| and r may come from sqrt_fast: kFastEps (l + r) is 2^-20 of the three parts of 2^-24 (l + r) left over.
// The reciprocal carries kFastEps under the outward factor 1 + 2^-20 in front of it (the cast and the last product are
// covered by the 1.0000002f, as before); a denormal tmin makes it NaN, which is "no estimate".
__device__ inline float ball_inverse_depth_bound(double l, double r) {
  const double tmin = (l - r) - 2.384185791015625e-7 * (l + fabs(r));
  if (!(tmin > 0.0) || !isfinite(tmin)) return 1.0e30f;
  const double inv = (1.0 + 9.5367431640625e-7) * rcp_newton(tmin);
  return (inv < 1.0e30) ? (float)inv * 1.0000002f : 1.0e30f;
}

// is[j] = 1 / |P_j| (0 for a zero or non-finite column): the units conic_trusted compares in.  tmax and emax carry the
// SAME factors is[i] is[j], so their kFastEps moves each maximum by 2^-43 of itself at most -- against the factor 4
// between the 2^-26 the margins cover and the 2^-24 the test asks for.
__device__ inline void inverse_lengths(const double* const P[3], double is[3]) {
  for (int j = 0; j < 3; ++j) {
    const double l2 = dot3(P[j], P[j]);
    is[j] = (l2 > 0.0) ? rsqrt_fast(l2) : 0.0;
  }
}

// Can the six fp64 coefficients of a conic be trusted?  `tmax` = largest |T_ij|, `emax` = largest sum of the absolute
// values of the terms T_ij was formed from (before they cancelled): the evaluation error is a few 2^-53 emax, and the
// margins of conic_record cover coefficient errors of 2^-26 of the conic's scale -- so trust needs tmax > 2^-24 emax.
// The entries live on different scales (x = (1, c, r): T_ij carries |Pi| |Pj|, and |Dc| is a pixel pitch), so both are
// taken in units of |Pi| |Pj|.
// (A disc with centre y = -1e20 and radius 1e20 passes through the scene, |oc|^2 and r^2 agree to the last bit, and
// the coefficients are rounding noise that happened to look like a small ellipse; found by the non-finite fuzz with
// seed 2002.)  Not trusted -> the record stays "always a candidate".
__device__ inline bool conic_trusted(double tmax, double emax) {
  return isfinite(emax) && tmax * 16777216.0 > emax;
}

// sphere silhouette  cq (Pi.Pj) - (oc.Pi)(oc.Pj)  with the trust test; `sq` = magnitude of the terms cq was formed from
// `ext`: see conic_record
__device__ inline void sphere_conic_record(const double oc[3], double cq, double sq, const double* const P[3], int W, int H,
                                           float* out, ConicExtent* ext) {
  double w[3], mw[3], is[3];
  inverse_lengths(P, is);                                  // entries are compared in units of |Pi| |Pj| (see below)
  for (int j = 0; j < 3; ++j) {
    w[j] = dot3(oc, P[j]); mw[j] = abs_dot3(oc, P[j]);
  }
  double t[6], tmax = 0.0, emax = 0.0;
  int q = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j, ++q) {
      t[q] = cq * dot3(P[i], P[j]) - w[i] * w[j];
      tmax = fmax(tmax, fabs(t[q]) * (is[i] * is[j]));
      emax = fmax(emax, (sq * abs_dot3(P[i], P[j]) + mw[i] * fabs(w[j]) + mw[j] * fabs(w[i]) + fabs(w[i] * w[j])) *
                            (is[i] * is[j]));
    }
  if (!conic_trusted(tmax, emax)) { rec_zero(out, 5); out[11] = 0.0f; *ext = no_extent(); return; }
  (void)conic_record(t[0], t[1], t[2], t[3], t[4], t[5], W, H, out, ext);
}

// disc: | oc (n.D) + k D |^2 <= r^2 (n.D)^2   (numpy/renderer.py:69,85-88 with t = k / (n.D))
// Occlusion fields (the front-to-back sweep of the binned disc kernel, srh_binned.h):
//   [8]  U = upper bound of 1 / t over every valid hit (ball_inverse_depth_bound; 1e30: none)
//   [11] s_in: a pixel whose fp32 value q (pair_bounds) is < s_in is a CERTAIN valid hit (conic_record's sure_in) --
//        only for a trusted, non-degenerate ellipse with finite, moderate coefficients whose whole ball lies inside
//        [near, far] with margin; -1e30 (never) otherwise.
//   `v_out` (the STORED record's word [10], see the layout above; out[10] itself keeps hi_u for the binning):
//        V = lower bound of 1 / t over every valid hit of a disc that has certain hits (s_in > -1e30); 1e30 for every
//        other disc, so that it never lowers the sweep's running minimum.  See kFarBoundMargin.
// `ext`: the half extents of the stored shape's box (conic_record), none when the record is "always a candidate".
// V = kFarBoundMargin / ((l + r) + slack), cast and rounded DOWN.  Every hit lies in the ball: t <= |oc| + r.  `slack` is
// 2^-20 (l + r): the kFastEps of l and of r (2^-44 of them) and the 2^-22 (l + r) by which the fp64 path's own distance may
// differ from the geometric one (ball_inverse_depth_bound) together stay below 2^-21.9 (l + r).  The factor 1 - 2^-20
// stands in front of the Newton reciprocal (kFastEps), its product with it (2^-53) and the cast to fp32 (2^-24, then
// pushed down by the 0.9999999f): 2^-23.9 of the 2^-20 are used.
constexpr double kFarBoundMargin = 1.0 - 9.5367431640625e-7;
__device__ inline void disk_reject_record(const double* R, const double o[3], const PixelBasis& B, int W, int H,
                                          double near_clip, double far_clip, float* out, ConicExtent* ext,
                                          float* v_out) {
  const double* n = R;
  const double k = R[3];
  const double oc[3] = {o[0] - R[4], o[1] - R[5], o[2] - R[6]};
  const double r2 = R[7];
  const double* P[3] = {B.D0, B.Dc, B.Dr};
  // mu: |terms of u| summed over the components, au: |u| (L1).  The exact path forms q = (eye + t d) - c
  // (hit_disk64, the reference's order): its eye + t d carries 2^-53 (|eye| + |t d|), which in the units of u = q (n.D)
  // is |eye| |n.P| + |k| |P| -- so |eye| joins the terms, and a camera 1e10 away from the origin makes the record
  // untrusted instead of wrong
  double nu[3], u[3][3], mu[3], au[3], is[3];
  inverse_lengths(P, is);
  const double ol1 = fabs(o[0]) + fabs(o[1]) + fabs(o[2]);
  for (int j = 0; j < 3; ++j) {
    nu[j] = dot3(n, P[j]);
    mu[j] = au[j] = 0.0;
    for (int a = 0; a < 3; ++a) {
      u[j][a] = oc[a] * nu[j] + k * P[j][a];
      mu[j] += fabs(oc[a] * nu[j]) + fabs(k * P[j][a]);
      au[j] += fabs(u[j][a]);
    }
    mu[j] += ol1 * fabs(nu[j]);
  }
  double t[6], tmax = 0.0, emax = 0.0;
  {
    int q = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j, ++q) {
        t[q] = dot3(u[i], u[j]) - r2 * nu[i] * nu[j];
        tmax = fmax(tmax, fabs(t[q]) * (is[i] * is[j]));
        emax = fmax(emax, (mu[i] * au[j] + mu[j] * au[i] + abs_dot3(u[i], u[j]) + fabs(r2 * nu[i] * nu[j])) *
                              (is[i] * is[j]));
      }
  }
  bool degenerate = true;
  double sure_in = -1.0e30;
  *ext = no_extent();
  if (conic_trusted(tmax, emax))
    degenerate = !conic_record(t[0], t[1], t[2], t[3], t[4], t[5], W, H, out, ext, &sure_in);
  // ONE |oc| and ONE radius for the stand-in below, the occlusion bound and the certain hits (sqrt_fast: see
  // ball_inverse_depth_bound and `slack`)
  const double oo = dot3(oc, oc);
  const double l = sqrt_fast(oo), r = sqrt_fast(r2);
  if (degenerate) {
    // The disc's own image is not a usable ellipse (seen edge-on: axis ratio beyond 512, parameters are noise).
    // Every hit lies on the disc, hence inside the sphere around its centre with its radius, and that sphere's
    // silhouette is a robust, well-conditioned ellipse.  Rare (|cos| < 2e-3), so the extra work is off the common path.
    sphere_conic_record(oc, oo - r2, oo + fabs(r2) + 2.0 * sqrt(dot3(o, o) * oo), P, W, H, out, ext);
  }
  plane_estimate_record(n, k, B, W, H, out + 5, out + 6, out + 7, out + 8, out + 9, out + 10);
  // A stand-in shape passes pixels the disc does not cover, and the plane-distance estimate means nothing there:
  // replace it by the bounding ball's (every hit lies in the ball, so t >= |oc| - r).  The kernel multiplies den by
  // 1 / |D|, so the constant is scaled by the largest |D| of the image (|D| is convex: a corner) -- a little weak, valid.
  if (degenerate) {
    double dmax2 = 0.0;
    for (int i = 0; i < 4; ++i) {
      const double c = (i & 1) ? (double)(W - 1) : 0.0, rr = (i & 2) ? (double)(H - 1) : 0.0;
      const double D[3] = {B.D0[0] + c * B.Dc[0] + rr * B.Dr[0], B.D0[1] + c * B.Dc[1] + rr * B.Dr[1],
                           B.D0[2] + c * B.Dc[2] + rr * B.Dr[2]};
      dmax2 = fmax(dmax2, dot3(D, D));
    }
    // (the root is monotone: one of the largest square; its kFastEps is under the 1.000001)
    const double u = (double)ball_inverse_depth_bound(l, r) * sqrt_fast(dmax2) * 1.000001;
    out[5] = (u < 1.0e30 && isfinite(u)) ? (float)u * 1.0000002f : 1.0e30f;
    out[6] = out[7] = 0.0f; out[9] = 3.0e38f; out[10] = -3.0e38f;
  }
  out[8] = ball_inverse_depth_bound(l, r);
  // certain hits: every point of the ball (hence every fp64 hit, whose distance ball_inverse_depth_bound's 2^-22 covers)
  // lies in [near, far], and the record's values stay finite at every pixel (no inf - inf, no NaN sign bit to read).
  // `slack` is 2^-20 (l + r) where 2^-22 (l + r) is needed: the kFastEps of l and r is 2^-24 of what is left.
  const double slack = 9.5367431640625e-7 * (l + r);
  bool sure = !degenerate && near_clip > 0.0 && (l - r) - slack > near_clip && (l + r) + slack < far_clip &&
              sure_in > -1.0 && out[9] < 1.0e30f;
  for (int i = 0; i < 11; ++i) sure = sure && fabsf(out[i]) < 1.0e30f;
  sure = sure && fabsf(out[2]) < 1.0e6f && fabsf(out[3]) < 1.0e6f && fabsf(out[4]) < 1.0e6f;
  out[11] = sure ? (float)sure_in : -1.0e30f;
  // `sure` has (l + r) + slack positive and below far_clip.  A disc WITH certain hits must never keep the 1e30 of one
  // without: a value beyond 1e30 is capped there (still a lower bound), and a NaN (denormal operand of the Newton
  // reciprocal) becomes 0, with which the sweep skips nothing.
  const double v = kFarBoundMargin * rcp_newton((l + r) + slack);
  const float vf = (v < 1.0e30) ? (float)v * 0.9999999f : 1.0e30f;
  *v_out = sure ? ((v == v) ? vf : 0.0f) : 1.0e30f;
}

// sphere: the ray's line meets it iff (oc.D)^2 - |D|^2 (|oc|^2 - r^2) >= 0   (numpy/renderer.py:20-25).
// With near <= 0 a missed line yields the valid t = 0 (Q2), so nothing may be rejected.
__device__ inline void sphere_reject_record(const double* R, const PixelBasis& B, int W, int H, bool near_positive,
                                            bool tch, float* out, ConicExtent* ext) {
  rec_zero(out, 12);
  out[5] = 1.0e30f;
  *ext = no_extent();
  if (!near_positive) return;
  const double* oc = R;
  const double cq = R[3];
  const double* P[3] = {B.D0, B.Dc, B.Dr};
  double w[3];
  for (int j = 0; j < 3; ++j) w[j] = dot3(oc, P[j]);
  // cq = |oc|^2 - r^2 comes from the exact record: the terms it was formed from are at most 2 |oc|^2 + |cq|
  const double oo = dot3(oc, oc);
  sphere_conic_record(oc, cq, 2.0 * oo + fabs(cq), P, W, H, out, ext);
  // Depth bound.  Eye outside the sphere (cq > 0): both roots have the sign of (pos - eye).D = -oc.D.  Positive roots
  // give t = t1 >= |oc| - r.  Negative roots are a miss under the torch semantics, but the numpy backend's sentinel
  // turns them into t = 1.0 (Q2) -- so there the bound holds only if -oc.D > 0 on the whole image (affine: its
  // minimum is at a corner); otherwise it is capped at t >= min(|oc| - r, 1).
  if (cq > 0.0) {
    float inv = ball_inverse_depth_bound(sqrt_fast(oo), sqrt_fast(fmax(oo - cq, 0.0)));
    if (!tch) {
      double front = 1e300;
      for (int i = 0; i < 4; ++i) {
        const double c = (i & 1) ? (double)(W - 1) : 0.0, rr = (i & 2) ? (double)(H - 1) : 0.0;
        front = fmin(front, -(w[0] + c * w[1] + rr * w[2]));
      }
      if (!(front > 0.0)) inv = fmaxf(inv, 1.000001f);
    }
    out[5] = inv;
  }
}

// triangle: for a valid hit (t >= near > 0) sign(n.D) = sign(k), so edge i is satisfied iff
// sign(k) * (s_i n + k m_i) . D >= 0 with m_i = n x e_i, s_i = (o - v_i) . m_i   (numpy/renderer.py:114-126)
//
// fp64 side.  E_i(D) = sg (s_i n + k m_i) . D is a scalar triple product expanded, and it cancels when vertices lie far
// away on two axes (terms |o - v| |e| ~ 1e40 for a result ~ 1e20): the coefficients computed here, and the value
// dot(cross(e_i, p - v_i), n^) the exact path computes per pixel, then both differ from E_i by rounding noise that has
// nothing to do with the fp32 margin.  Both are bounded through the ABSOLUTE terms: with am_j = |n_a e_b| + |n_b e_a|
// (terms of m_j), as = sum_j (|o_j| + |v_j|) am_j (terms of s) and Dsum >= every |D_j| of the image,
//   |computed E_i - E_i|,  |exact path's value * (n^.D) - E_i|   <=   2^-48 (2 as + |k| sum_j am_j) Dsum  =: err
// (32x the 2^-53 of each rounding; the exact path's own terms are the same ones: its p - v_i carries
// 2^-53 (|o| + |v| + |t d|), its n^.d another 2^-51, which multiplies s_i).  `err`, in pixels after the
// normalisation, is added to the edge's margin; an edge whose noise reaches a quarter pixel stays "always a candidate".
__device__ inline void triangle_reject_record(const double* R, const double o[3], const PixelBasis& B, int W, int H,
                                              bool near_positive, float* out) {
  rec_zero(out, 16);
  for (int i = 0; i < 3; ++i) out[4 * i + 2] = 1.0f;          // a = b = 0, g = 1: always a candidate
  const double* n = R;
  const double k = R[3];
  plane_estimate_record(n, k, B, W, H, out + 3, out + 7, out + 11, out + 12, out + 13, out + 14);
  if (!near_positive) return;
  const double sg = (k > 0.0) ? 1.0 : ((k < 0.0) ? -1.0 : 0.0);
  double dsum = 0.0;
  for (int j = 0; j < 3; ++j) dsum += fabs(B.D0[j]) + fabs(B.Dc[j]) * W + fabs(B.Dr[j]) * H;
  for (int i = 0; i < 3; ++i) {
    const double* v = R + 4 + 3 * i;
    const double* e = R + 13 + 3 * i;
    const double m[3] = {n[1] * e[2] - n[2] * e[1], n[2] * e[0] - n[0] * e[2], n[0] * e[1] - n[1] * e[0]};
    const double am[3] = {fabs(n[1] * e[2]) + fabs(n[2] * e[1]), fabs(n[2] * e[0]) + fabs(n[0] * e[2]),
                          fabs(n[0] * e[1]) + fabs(n[1] * e[0])};
    const double ov[3] = {o[0] - v[0], o[1] - v[1], o[2] - v[2]};
    const double s = dot3(ov, m);
    const double as = (fabs(o[0]) + fabs(v[0])) * am[0] + (fabs(o[1]) + fabs(v[1])) * am[1] + (fabs(o[2]) + fabs(v[2])) * am[2];
    const double w[3] = {sg * (s * n[0] + k * m[0]), sg * (s * n[1] + k * m[1]), sg * (s * n[2] + k * m[2])};
    double a = dot3(w, B.Dc), b = dot3(w, B.Dr), g = dot3(w, B.D0);
    const double len2 = a * a + b * b;
    if (!(len2 > 0.0) || !isfinite(len2) || !isfinite(g)) continue;
    // ONE reciprocal length for the four quotients: kFastEps of a, b and g against the 1.7 x 3 x 2^-24 (|g| + W + H)
    // that the margin below keeps spare, and of `err`, whose constant is 32x the rounding it stands for
    const double ilen = rsqrt_newton(len2);
    const double err = 3.552713678800501e-15 * (2.0 * as + fabs(k) * (am[0] + am[1] + am[2])) * dsum * ilen;   // pixels
    if (!(err < 0.25)) continue;
    a *= ilen; b *= ilen; g *= ilen;                          // signed distance to the edge line, pixels
    if (!(fabs(g) < 1.0e9)) continue;
    // fp32 evaluation of a*c + b*r + g with rounded a, b, g: error < 3 * 2^-24 (|g| + W + H); margin 2.7x that
    g += 0.000244140625 + 4.76837158203125e-7 * (fabs(g) + W + H) + err;
    out[4 * i + 0] = (float)a;
    out[4 * i + 1] = (float)b;
    out[4 * i + 2] = (float)g;
  }
}

__device__ inline void plane_reject_record(const double* R, const PixelBasis& B, int W, int H, float* out) {
  rec_zero(out, 8);
  plane_estimate_record(R, R[3], B, W, H, out + 0, out + 1, out + 2, out + 3, out + 4, out + 5);
}

// fp32 evaluation of the ellipse record for N pixels of one row: value <= 0 means "candidate".
template <int N>
__device__ __forceinline__ void ellipse_reject(const float* __restrict__ R, const float (&cf)[N], float rf,
                                               float (&q)[N]) {
  const float dr = rf - R[1];
  const float ee = R[3] * dr;
  const float gg = __builtin_fmaf(R[4] * dr, dr, -1.0f);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float dc = cf[j] - R[0];
    q[j] = __builtin_fmaf(dc, __builtin_fmaf(R[2], dc, ee), gg);
  }
}

// ---- conservative pixel bounding boxes of the reject shapes (for tile binning) ------------------------
struct BBox {
  double c0, c1, r0, r1;   // inclusive pixel range that contains every true hit of the primitive
  bool full;               // no useful bound: treat as covering the whole image
};

__device__ inline BBox bbox_full() { return BBox{0, 0, 0, 0, true}; }

// Box of the stored ellipse record from the extents its record function handed over, one pixel of slack.
__device__ inline BBox conic_bbox(const float* rec, const ConicExtent& e) {
  if (!(e.hc >= 0.0f)) return bbox_full();
  const double hc = e.hc, hr = e.hr;
  return BBox{(double)rec[0] - hc - 1.0, (double)rec[0] + hc + 1.0, (double)rec[1] - hr - 1.0, (double)rec[1] + hr + 1.0,
              false};
}

// Box of the triangle cut out by the three stored (inflated) edge half-planes, if it is bounded.
// Three half-planes a_i c + b_i r + g_i >= 0 with unit normals bound a region iff the normals turn the same way round
// from each to the next (all three cross products of one sign): otherwise some direction leaves none of them, and the
// region is a wedge, a strip or a half-plane.  The latter is what a huge triangle seen from near its plane looks like:
// its far edges all project onto the plane's HORIZON, three nearly identical lines -- whose pairwise "intersections"
// are rounding noise that used to pass for a tiny triangle somewhere off the image, and the primitive was then not
// binned at all (found by the adversarial campaign, seed 3505 scene 2238; tests/test_hip_adversarial.py).  Cross
// products below 1e-5 are refused too: a corner is (g_i n_j - g_j n_i) / D with |g| up to 1e9 pixels.
__device__ inline BBox triangle_bbox(const float* rec) {
  double a[3], b[3], g[3];
  for (int i = 0; i < 3; ++i) {
    a[i] = rec[4 * i]; b[i] = rec[4 * i + 1]; g[i] = rec[4 * i + 2];
    if (a[i] == 0.0 && b[i] == 0.0) return bbox_full();
  }
  const double D01 = a[0] * b[1] - a[1] * b[0], D12 = a[1] * b[2] - a[2] * b[1], D20 = a[2] * b[0] - a[0] * b[2];
  const bool ccw = D01 > 1.0e-5 && D12 > 1.0e-5 && D20 > 1.0e-5, cw = D01 < -1.0e-5 && D12 < -1.0e-5 && D20 < -1.0e-5;
  if (!ccw && !cw) return bbox_full();
  double cmin = 1e300, cmax = -1e300, rmin = 1e300, rmax = -1e300;
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    const double D = a[i] * b[j] - a[j] * b[i];
    const double c = (-g[i] * b[j] + g[j] * b[i]) / D;
    const double r = (-a[i] * g[j] + a[j] * g[i]) / D;
    if (!isfinite(c) || !isfinite(r)) return bbox_full();
    if (!(a[k] * c + b[k] * r + g[k] >= -1e-6 * (fabs(c) + fabs(r) + fabs(g[k]) + 1.0))) return bbox_full();
    cmin = fmin(cmin, c); cmax = fmax(cmax, c); rmin = fmin(rmin, r); rmax = fmax(rmax, r);
  }
  // the corners carry the rounding of the division: 2^-52 (|g_i| + |g_j|) / |D| pixels, far below the pixel of slack
  // for |g| < 1e9 and |D| > 1e-5 only if |g| stays below ~1e6 -- beyond that the slack grows with it
  const double gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
  const double slack = 1.0 + 1.0e-10 * gmax;
  return BBox{cmin - slack, cmax + slack, rmin - slack, rmax + slack, false};
}

// Can a pixel of the rectangle [c0,c1] x [r0,r1] (inclusive pixel coordinates) be a valid hit of the primitive whose
// reject record this is?  Used to drop tiles of a primitive's box that it cannot reach (box corners of round or
// slanted shapes, tiles where its plane is behind the eye).  Two proofs of "no":
//   shape   true hits lie inside the stored (inflated) reject shape, so the exact fp64 minimum of the stored
//           ellipse form over the rectangle being > 1, or one stored triangle edge function being negative at all
//           four corners, rules the rectangle out;
//   plane   den is affine, so its maximum sits at a corner; evaluated in fp64 on the stored coefficients it is
//           >= the true scaled s (n^.D), and a value <= hi_u means t < 0 everywhere (only used when near > 0).
struct RectTest {
  int type;
  bool ellipse, behind;
  double x0, y0, A11, A12, A22, i11, i22;       // ellipse centre, quadratic form, 1 / A11, 1 / A22
  double ea[3], eb[3], eg[3];                   // triangle edge functions
  double u0, u1, u2, hi;                        // depth-estimate denominator

  __device__ inline RectTest(int type_, const float* rec, bool near_positive) : type(type_), ellipse(false), behind(false) {
    if (type == SRH_PRIM_TRIANGLE) {
      for (int i = 0; i < 3; ++i) { ea[i] = rec[4 * i]; eb[i] = rec[4 * i + 1]; eg[i] = rec[4 * i + 2]; }
      u0 = rec[3]; u1 = rec[7]; u2 = rec[11]; hi = rec[14];
      behind = near_positive;
    } else if (type == SRH_PRIM_DISK || type == SRH_PRIM_SPHERE) {
      A11 = rec[2]; A12 = 0.5 * (double)rec[3]; A22 = rec[4];
      ellipse = (A11 > 0.0) && (A22 > 0.0);                    // else "always a candidate"
      // only the clamped vertices of `reaches` use them: a vertex off by kFastEps of itself raises the form's value
      // there by 2^-88 A v^2 <= 2^-69 (the form is about 1 where it matters, A v^2 <= 2^19 of that) -- under the 1e-6
      i11 = ellipse ? rcp_newton(A11) : 0.0;
      i22 = ellipse ? rcp_newton(A22) : 0.0;
      x0 = rec[0]; y0 = rec[1];
      if (type == SRH_PRIM_DISK) { u0 = rec[5]; u1 = rec[6]; u2 = rec[7]; hi = rec[10]; behind = near_positive; }
    }
  }

  __device__ inline bool reaches(double c0, double c1, double r0, double r1) const {
    if (behind && u0 + fmax(u1 * c0, u1 * c1) + fmax(u2 * r0, u2 * r1) <= hi) return false;
    if (type == SRH_PRIM_TRIANGLE) {
      for (int i = 0; i < 3; ++i)
        if (ea[i] * (ea[i] > 0.0 ? c1 : c0) + eb[i] * (eb[i] > 0.0 ? r1 : r0) + eg[i] < 0.0) return false;
      return true;
    }
    if (!ellipse) return true;
    if (x0 >= c0 && x0 <= c1 && y0 >= r0 && y0 <= r1) return true;
    // centre outside: the minimum of the form over the rectangle is on its boundary; per edge the form is a
    // parabola in the free coordinate, minimised at its clamped vertex
    double qmin = 1e300;
    for (int e = 0; e < 2; ++e) {
      const double dc = (e ? c1 : c0) - x0;
      const double dr = fmin(fmax(-A12 * dc * i22, r0 - y0), r1 - y0);
      qmin = fmin(qmin, A11 * dc * dc + 2.0 * A12 * dc * dr + A22 * dr * dr);
      const double dr2 = (e ? r1 : r0) - y0;
      const double dc2 = fmin(fmax(-A12 * dr2 * i11, c0 - x0), c1 - x0);
      qmin = fmin(qmin, A11 * dc2 * dc2 + 2.0 * A12 * dc2 * dr2 + A22 * dr2 * dr2);
    }
    return !(qmin > 1.000001);
  }

  // the `behind` expression of `reaches`, operation for operation, with the row term handed in:
  // rterm = fmax(u2 * r0, u2 * r1)
  __device__ __forceinline__ double den_max(double c0, double c1, double rterm) const {
    return u0 + fmax(u1 * c0, u1 * c1) + rterm;
  }
};

// ---- row spans of a stored ellipse (bin_place) --------------------------------------------------------------------------
// The candidate region q(dc, dr) = A11 dc^2 + 2 A12 dc dr + A22 dr^2 <= lambda (lambda = 1.000001, the threshold of
// `reaches`) is convex: over the band dr in [a, b] of one tile row its columns are ONE interval [lo, hi], and a tile of
// that row is reached iff its own column interval meets it.  For a fixed dr the region is
//   dc in (-A12 dr -+ sqrt(lambda A11 - det dr^2)) / A11,      det = A11 A22 - A12^2,
// empty beyond |dr| > dr_max = sqrt(lambda A11 / det).  The upper branch is concave in dr with its maximum
// dc_max = sqrt(lambda A22 / det) at dr* = -A12 dc_max / A22, the lower one is its mirror image (convex, minimum at
// -dr*): hi is the upper branch at clamp(dr*, a, b), lo the lower one at clamp(-dr*, a, b).  Every column between lo and
// hi has a dr in the band with q <= lambda, so the tiles found are exactly those whose exact minimum of q is <= lambda.
//
// Rounding.  A11, A12, A22 are fp32 values: the products of det are exact in fp64, det carries one rounding.  An error
// eta A11 on the radicand is the same as lambda moved by eta (a few 2^-52: one fma on terms <= lambda A11).  The
// reciprocals and roots are the Newton forms (kFastEps each, see above): with |A12 dr| / A11 and the root / A11 both
// <= dc_max they move lo and hi by less than 2^-42 dc_max; dr* is a stationary point of either branch, its error enters
// squared.  The sums with the centre (|x0| < 2^20 (1 + 2^-24): conic_record's far_lim and the fp32 store) and with the pad
// and the tile edge round three times, half an ulp each: 3 x 2^-53 (2^20 + dc_max + 32) = 0.375 x 2^-30 + 3 x 2^-53 dc_max
// pixels.  The span is widened OUTWARD by
//   m = 2^-30 (1 + dc_max) pixels                               (folded into the centre: xl = x0 - m, xh = x0 + m):
// its constant part is 2.6 times the roundings' at the 2^20-pixel limit (1300 times at |x0| = 2048), its dc_max part 4000
// times that of the fast forms and the roundings together; dr_max takes the factor 1 + 2^-30.  lambda itself stands 1e-6
// above the 1 a true hit can reach (conic_record's inflation is not touched), so the result is a superset of the tiles whose exact
// minimum is <= 1; the widening raises q at the span's ends by 2 sqrt(lambda A11) m at most (|dq / ddc| <= 2 sqrt(A11 q)),
// that is 2^-29 (sqrt(A11) + sqrt(A11 A22 / det)): 1e-6 for an ellipse 1/512 pixel thin, 2^-20 for axis ratio 512.
// The floor / ceil that turn lo and hi into tile indices are monotone and tile edges are integers: they only err outward.
//
// `usable` is false -- the caller keeps the per-tile loop -- when the record is no ellipse, det is not safely positive
// (below 2^-30 A11 A22; conic_record's axis-ratio limit keeps stored forms above 2^-17) or an extent is not finite.
struct ConicSpans {
  bool usable;
  double det, lam11, nA12, i11, dr_max, dr_star, xl, xh;

  __device__ inline explicit ConicSpans(const RectTest& T) : usable(false) {
    if (!T.ellipse) return;
    const double p = T.A11 * T.A22;
    det = p - T.A12 * T.A12;
    if (!(det > 9.313225746154785e-10 * p)) return;
    const double idet = rcp_newton(det);
    const double cx2 = 1.000001 * T.A22 * idet, ry2 = 1.000001 * T.A11 * idet;
    const double dc_max = cx2 * rsqrt_newton(cx2), ry = ry2 * rsqrt_newton(ry2);
    if (!(dc_max < 1.0e30) || !(ry < 1.0e30)) return;            // NaN, inf: the Newton forms over- or underflowed
    const double m = 9.313225746154785e-10 * (1.0 + dc_max);
    dr_star = -T.A12 * dc_max * T.i22;
    dr_max = ry * (1.0 + 9.313225746154785e-10);
    lam11 = 1.000001 * T.A11; nA12 = -T.A12; i11 = T.i11;
    xl = T.x0 - m; xh = T.x0 + m;
    usable = true;
  }

  // sqrt(max(x, 0)) for a radicand of the size of lam11 (a stored A11 is above 2^-60, conic_record): clamped at 1e-200
  // instead of 0 -- a root of 1e-100 where it should be 0 -- which keeps the Newton form clear of rsq(0) = inf
  static __device__ __forceinline__ double root(double x) {
    const double xm = fmax(x, 1.0e-200);
    return xm * rsqrt_newton(xm);
  }

  // column extent [lo, hi] (full-image pixel coordinates, widened) over the band dr in [a, b]; false: the band is empty
  __device__ __forceinline__ bool row(double a, double b, double* lo, double* hi) const {
    if (!(a <= dr_max) || !(b >= -dr_max)) return false;
    const double dR = fmin(fmax(dr_star, a), b), dL = fmin(fmax(-dr_star, a), b);
    const double sR = root(__builtin_fma(-det * dR, dR, lam11)), sL = root(__builtin_fma(-det * dL, dL, lam11));
    *hi = __builtin_fma(__builtin_fma(nA12, dR, sR), i11, xh);
    *lo = __builtin_fma(__builtin_fma(nA12, dL, -sL), i11, xl);
    return true;
  }
};

}  // namespace srh
