// Error check (MI355X): rcp_newton, rsqrt_newton (srh_device.h) and the forms k_prep builds from them (srh_reject.h)
// against the IEEE results 1.0 / x, 1.0 / sqrt(x), sqrt(x), n / x.  Prints the largest relative difference per operand class and
// the number of results whose class (finite / zero / inf / NaN) differs from the IEEE one.
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -I include -I surf_renderer_amd/csrc \
//         tools/ubench_newton.hip -o build/ubench/newton && build/ubench/newton
// Operand classes (x = m 2^e, m uniform in [1, 2)):
//   records    e in [-140, 140]: what k_prep's records hold -- squares and determinants of fp32 scene data and pixel counts
//   normal     e in [-1021, 1021]: every exponent at which operand and result are both normal numbers
//   edges      e within 3 of the ends of the normal range, denormal operands, and operands whose reciprocal is denormal;
//              only the class mismatches and the error of the *_fast forms mean anything here
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <cstring>
#include "srh_reject.h"

__device__ uint64_t rng(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

// relative difference as the bits of a non-negative double (they order like integers); results of different class -> `bad`
__device__ void cmp(double got, double want, unsigned long long& worst, unsigned long long& bad) {
  const bool fg = isfinite(got) && got != 0.0, fw = isfinite(want) && want != 0.0;
  if (!fg || !fw) {
    if (!(got == want || (got != got && want != want))) ++bad;
    return;
  }
  const double rel = fabs(got - want) / fabs(want);
  const unsigned long long b = (unsigned long long)__double_as_longlong(rel);
  if (b > worst) worst = b;
}

constexpr int kForms = 7;   // rcp_newton, rsqrt_newton, x * rsqrt_newton, n * rcp_newton, rcp_fast, rsqrt_fast, sqrt_fast

__global__ void k(unsigned long long* worst, unsigned long long* bad, int iters, int mode) {
  uint64_t s = 0x9E3779B97F4A7C15ull * (blockIdx.x * blockDim.x + threadIdx.x + 1) + (uint64_t)mode;
  unsigned long long w[kForms] = {}, nb[kForms] = {};
  for (int it = 0; it < iters; ++it) {
    const double m = 1.0 + (double)(rng(s) >> 12) * 2.220446049250313e-16;
    const double n = (1.0 + (double)(rng(s) >> 12) * 2.220446049250313e-16) * ((rng(s) & 1) ? -1.0 : 1.0);
    int e;
    if (mode == 0) e = (int)(rng(s) % 281) - 140;
    else if (mode == 1) e = (int)(rng(s) % 2043) - 1021;
    else {
      const int q = (int)(rng(s) % 4), d = (int)(rng(s) % 4);
      e = (q == 0) ? -1022 + d : (q == 1) ? 1023 - d : (q == 2) ? -1023 - (int)(rng(s) % 51) : 1020 + d;
    }
    const double x = ldexp(m, e);
    cmp(srh::rcp_newton(x), 1.0 / x, w[0], nb[0]);
    cmp(srh::rsqrt_newton(x), 1.0 / sqrt(x), w[1], nb[1]);
    cmp(x * srh::rsqrt_newton(x), sqrt(x), w[2], nb[2]);
    cmp(n * srh::rcp_newton(x), n / x, w[3], nb[3]);
    cmp(srh::rcp_fast(x), 1.0 / x, w[4], nb[4]);
    cmp(srh::rsqrt_fast(x), 1.0 / sqrt(x), w[5], nb[5]);
    cmp(srh::sqrt_fast(x), sqrt(x), w[6], nb[6]);
  }
  for (int f = 0; f < kForms; ++f) {
    atomicMax(&worst[f], w[f]);
    if (nb[f]) atomicAdd(&bad[f], nb[f]);
  }
}

// the special operands themselves, one thread: *_fast must return what IEEE returns
__global__ void k_special(unsigned long long* bad) {
  const double xs[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, -1.0, 4.9406564584124654e-324, 1.7976931348623157e308};
  unsigned long long nb = 0, unused = 0;
  for (double x : xs) {
    cmp(srh::rcp_fast(x), 1.0 / x, unused, nb);
    if (!(x < 0.0)) cmp(srh::rsqrt_fast(x), 1.0 / sqrt(x), unused, nb);
    cmp(srh::sqrt_fast(x), sqrt(x), unused, nb);
  }
  *bad = nb;
}

int main() {
  const char* forms[kForms] = {"rcp_newton(x)      vs 1/x      ", "rsqrt_newton(x)    vs 1/sqrt(x)", "x*rsqrt_newton(x)  vs sqrt(x)  ",
                               "n*rcp_newton(x)    vs n/x      ", "rcp_fast(x)        vs 1/x      ", "rsqrt_fast(x)      vs 1/sqrt(x)",
                               "sqrt_fast(x)       vs sqrt(x)  "};
  const char* modes[3] = {"records (2^-140..2^140)", "normal (2^-1021..2^1021)", "edges (ends of the range, denormals)"};
  unsigned long long *worst, *bad;
  if (hipMalloc(&worst, 8 * kForms) != hipSuccess || hipMalloc(&bad, 8 * kForms) != hipSuccess) { printf("no device\n"); return 1; }
  const int blocks = 4096, threads = 256, iters = 1024;
  for (int mode = 0; mode < 3; ++mode) {
    (void)hipMemset(worst, 0, 8 * kForms); (void)hipMemset(bad, 0, 8 * kForms);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), 0, 0, worst, bad, iters, mode);
    unsigned long long hw[kForms], hb[kForms];
    if (hipMemcpy(hw, worst, 8 * kForms, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 1; }
    (void)hipMemcpy(hb, bad, 8 * kForms, hipMemcpyDeviceToHost);
    printf("%s: %.4g operands per form\n", modes[mode], (double)blocks * threads * iters);
    for (int f = 0; f < kForms; ++f) {
      double rel; memcpy(&rel, &hw[f], 8);
      printf("  %s  max rel diff %.4g = 2^%.2f   class mismatches %llu\n", forms[f], rel, rel > 0 ? log2(rel) : -1074.0, hb[f]);
    }
  }
  hipLaunchKernelGGL(k_special, dim3(1), dim3(1), 0, 0, bad);
  unsigned long long hb = 0; (void)hipMemcpy(&hb, bad, 8, hipMemcpyDeviceToHost);
  printf("special operands (0, -0, inf, -inf, nan, -1, min denormal, max double) through the *_fast forms: %llu mismatches\n", hb);
  return 0;
}
