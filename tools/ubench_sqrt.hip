// Bit-identity check (MI355X): sqrt() of an fp64 operand as hipcc expands it, against the same Newton sequence without
// its range guards (sqrt_bounded, srh_device.h), over the operands the host admits for it (camera_to_frame: 1e-100 <= |D|
// <= 1e100, so 1e-200 <= |D|^2 <= 1e200).  Prints the number of mismatching results; anything but 0 means the form must go.
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -I surf_renderer_amd/csrc -I include tools/ubench_sqrt.hip -o build/ubench/sqrtcheck && build/ubench/sqrtcheck
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "srh.h"
#include "srh_device.h"
__device__ uint64_t rng(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
__global__ void k(unsigned long long* bad, int iters, int mode) {
  uint64_t s = 0x9E3779B97F4A7C15ull * (blockIdx.x * blockDim.x + threadIdx.x + 1);
  unsigned long long nb = 0;
  for (int it = 0; it < iters; ++it) {
    double x;
    if (mode == 0) {          // sums of three squares of camera-like magnitudes
      double v[3];
      for (int i = 0; i < 3; ++i) v[i] = ((double)(int64_t)rng(s)) * (1.0 / 9.2e18) * 3.0;
      x = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
      if (!(x >= 1e-200)) x = 1.0;
    } else if (mode == 1) {   // every mantissa, exponents -664 .. 664 (1e-200 .. 1e200)
      const double m = 1.0 + (double)(rng(s) >> 12) * 0x1p-52;
      x = ldexp(m, (int)(rng(s) % 1329) - 664);
    } else {                  // neighbours of perfect squares and of powers of two: where the last Newton step decides
      const double b = ldexp(1.0 + (double)(rng(s) >> 38) * 0x1p-26, (int)(rng(s) % 600) - 300);
      const long long sq = __double_as_longlong(b * b) + (long long)(rng(s) % 5) - 2;
      x = __longlong_as_double(sq);
    }
    const double a = sqrt(x), b = srh::sqrt_bounded(x);
    nb += (__double_as_longlong(a) != __double_as_longlong(b));
  }
  if (nb) atomicAdd(bad, nb);
}
int main() {
  unsigned long long* bad;
  if (hipMalloc(&bad, 8) != hipSuccess) { printf("no device\n"); return 2; }
  unsigned long long total = 0;
  for (int mode = 0; mode < 3; ++mode) {
    (void)hipMemset(bad, 0, 8);
    hipLaunchKernelGGL(k, dim3(4096), dim3(256), 0, 0, bad, 800, mode);
    unsigned long long h = ~0ull;
    if (hipMemcpy(&h, bad, 8, hipMemcpyDeviceToHost) != hipSuccess) { printf("mode %d: the run failed\n", mode); return 2; }
    printf("mode %d: %llu mismatches in %.3g square roots\n", mode, h, 4096.0 * 256 * 800);
    total += h;
  }
  return total ? 1 : 0;
}
