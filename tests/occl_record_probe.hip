// Test helper (tests/test_hip_occl_records.py): runs disk_reject_record (srh_reject.h) on a list of discs and writes the
// fp32 records with the stored word's V behind them, so that the test can hold U and V to fp64 hits record by record.
//   occl_record_probe IN OUT W H NEAR FAR
// IN:  n x 7 doubles (centre xyz, unit normal xyz, radius);  OUT: n x 13 floats (rec32[0..11], V).
// The camera is the tests' own: eye (0, 0, 4) looking down -z, fovy 45 degrees, D(c, r) = D0 + c Dc + r Dr.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "srh_reject.h"

__global__ void k_probe(const double* in, float* out, int n, srh::PixelBasis B, int W, int H, double near_clip,
                        double far_clip) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double o[3] = {0.0, 0.0, 4.0};
  const double* d = in + 7 * (size_t)i;
  // the fp64 record of prep_record64: unit normal, dist - n.eye, centre, r^2
  const double dist = (d[0] * d[3] + d[1] * d[4]) + d[2] * d[5];
  const double neye = (d[3] * o[0] + d[4] * o[1]) + d[5] * o[2];
  const double R[8] = {d[3], d[4], d[5], dist - neye, d[0], d[1], d[2], d[6] * d[6]};
  float rec[12], v = 0.0f;
  srh::ConicExtent ext;
  srh::disk_reject_record(R, o, B, W, H, near_clip, far_clip, rec, &ext, &v);
  for (int k = 0; k < 12; ++k) out[13 * (size_t)i + k] = rec[k];
  out[13 * (size_t)i + 12] = v;
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char** argv) {
  if (argc != 7) { std::fprintf(stderr, "usage: %s IN OUT W H NEAR FAR\n", argv[0]); return 1; }
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
  const double near_clip = std::atof(argv[5]), far_clip = std::atof(argv[6]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 1;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  const int n = (int)(bytes / (7 * sizeof(double)));
  std::vector<double> in(7 * (size_t)n);
  if (n <= 0 || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 1;
  std::fclose(f);
  const double hh = std::tan(0.5 * 0.78539816339744830962), ww = hh * W / H;
  srh::PixelBasis B;
  const double D0[3] = {-ww, hh, -1.0}, Dc[3] = {2.0 * ww / (W - 1), 0.0, 0.0}, Dr[3] = {0.0, -2.0 * hh / (H - 1), 0.0};
  for (int k = 0; k < 3; ++k) { B.D0[k] = D0[k]; B.Dc[k] = Dc[k]; B.Dr[k] = Dr[k]; }
  double* din = nullptr;
  float* dout = nullptr;
  CHECK(hipMalloc(&din, in.size() * sizeof(double)));
  CHECK(hipMalloc(&dout, 13 * (size_t)n * sizeof(float)));
  CHECK(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe, dim3((n + 63) / 64), dim3(64), 0, 0, din, dout, n, B, W, H, near_clip, far_clip);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> out(13 * (size_t)n);
  CHECK(hipMemcpy(out.data(), dout, out.size() * sizeof(float), hipMemcpyDeviceToHost));
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 1;
  std::fclose(f);
  CHECK(hipFree(din));
  CHECK(hipFree(dout));
  return 0;
}
