// The host side of srh_regularizers.h's per-pixel arithmetic (reg_pixel_fwd, reg_finish, reg_pixel_bwd) on one case,
// without a GPU and without a HIP API call: tests/test_regularizers_host_cpu.py builds this, runs it on every seeded and
// edge case and holds what it writes to the fp64 restatement.
//
//   regularizers_host IN OUT WANT_GEO WANT_IMG        (the last two 0 or 1: reg_pixel_bwd's switches)
//
// IN (raw, native endianness): int32 B, H, W; double z_min, z_max, z_scale, unit_normal_scale; float pos[B][H][W][3],
// normal[B][H][W][3], image[B][H][W][3], depth[B][H][W]; float weights[B][7].
// OUT (all double): per view the seven terms before the float cast, the seven after it, the four stats; then per view
// and pixel gp[3], gn[3], g_grey, g_dep as reg_pixel_bwd returns them.
//
// Per view the kRegSums sums are taken over the pixels in row-major order; the "before the cast" terms restate
// reg_finish's seven quotients on the same sums, and the driver fails if casting them does not give reg_finish's floats.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "srh_regularizers.h"

namespace {

template <class T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

bool same_float(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s IN OUT WANT_GEO WANT_IMG\n", argv[0]);
    return 2;
  }
  const bool want_geo = atoi(argv[3]) != 0, want_img = atoi(argv[4]) != 0;
  FILE* in = fopen(argv[1], "rb");
  if (!in) { perror(argv[1]); return 2; }
  int32_t dims[3];
  double par[4];
  if (fread(dims, sizeof(int32_t), 3, in) != 3 || fread(par, sizeof(double), 4, in) != 4) {
    fprintf(stderr, "%s: short header\n", argv[1]);
    return 2;
  }
  const int B = dims[0], H = dims[1], W = dims[2];
  if (B < 1 || H < 2 || W < 2 || (int64_t)H * W > (1 << 24)) {
    fprintf(stderr, "%s: B = %d, H = %d, W = %d\n", argv[1], B, H, W);
    return 2;
  }
  const size_t N = (size_t)H * W, BN = (size_t)B * N;
  std::vector<float> pos, normal, image, depth, weights;
  if (!read_n(in, pos, 3 * BN) || !read_n(in, normal, 3 * BN) || !read_n(in, image, 3 * BN) || !read_n(in, depth, BN) ||
      !read_n(in, weights, (size_t)B * srh::kRegTerms) || fgetc(in) != EOF) {
    fprintf(stderr, "%s: the arrays do not have the header's sizes\n", argv[1]);
    return 2;
  }
  fclose(in);

  srh::RegDev R{};
  R.B = B; R.W = W; R.H = H; R.N = (int)N; R.nblk = (int)((N + srh::kRegBlock - 1) / srh::kRegBlock);
  R.z_min = par[0]; R.z_max = par[1]; R.z_scale = par[2]; R.n_scale = par[3];
  R.pos = pos.data(); R.normal = normal.data(); R.image = image.data(); R.depth = depth.data();

  std::vector<double> head((size_t)B * (2 * srh::kRegTerms + srh::kRegStats)), grads(8 * BN);
  for (int b = 0; b < B; ++b) {
    double p0[3];
    for (int k = 0; k < 3; ++k) p0[k] = pos[3 * (size_t)b * N + k];
    double S[srh::kRegSums] = {};
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) {
        double acc[srh::kRegSums];
        srh::reg_pixel_fwd(R, b, i, j, p0, acc);
        for (int k = 0; k < srh::kRegSums; ++k) S[k] += acc[k];
      }
    float terms[srh::kRegTerms];
    double stats[srh::kRegStats];
    srh::reg_finish(R, S, p0, terms, stats);
    const double n = (double)N;
    const double wide[srh::kRegTerms] = {S[0] / n, S[1] / n, S[2] / (8.0 * n), S[3] / (8.0 * n),
                                         1.0 / (stats[3] + 1.0e-4), S[4] / (8.0 * n), S[5]};
    double* o = head.data() + (size_t)b * (2 * srh::kRegTerms + srh::kRegStats);
    for (int k = 0; k < srh::kRegTerms; ++k) {
      if (!same_float((float)wide[k], terms[k])) {
        fprintf(stderr, "view %d term %d: reg_finish stored %.9g, the driver's quotient casts to %.9g\n", b, k,
                (double)terms[k], (double)(float)wide[k]);
        return 3;
      }
      o[k] = wide[k];
      o[srh::kRegTerms + k] = (double)terms[k];
    }
    for (int k = 0; k < srh::kRegStats; ++k) o[2 * srh::kRegTerms + k] = stats[k];

    double w[srh::kRegTerms];
    for (int k = 0; k < srh::kRegTerms; ++k) w[k] = weights[(size_t)b * srh::kRegTerms + k];
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) {
        double* g = grads.data() + 8 * ((size_t)b * N + (size_t)i * W + j);
        srh::reg_pixel_bwd(R, b, i, j, w, stats, want_geo, want_img, g, g + 3, g[6], g[7]);
      }
  }

  FILE* out = fopen(argv[2], "wb");
  if (!out) { perror(argv[2]); return 2; }
  const bool ok = fwrite(head.data(), sizeof(double), head.size(), out) == head.size() &&
                  fwrite(grads.data(), sizeof(double), grads.size(), out) == grads.size();
  if (fclose(out) != 0 || !ok) {
    fprintf(stderr, "%s: short write\n", argv[2]);
    return 2;
  }
  return 0;
}
