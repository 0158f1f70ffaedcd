// Stand-alone host check of the resampling plan builder (eec_resample_plan, csrc/resample.hip), meant to be built with the host
// sanitizers; it makes no device call.  Builds plans into exactly sized heap buffers (a write past the end is caught), walks each image
// by the documented layout -- offsets in sequence, every stored range inside [0, K), no zero head or tail, the weights of a phase
// summing to about one (a constant comes out as that constant) --, recomputes every weight from the formula in fp64, and runs the
// refusals.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         early_exit_transformer_amd/csrc/resample.hip tools/resample_plan_check.cpp -o resample_plan_check && ./resample_plan_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <numeric>
#include <vector>

#include "../include/eec.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static int walk(const std::vector<int32_t>& orig, const std::vector<int32_t>& new_, int lpw, double rolloff, size_t* bytes_out) {
  const int R = (int)orig.size();
  const size_t need = eec_resample_plan_bytes(R, orig.data(), new_.data(), lpw, rolloff);
  CHECK(need > 0 && need % 4 == 0);
  std::vector<int32_t>* image = new std::vector<int32_t>(need / 4);  // exactly sized
  CHECK(eec_resample_plan(R, orig.data(), new_.data(), lpw, rolloff, image->data(), need) == 0);
  const int32_t* img = image->data();
  CHECK(img[0] == EEC_RESAMPLE_MAGIC && img[1] == R && (size_t)img[2] == need / 4 && img[3] == lpw);
  size_t at = 4 + 8 * (size_t)R;
  const double pi = 3.14159265358979323846;
  for (int r = 0; r < R; ++r) {
    const int32_t* rec = img + 4 + 8 * r;
    const int g = std::gcd(orig[r], new_[r]);
    const int o = rec[0], n = rec[1], width = rec[2], K = rec[3];
    CHECK(o == orig[r] / g && n == new_[r] / g);
    const double base = (double)(o < n ? o : n) * rolloff;
    CHECK(width == (int)ceil((double)(lpw * o) / base) && K == 2 * width + o);
    CHECK((size_t)rec[4] == at && (size_t)rec[5] == at + 3 * (size_t)n);
    const int32_t* ph = img + rec[4];
    const float* w = (const float*)(img + rec[5]);
    long long total = 0;
    int most = 0;
    double gain = 0.0;
    for (int j = 0; j < n; ++j) {
      const int first = ph[3 * j], count = ph[3 * j + 1], off = ph[3 * j + 2];
      CHECK(off == total && first >= 0 && count > 0 && first + count <= K);
      CHECK(w[off] != 0.0f && w[off + count - 1] != 0.0f);
      for (int k = 0; k < K; ++k) {
        double t = ((double)(-j) / n + (double)(k - width) / o) * base;
        t = t < -lpw ? -lpw : t > lpw ? lpw : t;
        const double c = cos(t * pi / lpw / 2.0), s = t == 0.0 ? 1.0 : sin(t * pi) / (t * pi);
        const double want = s * c * c * base / o;
        const double got = k >= first && k < first + count ? (double)w[off + k - first] : 0.0;
        CHECK(fabs(got - want) <= ldexp(base / o, -23));
        gain += got;
      }
      total += count;
      if (count > most) most = count;
    }
    CHECK(rec[6] == total && rec[7] == most);
    CHECK(fabs(gain / n - 1.0) < 2e-2);  // a constant input comes out as (nearly) the same constant
    at = (size_t)rec[5] + (size_t)total;
  }
  CHECK(at == need / 4);
  // one byte short: refused, nothing written
  std::vector<int32_t>* small = new std::vector<int32_t>(need / 4, 0x5a5a5a5a);
  CHECK(eec_resample_plan(R, orig.data(), new_.data(), lpw, rolloff, small->data(), need - 1) == EEC_ERR_WORKSPACE);
  for (int32_t v : *small) CHECK(v == 0x5a5a5a5a);
  delete small;
  delete image;
  *bytes_out = need;
  return 0;
}

int main() {
  size_t a = 0, b = 0, c = 0, d = 0;
  if (walk({14400, 16000, 17600}, {16000, 16000, 16000}, 6, 0.99, &a)) return 1;           // the speed factors 0.9 / 1.0 / 1.1 at 16 kHz
  if (walk({44100, 48000, 8000, 22050, 3, 1, 441, 16000}, {16000, 16000, 16000, 16000, 1, 2, 320, 24000}, 6, 0.99, &b)) return 1;  // eight ratios
  if (walk({640, 639, 1}, {1, 640, 640}, 6, 1.0, &c)) return 1;                             // the limits of the ratio
  if (walk({3, 2}, {2, 3}, 64, 0.5, &d)) return 1;                                          // the widest filter

  // the refusals (their messages are the tests' business: the error string's accessor lives in another file of the library)
  const int32_t nine[9] = {9, 9, 9, 9, 9, 9, 9, 9, 9}, ten[9] = {10, 10, 10, 10, 10, 10, 10, 10, 10}, big[1] = {641}, zero[1] = {0}, neg[1] = {-3};
  int32_t buf[1024];
  struct {
    int R;
    const int32_t *o, *n;
    int lpw;
    double rolloff;
  } bad[] = {{9, nine, ten, 6, 0.99},    {0, nine, ten, 6, 0.99},   {-1, nine, ten, 6, 0.99},  {1, big, ten, 6, 0.99},    {1, ten, big, 6, 0.99},
             {1, zero, ten, 6, 0.99},    {1, nine, neg, 6, 0.99},   {1, nine, ten, 0, 0.99},   {1, nine, ten, 65, 0.99},  {1, nine, ten, 6, 0.0},
             {1, nine, ten, 6, 1.5},     {1, nine, ten, 6, NAN},    {1, nullptr, ten, 6, 0.99}, {1, nine, nullptr, 6, 0.99}};
  for (const auto& k : bad) {
    CHECK(eec_resample_plan_bytes(k.R, k.o, k.n, k.lpw, k.rolloff) == 0);
    CHECK(eec_resample_plan(k.R, k.o, k.n, k.lpw, k.rolloff, buf, sizeof buf) == EEC_ERR_BAD_ARG);
  }
  CHECK(eec_resample_plan(1, nine, ten, 6, 0.99, nullptr, 4096) == EEC_ERR_BAD_ARG);
  // the device entries refuse before any device work
  CHECK(eec_resample(nullptr, nullptr, nullptr, 1, 10, nullptr, nullptr, 12, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_speed_draw(nullptr, 1, 10, 0, 0, nullptr, nullptr, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_resample_lengths(nullptr, nullptr, 1, (1 << 30) + 1, nullptr, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_resample(nullptr, nullptr, nullptr, 0, 10, nullptr, nullptr, 12, nullptr, nullptr) == 0);
  printf("resample_plan_check: images of %zu, %zu, %zu and %zu bytes walked, refusals ok\n", a, b, c, d);
  return 0;
}
