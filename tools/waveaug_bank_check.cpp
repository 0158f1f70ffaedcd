// Stand-alone host check of the bank builders of waveform augmentation (eec_rir_bank, eec_noise_bank, csrc/waveaug.hip), meant to be
// built with the host sanitizers; it makes no device call.  Builds banks into exactly sized heap buffers (a write past the end is
// caught), walks each image by the documented layout -- offsets in sequence, no zero head or tail, the peak where the header says, the
// normalisation recomputed in fp64 --, and runs the refusals.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         early_exit_transformer_amd/csrc/waveaug.hip tools/waveaug_bank_check.cpp -o waveaug_bank_check && ./waveaug_bank_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/eec.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static uint32_t g_state = 12345u;
static float noise01() {  // a small generator of its own: values in (-1, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)((int32_t)g_state) * (1.0f / 2147483648.0f);
}

static int walk_rirs(const std::vector<std::vector<float>>& rirs, int normalize, int shift, size_t* bytes_out) {
  const int R = (int)rirs.size();
  std::vector<float> taps;
  std::vector<int32_t> n;
  for (const auto& h : rirs) taps.insert(taps.end(), h.begin(), h.end()), n.push_back((int32_t)h.size());
  const size_t need = eec_rir_bank_bytes(R, taps.data(), n.data(), normalize, shift);
  CHECK(need > 0 && need % 4 == 0);
  std::vector<int32_t>* image = new std::vector<int32_t>(need / 4);  // exactly sized
  CHECK(eec_rir_bank(R, taps.data(), n.data(), normalize, shift, image->data(), need) == 0);
  const int32_t* img = image->data();
  CHECK(img[0] == EEC_RIR_MAGIC && img[1] == R && (size_t)img[2] == need / 4 && img[3] == (normalize | (shift ? 1 : 0) << 8));
  size_t at = 4 + 4 * (size_t)R;
  for (int r = 0; r < R; ++r) {
    const std::vector<float>& h = rirs[r];
    const int32_t* rec = img + 4 + 4 * r;
    const int K = rec[0], d = rec[1], peak = rec[3];
    CHECK(K >= 1 && K <= (int)h.size() && (size_t)rec[2] == at && peak >= 0 && peak < K);
    const float* w = (const float*)(img + rec[2]);
    CHECK(w[0] != 0.0f && w[K - 1] != 0.0f);
    int p = 0;
    double energy = 0.0;
    for (size_t k = 0; k < h.size(); ++k) {
      if (fabsf(h[k]) > fabsf(h[p])) p = (int)k;
      energy += (double)h[k] * (double)h[k];
    }
    const int lo = p - peak;  // the zeros dropped in front
    CHECK(lo >= 0 && lo + K <= (int)h.size() && d == (shift ? peak : -lo));
    const double div = normalize == EEC_RIR_NORM_L2 ? sqrt(energy) : normalize == EEC_RIR_NORM_PEAK ? fabs((double)h[p]) : 1.0;
    double got_energy = 0.0;
    for (size_t k = 0; k < h.size(); ++k) {
      const double want = (double)h[k] / div;
      const double got = (int)k >= lo && (int)k < lo + K ? (double)w[k - lo] : 0.0;
      CHECK(fabs(got - want) <= fabs(want) * ldexp(1.0, -23) + 1e-45);
      got_energy += got * got;
    }
    for (int k = 0; k < K; ++k) CHECK(fabsf(w[k]) <= fabsf(w[peak]));
    for (int k = 0; k < peak; ++k) CHECK(fabsf(w[k]) < fabsf(w[peak]) || fabsf(h[lo + k]) < fabsf(h[p]));
    if (normalize == EEC_RIR_NORM_L2) CHECK(fabs(got_energy - 1.0) < 1e-4);
    if (normalize == EEC_RIR_NORM_PEAK) CHECK(fabsf(w[peak]) == 1.0f);
    at += (size_t)K;
  }
  CHECK(at == need / 4);
  // one byte short: refused, nothing written
  std::vector<int32_t>* small = new std::vector<int32_t>(need / 4, 0x5a5a5a5a);
  CHECK(eec_rir_bank(R, taps.data(), n.data(), normalize, shift, small->data(), need - 1) == EEC_ERR_WORKSPACE);
  for (int32_t v : *small) CHECK(v == 0x5a5a5a5a);
  delete small;
  delete image;
  *bytes_out = need;
  return 0;
}

static int walk_noises(const std::vector<std::vector<float>>& rows, size_t* bytes_out) {
  const int M = (int)rows.size();
  std::vector<float> samples;
  std::vector<int32_t> n;
  for (const auto& x : rows) samples.insert(samples.end(), x.begin(), x.end()), n.push_back((int32_t)x.size());
  const size_t need = eec_noise_bank_bytes(M, samples.data(), n.data());
  CHECK(need > 0 && need % 4 == 0);
  std::vector<int32_t>* image = new std::vector<int32_t>(need / 4);
  CHECK(eec_noise_bank(M, samples.data(), n.data(), image->data(), need) == 0);
  const int32_t* img = image->data();
  CHECK(img[0] == EEC_NOISE_MAGIC && img[1] == M && (size_t)img[2] == need / 4 && img[3] == 0);
  size_t at = 4 + 2 * (size_t)M;
  for (int m = 0; m < M; ++m) {
    CHECK(img[4 + 2 * m] == (int32_t)rows[m].size() && (size_t)img[5 + 2 * m] == at);
    CHECK(memcmp(img + at, rows[m].data(), 4 * rows[m].size()) == 0);
    at += rows[m].size();
  }
  CHECK(at == need / 4);
  std::vector<int32_t>* small = new std::vector<int32_t>(need / 4, 0x5a5a5a5a);
  CHECK(eec_noise_bank(M, samples.data(), n.data(), small->data(), need - 1) == EEC_ERR_WORKSPACE);
  for (int32_t v : *small) CHECK(v == 0x5a5a5a5a);
  delete small;
  delete image;
  *bytes_out = need;
  return 0;
}

int main() {
  std::vector<std::vector<float>> rirs;
  for (int K : {1, 2, 63, 64, 65, 1025, 2500, EEC_REVERB_MAX_TAPS}) {
    std::vector<float> h(K);
    for (int k = 0; k < K; ++k) h[k] = noise01() * expf(-(float)k / (1.0f + K / 8.0f));
    h[K / 3] = 1.5f;
    rirs.push_back(h);
  }
  std::vector<float> padded(40, 0.0f);
  for (int k = 5; k < 33; ++k) padded[k] = 0.2f * noise01();
  padded[11] = -0.9f;
  rirs.push_back(padded);
  rirs.push_back({0.0f, 0.0f, 0.5f, -0.5f, 0.0f});      // a tie: the peak is the first of the two
  rirs.push_back({1e-30f, 1.0f, 1e-30f});               // tiny taps stay (they do not round to zero)
  size_t a[6] = {0}, b = 0, c = 0;
  int at = 0;
  for (int normalize : {EEC_RIR_NORM_NONE, EEC_RIR_NORM_L2, EEC_RIR_NORM_PEAK})
    for (int shift : {0, 1})
      if (walk_rirs(rirs, normalize, shift, &a[at++])) return 1;
  std::vector<std::vector<float>> many(EEC_WAVEAUG_MAX_BANK, std::vector<float>{0.25f});  // the limit of the count
  if (walk_rirs(many, EEC_RIR_NORM_L2, 1, &b)) return 1;

  std::vector<std::vector<float>> rows;
  for (int n : {1, 5, 2999, 3000, 4001, 17}) {
    std::vector<float> x(n);
    for (int i = 0; i < n; ++i) x[i] = n == 17 ? 0.0f : noise01();
    rows.push_back(x);
  }
  if (walk_noises(rows, &c)) return 1;
  if (walk_noises(many, &b)) return 1;

  // the refusals (their messages are the tests' business: the error string's accessor lives in another file of the library)
  int32_t buf[64];
  const float ok[3] = {0.0f, 1.0f, 0.5f}, nan_[3] = {1.0f, NAN, 0.5f}, inf_[3] = {1.0f, INFINITY, 0.5f}, zero[3] = {0.0f, -0.0f, 0.0f};
  const int32_t three[1] = {3}, none[1] = {0}, over[1] = {EEC_REVERB_MAX_TAPS + 1}, huge[1] = {(1 << 30) + 1};
  struct {
    int R;
    const float* taps;
    const int32_t* n;
    int normalize;
  } bad[] = {{0, ok, three, 1},   {-1, ok, three, 1}, {EEC_WAVEAUG_MAX_BANK + 1, ok, three, 1}, {1, nullptr, three, 1}, {1, ok, nullptr, 1},
             {1, ok, none, 1},    {1, ok, over, 1},   {1, ok, three, 3},                        {1, ok, three, -1},     {1, nan_, three, 1},
             {1, inf_, three, 0}, {1, zero, three, 1}, {1, zero, three, 0}};
  for (const auto& k : bad) {
    CHECK(eec_rir_bank_bytes(k.R, k.taps, k.n, k.normalize, 1) == 0);
    CHECK(eec_rir_bank(k.R, k.taps, k.n, k.normalize, 1, buf, sizeof buf) == EEC_ERR_BAD_ARG);
  }
  CHECK(eec_rir_bank(1, ok, three, 1, 1, nullptr, 4096) == EEC_ERR_BAD_ARG);
  struct {
    int M;
    const float* x;
    const int32_t* n;
  } bad_noise[] = {{0, ok, three}, {EEC_WAVEAUG_MAX_BANK + 1, ok, three}, {1, nullptr, three}, {1, ok, nullptr}, {1, ok, none}, {1, ok, huge},
                   {1, nan_, three}, {1, inf_, three}};
  for (const auto& k : bad_noise) {
    CHECK(eec_noise_bank_bytes(k.M, k.x, k.n) == 0);
    CHECK(eec_noise_bank(k.M, k.x, k.n, buf, sizeof buf) == EEC_ERR_BAD_ARG);
  }
  CHECK(eec_noise_bank(1, ok, three, nullptr, 4096) == EEC_ERR_BAD_ARG);
  // the device entries refuse before any device work
  const double g[2] = {0.1, 1.0};
  CHECK(eec_waveaug_draw(1, 0, 0, nullptr, 0, nullptr, 0, 2, 0, 1.0, 1.0, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_waveaug_draw(1, 0, 0, nullptr, (1ull << 32) + 1, nullptr, 0, 2, 0, 1.0, 1.0, buf, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_reverb(nullptr, nullptr, nullptr, 1, 10, nullptr, nullptr, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_noise_energy(nullptr, nullptr, nullptr, 1, (1 << 30) + 1, nullptr, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_noise_mix(nullptr, nullptr, nullptr, 1, 10, nullptr, g, 65, nullptr, nullptr, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_noise_mix(nullptr, nullptr, nullptr, 0, 10, nullptr, g, 2, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(eec_waveaug_partials_bytes(3, 1025) == 3 * 2 * 2 * sizeof(double));
  printf("waveaug_bank_check: RIR images of %zu .. %zu bytes, noise images of %zu and %zu bytes walked, refusals ok\n", a[0], a[5], c, b);
  return 0;
}
