// Stand-alone host check of the spectral image of reverberation by FFT (eec_rir_spectra, csrc/reverb_fft.hip), meant to be built with
// the host sanitizers; it makes no device call.  Builds tap images and their spectral images into exactly sized heap buffers (a write
// past the end is caught), walks each spectral image by the documented layout -- header, records and offsets in sequence, the twiddle
// table, every partition's spectrum against a naive fp64 DFT of the stored taps --, and runs the refusals.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined early_exit_transformer_amd/csrc/waveaug.hip \
//         early_exit_transformer_amd/csrc/reverb_fft.hip tools/rir_spectra_check.cpp -o rir_spectra_check && ./rir_spectra_check
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

static const int S = EEC_REVERB_FFT_BLOCK, N = 2 * EEC_REVERB_FFT_BLOCK;

static uint32_t g_state = 54321u;
static float noise01() {  // a small generator of its own: values in (-1, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)((int32_t)g_state) * (1.0f / 2147483648.0f);
}

// cos and sin of 2 pi t / N for an integer t, the angle reduced exactly
static void unit(long long t, double* c, double* s) {
  const double a = 6.283185307179586476925286766559 * (double)(t % N) / N;
  *c = cos(a), *s = sin(a);
}

static int walk(const std::vector<std::vector<float>>& rirs, int normalize, int shift, int every, size_t* bytes_out, double* worst_out) {
  const int R = (int)rirs.size();
  std::vector<float> taps;
  std::vector<int32_t> n;
  for (const auto& h : rirs) taps.insert(taps.end(), h.begin(), h.end()), n.push_back((int32_t)h.size());
  const size_t bank_bytes = eec_rir_bank_bytes(R, taps.data(), n.data(), normalize, shift);
  CHECK(bank_bytes > 0);
  std::vector<int32_t>* bank = new std::vector<int32_t>(bank_bytes / 4);
  CHECK(eec_rir_bank(R, taps.data(), n.data(), normalize, shift, bank->data(), bank_bytes) == 0);
  const size_t need = eec_rir_spectra_bytes(bank->data());
  CHECK(need > 0 && need % 16 == 0);
  std::vector<int32_t>* image = new std::vector<int32_t>(need / 4);  // exactly sized
  CHECK(eec_rir_spectra(bank->data(), image->data(), need) == 0);
  const int32_t* img = image->data();
  CHECK(img[0] == EEC_RIR_SPECTRA_MAGIC && img[1] == R && (size_t)img[2] == need / 4 && img[3] == S);
  CHECK(img[5] == 0 && img[6] == 0 && img[7] == 0);
  size_t at = ((size_t)8 + 2 * (size_t)R + 3) & ~(size_t)3;
  CHECK((size_t)img[4] == at);
  const float* tw = (const float*)(img + at);
  for (int u = 0; u < N / 2; ++u) {
    double c, s;
    unit(u, &c, &s);
    CHECK(fabs((double)tw[2 * u] - c) <= ldexp(1.0, -24) && fabs((double)tw[2 * u + 1] + s) <= ldexp(1.0, -24));
  }
  CHECK(tw[0] == 1.0f && tw[1] == 0.0f && tw[N / 2] == 0.0f && tw[N / 2 + 1] == -1.0f);  // exact on the axes
  at += N;
  double worst = 0.0;
  for (int r = 0; r < R; ++r) {
    const int32_t* rec = bank->data() + 4 + 4 * r;
    const int K = rec[0], P = (K + S - 1) / S;
    const float* h = (const float*)(bank->data() + rec[2]);
    CHECK(img[8 + 2 * r] == P && (size_t)img[9 + 2 * r] == at && at % 4 == 0);
    for (int p = 0; p < P; ++p, at += N) {
      const float* H = (const float*)(img + at);
      const int taps_here = K - p * S < S ? K - p * S : S;
      double l1 = 0.0;
      for (int k = 0; k < taps_here; ++k) l1 += fabs((double)h[p * S + k]);
      std::vector<int> bins = {0, N / 2};
      for (int k = 1; k < N / 2; k += every) bins.push_back(k);
      for (int k : bins) {
        double re = 0.0, im = 0.0;
        for (int t = 0; t < taps_here; ++t) {
          double c, s;
          unit((long long)t * k, &c, &s);
          re += (double)h[p * S + t] * c, im -= (double)h[p * S + t] * s;
        }
        const double got_re = k == 0 ? H[0] : k == N / 2 ? H[1] : H[2 * k], got_im = k == 0 || k == N / 2 ? 0.0 : H[2 * k + 1];
        // one rounding to fp32 of a value of at most ||h||_1, and the naive sum's own fp64 error
        const double allow = ldexp(l1, -24) + 1e-12 * l1;
        CHECK(fabs(got_re - re) <= allow && fabs(got_im - im) <= allow);
        if (l1 > 0.0) worst = fmax(worst, fmax(fabs(got_re - re), fabs(got_im - im)) / ldexp(l1, -24));
      }
    }
  }
  CHECK(at == need / 4);
  // one byte short: refused, nothing written
  std::vector<int32_t>* small = new std::vector<int32_t>(need / 4, 0x5a5a5a5a);
  CHECK(eec_rir_spectra(bank->data(), small->data(), need - 1) == EEC_ERR_WORKSPACE);
  for (int32_t v : *small) CHECK(v == 0x5a5a5a5a);
  delete small;
  delete image;
  delete bank;
  *bytes_out = need, *worst_out = worst;
  return 0;
}

int main() {
  std::vector<std::vector<float>> rirs;
  for (int K : {1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, EEC_REVERB_MAX_TAPS}) {
    std::vector<float> h(K);
    for (int k = 0; k < K; ++k) h[k] = noise01() * expf(-(float)k / (1.0f + K / 8.0f));
    h[K / 3] = 1.5f;
    rirs.push_back(h);
  }
  std::vector<float> padded(S + 40, 0.0f);
  for (int k = 5; k < S + 33; ++k) padded[k] = 0.2f * noise01();
  padded[11] = -0.9f;
  rirs.push_back(padded);
  size_t a[4] = {0}, b = 0;
  double worst[4] = {0}, w = 0.0;
  int at = 0;
  for (int normalize : {EEC_RIR_NORM_NONE, EEC_RIR_NORM_L2})
    for (int shift : {0, 1}) {
      if (walk(rirs, normalize, shift, 97, &a[at], &worst[at])) return 1;
      ++at;
    }
  std::vector<std::vector<float>> many(EEC_WAVEAUG_MAX_BANK, std::vector<float>{0.25f});  // the limit of the count
  if (walk(many, EEC_RIR_NORM_L2, 1, 1000, &b, &w)) return 1;

  // the refusals (their messages are the tests' business: the error string's accessor lives in another file of the library)
  int32_t buf[64], bank[16] = {0};
  const float one[1] = {1.0f};
  const int32_t n1[1] = {1};
  CHECK(eec_rir_bank(1, one, n1, EEC_RIR_NORM_NONE, 1, bank, sizeof bank) == 0);
  CHECK(eec_rir_spectra_bytes(bank) == 4 * (size_t)(12 + 2 * N));
  CHECK(eec_rir_spectra_bytes(nullptr) == 0 && eec_rir_spectra(nullptr, buf, sizeof buf) == EEC_ERR_BAD_ARG);
  CHECK(eec_rir_spectra(bank, nullptr, 1 << 20) == EEC_ERR_BAD_ARG);
  CHECK(eec_rir_spectra(bank, buf, sizeof buf) == EEC_ERR_WORKSPACE);
  int32_t broken[16];
  memcpy(broken, bank, sizeof bank), broken[0] ^= 1;
  CHECK(eec_rir_spectra_bytes(broken) == 0);  // not a tap image
  memcpy(broken, bank, sizeof bank), broken[1] = EEC_WAVEAUG_MAX_BANK + 1;
  CHECK(eec_rir_spectra_bytes(broken) == 0);  // a count outside its range
  memcpy(broken, bank, sizeof bank), broken[4] = EEC_REVERB_MAX_TAPS + 1;
  CHECK(eec_rir_spectra_bytes(broken) == 0);  // a record outside its range
  memcpy(broken, bank, sizeof bank), broken[6] = broken[2];
  CHECK(eec_rir_spectra_bytes(broken) == 0);  // taps past the image
  // the device entry refuses before any device work
  float x[4] = {0}, y[4] = {0};
  CHECK(eec_reverb_fft_workspace_bytes(3, 2 * S + 1) == (size_t)3 * (3 + EEC_REVERB_MAX_TAPS / S - 1) * N * 4);
  CHECK(eec_reverb_fft_workspace_bytes(-1, 4) == 0 && eec_reverb_fft_workspace_bytes(1, (1 << 30) + 1) == 0);
  CHECK(eec_reverb_fft(nullptr, nullptr, nullptr, 1, 4, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_reverb_fft(x, nullptr, buf, 1, 4, nullptr, nullptr, x, nullptr, nullptr, 0, nullptr) == EEC_ERR_BAD_ARG);  // out == wave
  CHECK(eec_reverb_fft(x, nullptr, buf, -1, 4, nullptr, nullptr, y, nullptr, nullptr, 0, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_reverb_fft(x, nullptr, buf, 1, 4, bank, bank, y, nullptr, nullptr, 0, nullptr) == EEC_ERR_WORKSPACE);
  CHECK(eec_reverb_fft(x, nullptr, buf, 1, 4, bank, bank, y, nullptr, buf, 16, nullptr) == EEC_ERR_WORKSPACE);
  CHECK(eec_reverb_fft(x, nullptr, buf, 0, 4, nullptr, nullptr, y, nullptr, nullptr, 0, nullptr) == 0);
  printf("rir_spectra_check: spectral images of %zu .. %zu bytes and of %zu bytes walked, worst bin at %.3f of 2^-24 ||h_p||_1, refusals ok\n", a[0],
         a[3], b, fmax(fmax(worst[0], worst[1]), fmax(worst[2], worst[3])));
  return 0;
}
