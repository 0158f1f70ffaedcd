// Stand-alone host check of log_add (eec_ctc_log_add_host, csrc/ctc_lexbeam.hip: the function the log-add beam search folds its
// merges with), meant to be built with the host sanitizers; it makes no device call.  Sweeps d = lo - hi over [cutoff - 1, 0]
// (argv[1]: points, default 2 000 000) at three magnitudes of hi and both argument orders, and checks what include/eec.h promises
// of every value: symmetry bit for bit, hi alone at and below the cutoff, hi + 0.693147182 at a == b, a result within the written
// bound (plus the rounding of the final addition) of the float64 log-sum, and a non-decreasing result as lo rises.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         early_exit_transformer_amd/csrc/ctc_lexbeam.hip early_exit_transformer_amd/csrc/ctc_lexbeam_wide.hip \
//         tools/logadd_check.cpp -o logadd_check
//   ./logadd_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/eec.h"

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      return 1;                                                             \
    }                                                                       \
  } while (0)

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

int main(int argc, char** argv) {
  const int points = argc > 1 ? atoi(argv[1]) : 2000000;
  CHECK(points >= 1000);
  const float cutoff = -17.34375f;
  const double bound = 1.2e-7;  // include/eec.h
  double worst = 0.0;
  const float his[3] = {0.0f, -3.0f, -250.0f};
  for (int h = 0; h < 3; ++h) {
    const float hi = his[h];
    const double ulp = hi == 0.0f ? 0.0 : ldexp(1.0, ilogbf(hi) - 23);  // of the final addition's result (it stays in hi's binade or the next)
    float last = -INFINITY;
    for (int k = 0; k <= points; ++k) {
      const float lo = hi + (float)((double)(cutoff - 1.0f) * (double)(points - k) / (double)points);
      const float d = lo - hi;
      const float r = eec_ctc_log_add_host(hi, lo);
      CHECK(bits(r) == bits(eec_ctc_log_add_host(lo, hi)));
      if (!(d > cutoff)) {
        CHECK(bits(r) == bits(hi));
      } else {
        const double want = (double)hi + log1p(exp((double)lo - (double)hi));
        const double err = fabs((double)r - want);
        if (hi == 0.0f && err > worst) worst = err;
        CHECK(err <= bound + ulp);
      }
      CHECK(r >= last || h > 0);  // at hi = 0 nothing is rounded after the function: it must not decrease
      last = r;
    }
    CHECK(bits(eec_ctc_log_add_host(hi, hi)) == bits(hi + 0.693147182f));
  }
  CHECK(worst <= bound);
  printf("logadd_check: %d points x 3 magnitudes x 2 orders, worst |log_add(0, d) - fp64| = %.3e (bound %.1e)\n", points + 1, worst, bound);
  return 0;
}
