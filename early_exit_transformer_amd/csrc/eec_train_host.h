// Host helpers the two training steps share (train.hip: the encoder's, decoder_train.hip: the AED decoder's): what a run
// launches with, and the Linear / LayerNorm launches that are the same in both.  linear_bwd_weight is NOT here: the two
// files choose different split counts and the encoder's runs on its side stream, so one copy would change grids and the
// order of the partial sums.
#pragma once
#include "eec_host.h"
#include "eec_train.h"

namespace eech {

struct TrainRun : Deferred {
  hipStream_t st;
  int np;    // GEMM passes: 1 (bf16) or 3 (bf16x3)
  Bump scr;  // main-stream scratch
  TrainRun(bool dry_, hipStream_t st_, int np_) : st(st_), np(np_) { dry = dry_; }
};

// y[M][N] = x[M][K] . W[N][K]^T + bias
inline void linear_fwd(TrainRun& r, const float* x, const float* W, const float* bias, float* y, long M, int N, int K) {
  eect::GemmArgs g = eect::gemm_args(x, K, 1, W, K, 1, y, N, (int)M, N, K);
  g.bias = bias;
  RUN(eect::launch_gemm(g, r.np, r.st));
}
// dx[M][K] (+)= dy[M][N] . W[N][K]
inline void linear_bwd_data(TrainRun& r, const float* dy, const float* W, float* dx, long M, int N, int K, bool accumulate = false) {
  eect::GemmArgs g = eect::gemm_args(dy, N, 1, W, 1, K, dx, K, (int)M, K, N);
  g.accumulate = accumulate;
  RUN(eect::launch_gemm(g, r.np, r.st));
}
// dx = (add_res ? dx : 0) + LN'(dln) in place; dg / db from the per-block partials
inline void ln_bwd(TrainRun& r, const float* dln, const float* x, const float* g, const float* mean, const float* rstd, float* dx, bool add_res,
                   float* dg, float* db, long M, int D) {
  const size_t mark = r.scr.off;
  const int nb = eect::ln_bwd_blocks((int)M);
  float* part = r.scr.f((size_t)nb * 2 * D);
  RUN(eect::launch_ln_bwd(dln, x, g, mean, rstd, add_res ? dx : nullptr, dx, part, (int)M, D, r.st));
  RUN(eect::launch_reduce_leading2(part, nb, D, dg, db, r.st));
  r.scr.reset(mark);
}

}  // namespace eech
