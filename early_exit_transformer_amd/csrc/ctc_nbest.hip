// N-best from the CTC prefix beam search (eec_ctc_beam_decode_nbest): ctc_beam.hip compiled once more with EEC_CTC_NBEST -- the
// same search, kernel body, candidate ids and tie rules; only the end differs, which ranks the final beam and traces up to
// `nbest` prefixes back instead of one.  This file holds the form without input lengths and the entry point; ctc_nbest_len.hip
// compiles the form with lengths.
#define EEC_CTC_NBEST 1
#include "ctc_beam.hip"

namespace eec {
// ctc_nbest_len.hip
hipError_t launch_ctc_beam(const float* logp, const int* em_len, int n_seq, int Tq, int V, int blank, int beam, float blank_skip_threshold,
                           int skip_drops, int* backptr, int* tokens, int* counts, float* scores, hipStream_t st, int nbest, int* n_hyp);
}  // namespace eec

extern "C" int eec_ctc_beam_decode_nbest(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                                         float blank_skip_threshold, int skip_drops_frame, int nbest, void* workspace, int32_t* tokens,
                                         int32_t* counts, float* scores, int32_t* n_hyp, void* stream) {
  using eech::fail;
  if (!logp || !workspace || !tokens || !counts || !scores || !n_hyp) return fail(EEC_ERR_BAD_ARG, "eec_ctc_beam_decode_nbest: null argument");
  if (n_seq <= 0 || Tq <= 0) return fail(EEC_ERR_BAD_ARG, "eec_ctc_beam_decode_nbest: n_seq and Tq must be positive");
  if (V < 1 || V > 256 || beam_size < 1 || beam_size > eec::kCbMaxBeam || blank < 0 || blank >= V)
    return fail(EEC_ERR_UNSUPPORTED,
                "eec_ctc_beam_decode_nbest: needs 1 <= V <= 256, 1 <= beam_size <= " + std::to_string(eec::kCbMaxBeam) + ", blank in [0, V)");
  if (nbest < 1 || nbest > beam_size) return fail(EEC_ERR_BAD_ARG, "eec_ctc_beam_decode_nbest: needs 1 <= nbest <= beam_size");
  hipStream_t st = (hipStream_t)stream;
  if (em_len)
    EEC_HIP(eec::launch_ctc_beam(logp, em_len, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens,
                                 counts, scores, st, nbest, n_hyp));
  else
    EEC_HIP(eec::launch_ctc_beam(logp, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens, counts,
                                 scores, st, nbest, n_hyp));
  return 0;
}
