// The CTC prefix beam search under contextual biasing (eec_ctc_beam_decode_ctx, eec_ctc_beam_decode_nbest_ctx): the kernel and
// launcher of ctc_beam.hip compiled a second time with the context switch, under names of their own.
#define EEC_CTC_CTX 1
#include "ctc_beam.hip"
