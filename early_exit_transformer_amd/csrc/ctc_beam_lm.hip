// The CTC prefix beam search under shallow fusion with a token-level n-gram model (eec_ctc_beam_decode_lm,
// eec_ctc_beam_decode_nbest_lm): the kernel and launcher of ctc_beam.hip compiled a third time with the model switch, under names of
// their own.
#define EEC_CTC_LM 1
#include "ctc_beam.hip"
