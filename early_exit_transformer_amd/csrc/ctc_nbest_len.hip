// The N-best prefix beam search with per-sequence input lengths: ctc_beam.hip compiled with both switches (eec_len.h and
// EEC_CTC_NBEST), as the overload of launch_ctc_beam that takes the frame counts and the N-best outputs.  Its entry point,
// eec_ctc_beam_decode_nbest, is in ctc_nbest.hip.
#define EEC_CTC_LEN 1
#define EEC_CTC_NBEST 1
#include "ctc_beam.hip"
