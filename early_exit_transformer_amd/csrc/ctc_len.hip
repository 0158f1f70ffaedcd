// The CTC loss, its gradient, the greedy decoder and the prefix beam search with per-sequence input lengths (eec_ctc_loss_len,
// eec_ctc_loss_forward_len / _backward_len, eec_greedy_ctc_len, eec_ctc_beam_decode_len): the kernels and launchers of ctc.hip,
// pack.hip and ctc_beam.hip compiled a second time with the length switch of eec_len.h, as overloads that take the frame counts.
#define EEC_CTC_LEN 1
#include "ctc.hip"
#include "ctc_beam.hip"
#include "pack.hip"
