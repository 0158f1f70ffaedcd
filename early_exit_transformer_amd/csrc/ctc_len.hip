// The CTC loss and its gradient with per-utterance input lengths (eec_ctc_loss_len, eec_ctc_loss_forward_len / _backward_len): the
// kernels and launchers of ctc.hip compiled a second time with the length switch of eec_len.h, as overloads that take the frame counts.
#define EEC_CTC_LEN 1
#include "ctc.hip"
