// Per-sequence input lengths as a compile-time switch.  ctc.hip, ctc_beam.hip and the greedy decoder of pack.hip assume the
// reference's convention, T' frames for every sequence; ctc_len.hip compiles the three a second time with EEC_CTC_LEN defined, and
// then every kernel and launcher among them takes one more argument, a device array of frame counts (`input_len` [B], shared by
// the E exits of an utterance; `em_len` [n_seq] for the decoders), and walks clamp(count, 0, T') frames instead of T'.  The extra
// parameter makes the second set overloads of the first: both live in one library.  Without the macro the parameter, the clamp
// and every branch on kLen are gone before code generation, so the entries without lengths keep their device code to the byte
// (tools/isa_diff.sh).  Strides, workspaces and output layouts stay on T' in both.
#pragma once

namespace eec {

#ifdef EEC_CTC_LEN
constexpr bool kLen = true;
#define EEC_LEN_PARAM(decl) decl,              // in a parameter list: `decl,`; in an argument list: `name,`
#define EEC_LEN_FRAMES(len, i, Tq) min(max((len)[i], 0), (Tq))
#else
constexpr bool kLen = false;
#define EEC_LEN_PARAM(decl)
#define EEC_LEN_FRAMES(len, i, Tq) (Tq)
#endif

}  // namespace eec
