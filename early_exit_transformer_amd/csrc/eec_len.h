// Per-utterance input lengths of the CTC loss as a compile-time switch.  ctc.hip assumes the reference's convention, T' frames for
// every utterance; ctc_len.hip compiles it a second time with EEC_CTC_LEN defined, and then every kernel and launcher in it takes one
// more argument, a device array of frame counts (`input_len` [B], shared by the E exits of an utterance), and walks clamp(count, 0,
// T') frames instead of T'.  The extra parameter makes the second set overloads of the first: both live in one library.  Without the
// macro the parameter, the clamp and every branch on kLen are gone before code generation.  Strides, workspaces and output layouts
// stay on T' in both.  (The decoders take a nullable runtime pointer instead: ctc_frames, eec_kernels.h.  The loss keeps the switch
// because its 8-states-per-lane loss kernel measured 0.5 % slower with the pointer than this compilation of it: DESIGN.md.)
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
