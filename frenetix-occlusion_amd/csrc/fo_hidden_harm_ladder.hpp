// fo_hidden_harm_ladder.hpp -- the value rules of the hidden-traffic harm ladder (fo_scene_hidden_brake_harm_ladder; DESIGN.md §5.10
// "Harm ladder"): when a hit counts as over the harm limit, how the greatest harm of a level and the lowest class that attains it are
// kept and merged, and what the curve holds at the end -- for a level without a hit and for a candidate with a non-finite pose.
// Plain functions of values, compiled for the device by fo_scene.hip (fo_hidden_brake_harm_ladder.hpp calls them per lane and from
// the lanes that write the curve) and for the host by tests/test_hidden_harm_ladder_cpu.py (the style of fo_hidden_impact.hpp).  The
// harm itself is fo_hidden_impact_logistic; the ladder reduction is fo_hidden_ladder_verdict.hpp's.  The definition stands in
// include/fo_hip.h, steps 4 and 6.
#pragma once
#include <stdint.h>
#include "fo_hip.h"

#if defined(__HIPCC__)
#define FO_HIDDEN_HARM_LADDER_HD __host__ __device__ __forceinline__
#else
#define FO_HIDDEN_HARM_LADDER_HD inline
#endif

#define FO_HIDDEN_HARM_LADDER_NO_CLASS 0x7fffffff   // above every class: the lower class wins among equal harms

// the state of a level: the greatest harm so far and the lowest class attaining it
struct fo_hidden_harm_ladder_best_t {
  double harm;         // -1.0 before the first harm that compares: below every harm
  int32_t cls;         // FO_HIDDEN_HARM_LADDER_NO_CLASS before it
};

FO_HIDDEN_HARM_LADDER_HD fo_hidden_harm_ladder_best_t fo_hidden_harm_ladder_none() {
  return fo_hidden_harm_ladder_best_t{-1.0, FO_HIDDEN_HARM_LADDER_NO_CLASS};
}

// step 4: a hit is over the limit when its harm is strictly above it; a NaN never counts as over
FO_HIDDEN_HARM_LADDER_HD bool fo_hidden_harm_ladder_over(bool hit, double ho, double harm_limit) { return hit && ho > harm_limit; }

// step 6, one harm of class c and likewise the state of another lane: the larger harm wins, on equal harm the lower class; a NaN
// never wins
FO_HIDDEN_HARM_LADDER_HD void fo_hidden_harm_ladder_take(fo_hidden_harm_ladder_best_t &s, double ho, int32_t c) {
  if (ho > s.harm || (ho == s.harm && c < s.cls)) {
    s.harm = ho;
    s.cls = c;
  }
}

// step 6, what the curve holds: 0.0 / -1 without a hit (or none whose harm compares), 1.0 / FO_HIDDEN_VERDICT_NOT_FINITE where the
// candidate fails closed
FO_HIDDEN_HARM_LADDER_HD void fo_hidden_harm_ladder_curve(const fo_hidden_harm_ladder_best_t &s, bool finite, double *harm_at,
                                                          int32_t *user_at) {
  const bool none = s.cls == FO_HIDDEN_HARM_LADDER_NO_CLASS;
  *harm_at = !finite ? 1.0 : none ? 0.0 : s.harm;
  *user_at = !finite ? FO_HIDDEN_VERDICT_NOT_FINITE : none ? -1 : s.cls;
}
