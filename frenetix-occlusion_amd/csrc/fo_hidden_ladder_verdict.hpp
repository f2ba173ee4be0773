// fo_hidden_ladder_verdict.hpp -- what the hidden-traffic ladder verdict (fo_scene_hidden_brake_ladder_verdict; DESIGN.md §5.10
// "Ladder verdict") decides per trajectory once the walk has, per brake start, the first level clear of every class and the classes
// that block the level below it: the level the worst brake start needs, that start, its blocking classes, the deceleration, the
// fail-closed row of a candidate with a non-finite pose, and what of that goes into the cost row and the safety flag.  Plain
// functions of values, compiled for the device by fo_scene.hip (fo_hidden_brake_ladder_verdict.hpp calls them per (m, b) group and
// from lane 0 of each trajectory) and for the host by tests/test_hidden_brake_ladder_verdict_cpu.py (the style of
// fo_hidden_verdict.hpp).  The definition stands in include/fo_hip.h, steps 1 - 7.
//
// Steps 1 - 3 are ONE maximum: a brake start's rank, the start and its blocking mask travel as one int32 key,
//   rank << 16 | (255 - b) << 8 | blocking      (rank <= L <= 64, b <= 253, blocking < 2^8: C <= 8)
// so that the largest key holds the largest rank, among equal ranks the smallest b, and that start's mask.  A start without a
// manoeuvre has no key (FO_HIDDEN_LADDER_NO_KEY, below every key).
#pragma once
#include <stdint.h>
#include "fo_hip.h"

#if defined(__HIPCC__)
#define FO_HIDDEN_LADDER_HD __host__ __device__ __forceinline__
#else
#define FO_HIDDEN_LADDER_HD inline
#endif

#define FO_HIDDEN_LADDER_NO_KEY (-1)

struct fo_hidden_ladder_verdict_t {
  int32_t need;        // the level the worst of the brake starts needs: 0 .. L-1, L = no level of the ladder, -1 = nothing asked
  int32_t at;          // the first brake start that needs it, -1 = nothing asked
  int32_t blocking;    // bit c: class c keeps that start from the next gentler level
  int32_t user;        // the lowest such class, -1 = none, FO_HIDDEN_VERDICT_NOT_FINITE = fails closed
  double decel;        // levels[need], +inf for need = L, 0.0 for need = -1
};

// step 1: required / required_all of fo_scene_hidden_brake_ladder_users at a brake start with a manoeuvre, as a rank
FO_HIDDEN_LADDER_HD int32_t fo_hidden_ladder_rank(int32_t required, int L) { return required >= 0 ? required : L; }

// the key of brake start b (b < min(B, Lm))
FO_HIDDEN_LADDER_HD int32_t fo_hidden_ladder_key(int32_t rank, int b, int32_t blocking) {
  return (int32_t)((uint32_t)rank << 16 | (uint32_t)(255 - b) << 8 | ((uint32_t)blocking & 0xffu));
}

// the reduction over the brake starts of a trajectory, for the keys and for the per-class ranks (-1 = none yet)
FO_HIDDEN_LADDER_HD int32_t fo_hidden_ladder_max(int32_t a, int32_t b) { return a > b ? a : b; }

// step 5
FO_HIDDEN_LADDER_HD double fo_hidden_ladder_decel(int32_t need, int L, double level_of_need) {
  return need < 0 ? 0.0 : need >= L ? (double)__builtin_inf() : level_of_need;
}

// steps 1 - 3 and 6 from the largest key of the trajectory; decel is the caller's (it holds the levels): step 5 where finite
FO_HIDDEN_LADDER_HD fo_hidden_ladder_verdict_t fo_hidden_ladder_verdict_of(int32_t key, int L, bool finite) {
  fo_hidden_ladder_verdict_t r{-1, -1, 0, -1, 0.0};
  if (key >= 0) {
    r.need = key >> 16;
    r.at = 255 - (key >> 8 & 0xff);
    r.blocking = key & 0xff;
    r.user = __builtin_ffs(r.blocking) - 1;   // (no bit: -1)
  }
  if (!finite) {
    r.need = L;
    r.at = 0;
    r.blocking = 0;
    r.user = FO_HIDDEN_VERDICT_NOT_FINITE;
  }
  return r;
}

// step 7: the two reserved columns always; the flag and FO_C_SAFE only ever lose safety; no other column is touched (a row that
// fo_verdict poisoned keeps its NaNs)
FO_HIDDEN_LADDER_HD void fo_hidden_ladder_verdict_fold(const fo_hidden_ladder_verdict_t &r, int L, double a_limit, double *cost_row,
                                                       uint8_t *safe) {
  cost_row[FO_C_RES0] = r.decel;
  cost_row[FO_C_RES1] = (double)r.user;
  if (r.need == L || r.decel > a_limit) {
    *safe = 0;
    cost_row[FO_C_SAFE] = 0.0;
  }
}
