// fo_hidden_verdict.hpp -- what the hidden-traffic fail-safe verdict (fo_scene_hidden_brake_verdict; DESIGN.md §5.10 "Fail-safe
// verdict") decides per trajectory once the walk has its commit per class: the number of leading brake starts that are fail-safe,
// the class that ends them, the fail-closed row of a candidate with a non-finite pose, and what of that goes into the cost row and the
// safety flag.  Plain functions of values, compiled for the device by fo_scene.hip (fo_hidden_brake_verdict.hpp calls them from lane
// 0 of each trajectory) and for the host by tests/test_hidden_brake_verdict_cpu.py (the style of fo_verdict.hpp with
// tests/test_rule_refusal_cpu.py).  The definition stands in include/fo_hip.h, steps 1 - 5.
#pragma once
#include <stdint.h>
#include "fo_hip.h"

#if defined(__HIPCC__)
#define FO_HIDDEN_VERDICT_HD __host__ __device__ __forceinline__
#else
#define FO_HIDDEN_VERDICT_HD inline
#endif

struct fo_hidden_verdict_t {
  int32_t fail_safe;   // leading brake starts from which braking keeps the ego clear of every class: 0 .. B
  int32_t user;        // the lowest class that ends them, -1 = none (fail_safe = B), FO_HIDDEN_VERDICT_NOT_FINITE = fails closed
};

// step 1: the commit of fo_scene_hidden_brake_users seen through the B brake starts that were asked for
FO_HIDDEN_VERDICT_HD int32_t fo_hidden_verdict_commit(int32_t commit_users, int B) {
  return commit_users >= 0 && commit_users < B ? commit_users : -1;
}

// steps 2 - 4 over commit[c], c < C <= NC (step 1 applied): NC is the caller's compile-time width, so that a kernel's per-class
// registers are indexed by an unrolled loop alone
template <int NC>
FO_HIDDEN_VERDICT_HD fo_hidden_verdict_t fo_hidden_verdict_classes(const int32_t (&commit)[NC], int C, int B, bool finite) {
  fo_hidden_verdict_t r{B, -1};
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int c = 0; c < NC; ++c)
    if (c < C && commit[c] >= 0 && commit[c] < r.fail_safe) {   // (strictly below: a tie stays with the lowest class)
      r.fail_safe = commit[c];
      r.user = c;
    }
  if (!finite) {
    r.fail_safe = 0;
    r.user = FO_HIDDEN_VERDICT_NOT_FINITE;
  }
  return r;
}

// step 5: the two reserved columns always; the flag and FO_C_SAFE only ever lose safety; no other column is touched (a row that
// fo_verdict poisoned keeps its NaNs)
FO_HIDDEN_VERDICT_HD void fo_hidden_verdict_fold(const fo_hidden_verdict_t &r, int commit_min, double *cost_row, uint8_t *safe) {
  cost_row[FO_C_RES0] = (double)r.fail_safe;
  cost_row[FO_C_RES1] = (double)r.user;
  if (r.fail_safe < commit_min) {
    *safe = 0;
    cost_row[FO_C_SAFE] = 0.0;
  }
}
