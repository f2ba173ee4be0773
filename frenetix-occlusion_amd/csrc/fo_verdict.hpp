// fo_verdict.hpp -- what fo_reduce_kernel decides per trajectory once the chunk partials are folded: the safety flag and
// which cost columns a poisoned agent set takes away.  Plain functions of values, compiled for the device by fo_sweep.hip
// and for the host by tests/test_rule_refusal_cpu.py (the style of fo_rule_plan.hpp with tests/test_rule_plan_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>
#include "fo_hip.h"

#if defined(__HIPCC__)
#define FO_VERDICT_HD __host__ __device__ __forceinline__
#else
#define FO_VERDICT_HD inline
#endif

// the folded partials of one trajectory (the float columns of its cost row, and the DCE flag)
struct fo_folded_t {
  double min_ttc, min_dce, max_er, max_or, max_eh, max_oh, max_cp, max_hwc, min_ttce, arg_dce, arg_ttc, arg_or, max_btn, flag;
};

// Returns the safety flag; poisons f where the agent set cannot be judged.
//   cov_unusable: the set holds a matrix that is no usable covariance (status word 0 of this generation) -- gated on the
//     metrics that read a collision probability, and on A > 0 like every threshold (no agents -> ({}, True), metric.py:44-45);
//   refused: the set holds a refused rule list (status word 2) -- NOT gated: the agents that are missing would have
//     mattered to every metric, so no column of the row is a usable number and the trajectory is not safe, whatever the
//     mask and however many slots the set has.
FO_VERDICT_HD bool fo_verdict(int A, uint32_t mask, const fo_thresholds_t &thr, bool cov_unusable, bool refused, fo_folded_t &f) {
  bool ok = true;
  if (A > 0) {
    if ((mask & FO_M_HR) && f.max_hwc > thr.harm) ok = false;  // NaN thresholds compare false = disabled
    if ((mask & FO_M_HR) && f.max_or > thr.risk) ok = false;
    if ((mask & FO_M_HR) && f.max_cp > thr.cp) ok = false;
    if ((mask & FO_M_TTC) && f.min_ttc < thr.ttc) ok = false;
    if ((mask & FO_M_DCE) && f.flag > 0.0) ok = false;
    if ((mask & FO_M_BE) && f.max_btn > thr.be) ok = false;  // metric.py:54-61
    // The current agent set holds an off-diagonal covariance (fo_prep_agents_kernel poisoned those rows and tagged
    // the status word with this generation): fmax() in the fold drops the NaNs, so say it here -- nothing that depends
    // on a collision probability may read as "safe", whether or not the caller runs fo_sweep_check.
    if ((mask & (FO_M_CP | FO_M_HR)) && cov_unusable) {
      ok = false;
      f.max_cp = f.max_er = f.max_or = f.max_hwc = NAN;
    }
  }
  if (refused) {
    ok = false;
    f.min_ttc = f.min_dce = f.max_er = f.max_or = f.max_eh = f.max_oh = f.max_cp = f.max_hwc = f.min_ttce = NAN;
    f.arg_dce = f.arg_ttc = f.arg_or = f.max_btn = NAN;
  }
  return ok;
}
