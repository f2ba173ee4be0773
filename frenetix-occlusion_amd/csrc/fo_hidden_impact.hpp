// fo_hidden_impact.hpp -- what the hidden-traffic impact verdict (fo_scene_hidden_brake_impact; DESIGN.md §5.10 "Impact verdict")
// makes of the speed the ego has left where a braking manoeuvre is hit: the harm row of a class of hidden road user, the two
// logistics, the choice of the class, the fail-closed row of a candidate with a non-finite pose, and what of that goes into the cost
// row and the safety flag.  Plain functions of values, compiled for the device by fo_scene.hip (fo_hidden_brake_impact.hpp calls them
// from lane 0 of each trajectory) and for the host by fo_scene_hidden.hpp (fo_hidden_impact_row) and
// tests/test_hidden_impact_cpu.py (the style of fo_hidden_verdict.hpp).  The definition stands in include/fo_hip.h, steps 4 - 7.
//
// WHAT A ROW MEANS.  The reference prices a (pose, obstacle sample) pair by the MAIS3+ probability of harm_model.py:80-155: the
// speed change dv = sqrt(v_ego^2 + v_obs^2 + 2 v_ego v_obs cos(pdof)) is split by mass -- m_obs / (m_ego + m_obs) of it for the ego,
// m_ego / (m_ego + m_obs) for the obstacle -- and goes through a logistic whose constant depends, for a protected road user, on the
// area of impact (LR4S, logistic_regression.py:11-52: front 0, side, rear).  A hidden road user has a speed and a kind; its heading
// and the area of impact are unknown.  The row states the reference's harm at its WORST over both:
//   dv    is greatest head-on: cos(pdof) = 1 gives dv = v_ego + v_obs = w;
//   area  the logistic rises with the area term, so the term is max(0, lr4s_side, lr4s_rear) -- `side` with the shipped
//         coefficients; taken as the maximum, so that the row stays a bound under another coefficient file.
// With split_ego = m_obs / (m_ego + m_obs), split_obst = m_ego / (m_ego + m_obs), m_obs the reference's mass by type and size
// (harm_model.py:158-190), harm = 1 / (1 + exp(p0 + p1 w)) for the obstacle and 1 / (1 + exp(p2 + p3 w)) for the ego with
//   protected (LR4S for both, harm_model.py:127-133)          p0 = -lr4s_const - area   p1 = -lr4s_speed * split_obst
//                                                              p2 = -lr4s_const - area   p3 = -lr4s_speed * split_ego
//   unprotected (pedestrian, bicycle, ...; :135-147)          p0 =  ped_const           p1 = -ped_speed  * split_obst
//                                                              p2 = -lr1s_const          p3 = -lr1s_speed * split_ego
// A type whose protection entry is None (harm_model.py:26-30: the reference answers 1 for it) has no row: the host refuses it.
#pragma once
#include <math.h>
#include <stdint.h>
#include "fo_hip.h"

#if defined(__HIPCC__)
#define FO_HIDDEN_IMPACT_HD __host__ __device__ __forceinline__
#else
#define FO_HIDDEN_IMPACT_HD inline
#endif

// the reference's tables by type (harm_model.py:15-32, 158-190), for the host and the device alike
FO_HIDDEN_IMPACT_HD double fo_hidden_impact_mass(int type, double size) {
  switch (type) {
    case FO_TYPE_CAR: case FO_TYPE_PRIORITY_VEHICLE: case FO_TYPE_PARKED_VEHICLE: case FO_TYPE_TAXI:
      return -1333.5 + 526.9 * pow(size, 0.8);
    case FO_TYPE_TRUCK: return 25000.0;
    case FO_TYPE_BUS: return 13000.0;
    case FO_TYPE_BICYCLE: return 90.0;
    case FO_TYPE_PEDESTRIAN: return 75.0;
    case FO_TYPE_TRAIN: return 118800.0;
    case FO_TYPE_MOTORCYCLE: return 250.0;
    default: return 0.0;
  }
}
// 1 protected, 0 unprotected, 2 = None
FO_HIDDEN_IMPACT_HD int fo_hidden_impact_protection(int type) {
  switch (type) {
    case FO_TYPE_CAR: case FO_TYPE_TRUCK: case FO_TYPE_BUS: case FO_TYPE_PRIORITY_VEHICLE:
    case FO_TYPE_PARKED_VEHICLE: case FO_TYPE_TRAIN: case FO_TYPE_TAXI: return 1;
    case FO_TYPE_BICYCLE: case FO_TYPE_PEDESTRIAN: case FO_TYPE_MOTORCYCLE: case FO_TYPE_UNKNOWN: return 0;
    default: return 2;
  }
}

// the row (p0, p1, p2, p3) of a road user of `type` and `size` = length * width against an ego of ego_mass; false: no row (the
// type has no protection entry), row is left alone
FO_HIDDEN_IMPACT_HD bool fo_hidden_impact_row_of(int type, double size, double ego_mass, const fo_harm_coeff_t &hc, double (&row)[4]) {
  const int prot = fo_hidden_impact_protection(type);
  if (prot == 2) return false;
  const double m_obs = fo_hidden_impact_mass(type, size);
  const double split_ego = m_obs / (ego_mass + m_obs), split_obst = ego_mass / (ego_mass + m_obs);
  if (prot == 1) {
    const double area = fmax(0.0, fmax(hc.lr4s_side, hc.lr4s_rear));
    row[0] = -hc.lr4s_const - area;
    row[1] = -hc.lr4s_speed * split_obst;
    row[2] = -hc.lr4s_const - area;
    row[3] = -hc.lr4s_speed * split_ego;
  } else {
    row[0] = hc.ped_const;
    row[1] = -hc.ped_speed * split_obst;
    row[2] = -hc.lr1s_const;
    row[3] = -hc.lr1s_speed * split_ego;
  }
  return true;
}

// step 4: one logistic, float64, plain exp
FO_HIDDEN_IMPACT_HD double fo_hidden_impact_logistic(double p_const, double p_speed, double w) {
  return 1.0 / (1.0 + exp(p_const + p_speed * w));
}

struct fo_hidden_impact_t {
  double obst_harm, ego_harm;   // of the chosen class; (0, 0) without one, (1, 1) where the candidate fails closed
  int32_t user;                 // the lowest class with a hit whose obstacle harm is greatest, -1 = no class has a hit,
                                // FO_HIDDEN_VERDICT_NOT_FINITE = fails closed
};

// steps 4 - 6 over speed[c], at[c], c < C <= NC: NC is the caller's compile-time width, so that a kernel's per-class registers are
// indexed by an unrolled loop alone.  rows [C][4], speed_of [C].
template <int NC>
FO_HIDDEN_IMPACT_HD fo_hidden_impact_t fo_hidden_impact_classes(const double (&speed)[NC], const int32_t (&at)[NC], int C,
                                                                const double *rows, const double *speed_of, bool finite) {
  fo_hidden_impact_t r{0.0, 0.0, -1};
  double best = -1.0;                   // (below every harm; strictly above it: a tie stays with the lowest class, a NaN never wins)
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int c = 0; c < NC; ++c)
    if (c < C && at[c] >= 0) {
      const double w = speed[c] + speed_of[c];
      const double ho = fo_hidden_impact_logistic(rows[4 * c], rows[4 * c + 1], w);
      const double he = fo_hidden_impact_logistic(rows[4 * c + 2], rows[4 * c + 3], w);
      if (ho > best) {
        best = ho;
        r.obst_harm = ho;
        r.ego_harm = he;
        r.user = c;
      }
    }
  if (!finite) {
    r.obst_harm = 1.0;
    r.ego_harm = 1.0;
    r.user = FO_HIDDEN_VERDICT_NOT_FINITE;
  }
  return r;
}

// the same steps where the caller holds the closing speed w of each class itself (fo_scene_hidden_brake_impact_lanes, whose w is no
// sum: csrc/fo_hidden_approach.hpp): the two logistics at closing[c], the same choice, the same fail-closed row
template <int NC>
FO_HIDDEN_IMPACT_HD fo_hidden_impact_t fo_hidden_impact_classes_closing(const double (&closing)[NC], const int32_t (&at)[NC], int C,
                                                                        const double *rows, bool finite) {
  fo_hidden_impact_t r{0.0, 0.0, -1};
  double best = -1.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int c = 0; c < NC; ++c)
    if (c < C && at[c] >= 0) {
      const double ho = fo_hidden_impact_logistic(rows[4 * c], rows[4 * c + 1], closing[c]);
      const double he = fo_hidden_impact_logistic(rows[4 * c + 2], rows[4 * c + 3], closing[c]);
      if (ho > best) {
        best = ho;
        r.obst_harm = ho;
        r.ego_harm = he;
        r.user = c;
      }
    }
  if (!finite) {
    r.obst_harm = 1.0;
    r.ego_harm = 1.0;
    r.user = FO_HIDDEN_VERDICT_NOT_FINITE;
  }
  return r;
}

// step 7: the two reserved columns always; the flag and FO_C_SAFE only ever lose safety; no other column is touched (a row that
// fo_verdict poisoned keeps its NaNs)
FO_HIDDEN_IMPACT_HD void fo_hidden_impact_fold(const fo_hidden_impact_t &r, double harm_limit, double *cost_row, uint8_t *safe) {
  cost_row[FO_C_RES0] = r.obst_harm;
  cost_row[FO_C_RES1] = (double)r.user;
  if (r.obst_harm > harm_limit || r.user == FO_HIDDEN_VERDICT_NOT_FINITE) {
    *safe = 0;
    cost_row[FO_C_SAFE] = 0.0;
  }
}
