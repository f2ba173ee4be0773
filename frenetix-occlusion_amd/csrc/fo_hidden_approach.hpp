// fo_hidden_approach.hpp -- what the impact verdict by approach angle (fo_scene_hidden_brake_impact_lanes; DESIGN.md §5.10 "Impact
// verdict by approach angle") makes of the move bytes under a hit pose: the directions the lanes allow there, the greatest cosine of
// the reference's principal direction of force they leave, and the closing speed at that cosine.  Plain functions of values, compiled
// for the device by fo_scene.hip (fo_hidden_brake_impact_lanes.hpp calls them where a class is first hit) and for the host by
// tests/test_hidden_impact_lanes_cpu.py (the style of fo_hidden_impact.hpp).  The definition stands in include/fo_hip.h, steps 3 - 4.
//
// WHAT A MOVE BYTE SAYS.  scenario.lane_move_raster sets bit k of a cell iff cos(k 45° - yaw) >= cos(67.5°) for a lanelet of heading
// yaw that contains the cell (the union over the lanelets; 0xFF off-lane).  Direction k is CENTRAL in a byte when bits k - 1, k and
// k + 1 (mod 8) are all set: every heading that generates a byte with a central direction lies within 22.5° of a central one, so the
// headings of a lane-abiding vehicle on the cell are H = the union over the central k of [k 45° - h, k 45° + h], h = 22.5° +
// heading_slack.  A byte without a central direction says nothing and is priced head-on.
// The reference's dv = sqrt(v_ego^2 + v_obs^2 + 2 v_ego v_obs cos(pdof)), pdof = yaw_obs - theta_ego + pi (harm_model.py:81-95), is
// greatest where cos(pdof) is: with g_k = cos(k 45° - theta_ego + pi) = -(cos theta cos k45 + sin theta sin k45) the greatest cosine
// over [k 45° - h, k 45° + h] is 1 if the sector holds theta_ego + pi (g_k >= cos h) and cos(acos(g_k) - h) = g_k cos h +
// sqrt(1 - g_k^2) sin h otherwise.  No trigonometric call: cos h and sin h come from the host, the lattice vectors are constants.
#pragma once
#include <math.h>
#include <stdint.h>
#include "fo_hidden_impact.hpp"

// bit k: direction k is central in the byte mv
FO_HIDDEN_IMPACT_HD unsigned fo_hidden_approach_central(unsigned mv) {
  const unsigned m = mv & 0xffu;
  return m & ((m << 1 | m >> 7) & 0xffu) & ((m >> 1 | m << 7) & 0xffu);
}

// step 3: cm, the greatest cos(pdof) the move bytes mv under a hit pose of unit heading (ct, st) allow a class; `bound`: the class
// is lane-bound.  cos_h <= -1 states h >= pi: head-on.
FO_HIDDEN_IMPACT_HD double fo_hidden_approach_cosine(unsigned mv, bool bound, double ct, double st, double cos_h, double sin_h) {
  const unsigned central = fo_hidden_approach_central(mv);
  if (!bound || central == 0u || !(cos_h > -1.0)) return 1.0;
  const double R = 0.70710678118654757;   // sqrt(0.5), correctly rounded
  double cm = 0.0;
  bool any = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 8; ++k)
    if (central >> k & 1u) {
      const double ck = k == 0 ? 1.0 : (k == 4 ? -1.0 : (k == 2 || k == 6 ? 0.0 : (k == 1 || k == 7 ? R : -R)));
      const double sk = k == 2 ? 1.0 : (k == 6 ? -1.0 : (k == 0 || k == 4 ? 0.0 : (k == 1 || k == 3 ? R : -R)));
      const double g = -(ct * ck + st * sk);
      const double c = g >= cos_h ? 1.0 : g * cos_h + sqrt(fmax(0.0, 1.0 - g * g)) * sin_h;
      if (!any || c > cm) cm = c;
      any = true;
    }
  return cm;
}

// step 4: the closing speed of an ego at u against a user at s under the cosine cm; cm == 1.0 is u + s, bit for bit the head-on stage's
FO_HIDDEN_IMPACT_HD double fo_hidden_approach_closing(double u, double s, double cm) {
  if (cm == 1.0) return u + s;
  return sqrt(fmax(0.0, u * u + s * s + 2.0 * u * s * cm));
}
