// fo_rule_pedestrian.hpp -- the two pedestrian families of the spawn rules: behind a turn (one wave) and behind a visible static
// obstacle (a wave per cross line).  Each writes its per-workgroup record; fo_spawn_rules_select_kernel applies what depends on
// the order of the obstacles.
#pragma once
#include "fo_rule_frame.hpp"

namespace {

// ---------------------------------------------------------------- pedestrian behind a turn (one wave)
// rec: [0] valid, [1] x, [2] y, [3] s_ph, [4] d (the lateral phantom offset), [5] source
__device__ __forceinline__ void rl_turn_rule(const RuleView &v, const RuleParams &pr, double *rec, double *lx, double *ly, double *cum,
                             unsigned char *inside) {
  const int lane = threadIdx.x & 63;
  if (lane == 0) rec[0] = 0.0;
  const int nw = pr.win_i1 - pr.win_i0;
  if (nw < 2) return;
  if (nw > RL_TURNW) { if (lane == 0) rec[0] = -1.0; return; }   // (refused by the host entry already; -1: out of table space, see the selection kernel)
  const bool left = pr.intention == 1;
  // the line: the reference window, for a left turn shifted 3 m to the left (spawn_locator.py:510-518) -- at the POLYLINE arc
  // lengths of the window's vertices (`reference_s`, :683), which the caller's table holds in column 3
  bool ok = true;
  for (int i = lane; i < nw; i += 64) {
    const double *q = v.path + 6 * (size_t)(pr.win_i0 + i);
    double x = q[0], y = q[1];
    if (left) ok = rl_to_cart(v, v.frame ? q[3] : q[2], 3.0, x, y) && ok;
    lx[i] = x;
    ly[i] = y;
  }
  if (__ballot(!ok)) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  if (lane == 0) {
    cum[0] = 0.0;
    for (int i = 1; i < nw; ++i) cum[i] = cum[i - 1] + sqrt((lx[i] - lx[i - 1]) * (lx[i] - lx[i - 1]) + (ly[i] - ly[i - 1]) * (ly[i] - ly[i - 1]));
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const double total = cum[nw - 1], step = v.cs / 8.0;
  if (!(total > 0.0)) return;
  const int ns = (int)ceil((total + 0.5 * step) / step);
  if (ns > RL_MAXSAMP) { if (lane == 0) rec[0] = -1.0; return; }   // a line longer than the sample table (cells below 0.32 m at a 40 m window)
  for (int i = lane; i < ns; i += 64) {
    double x, y;
    rl_sample(lx, ly, cum, nw, fmin((double)i * step, total), x, y);
    inside[i] = (rl_class_at(v, x, y) & 4) ? 1 : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  // runs of consecutive samples in occluded cells: the first point of the only run, of the LAST run when there are several (:528)
  int first_of_last = -1;
  for (int i = lane; i < ns; i += 64)
    if (inside[i] && (i == 0 || !inside[i - 1])) first_of_last = i;      // ascending per lane: its last run start
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) first_of_last = max(first_of_last, __shfl_xor(first_of_last, off));
  if (first_of_last < 0) return;
  double fx, fy;
  rl_sample(lx, ly, cum, nw, fmin((double)first_of_last * step, total), fx, fy);
  double s_int, d_int;
  if (!rl_to_curv_wave(v, fx, fy, s_int, d_int)) return;
  if (lane != 0) return;
  double s_ph = s_int + (left ? -0.5 : 0.0);
  if (s_ph > pr.s_threshold || s_ph < pr.ego_s + 3.0) return;                    // :542
  const double d_ph = left ? 1.0 : -1.0, d_off = d_ph + (left ? 3.0 : 0.0);     // :546
  double x, y;
  if (!rl_to_cart(v, s_ph, d_off, x, y)) return;
  while (rl_disc_touches(v, x, y, 0.5, 2)) {                                     // :552-554
    s_ph += 0.5;
    if (!rl_to_cart(v, s_ph, d_off, x, y)) return;
  }
  rec[1] = x; rec[2] = y; rec[3] = s_ph; rec[4] = d_ph; rec[5] = left ? RL_SRC_LEFT : RL_SRC_RIGHT;
  rec[0] = 1.0;   // (the obstacle and heading conditions, :557-572, are applied by the selection workgroup)
}

// the static rule's point on a sampled cross line (sx, sy, near: ns samples; cx, cy: the obstacle's centre); lane 0's verdict counts
// candidates: where "the disc touches the visible area" flips, the sample just outside (:414-415) -- a lane per sample
// pair; one candidate: that one; several (MultiPoint, :419-433): the one nearest to the lanelet's first left vertex among
// those inside the occluded area (the first of equally near ones: smallest (distance, index) over the wave)
__device__ __forceinline__ bool rl_static_candidate(const RuleView &v, double cx, double cy, int ns, const double *sx, const double *sy,
                                                    const unsigned char *near, double &spx, double &spy) {
  const int lane = threadIdx.x & 63;
  bool okp = false;
  int n_c = 0, only = -1;
  for (int i = lane; i + 1 < ns; i += 64)
    if (near[i] != near[i + 1]) { ++n_c; only = near[i] ? i + 1 : i; }
  int n_all = n_c, only_all = only;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { n_all += __shfl_xor(n_all, off); only_all = max(only_all, __shfl_xor(only_all, off)); }
  bool found = false;
  if (n_all == 1) {
    spx = sx[only_all]; spy = sy[only_all]; found = true;
  } else if (n_all > 1) {
    const int ll = rl_lanelet_of_wave(v, cx, cy);
    const double anx = (ll >= 0 && v.left0) ? v.left0[2 * ll] : cx, any_ = (ll >= 0 && v.left0) ? v.left0[2 * ll + 1] : cy;
    double bestd = INFINITY;
    int bc = 0x7fffffff, bi = 0x7fffffff;   // candidate sample, and the sample pair it came from (orders ties)
    for (int i = lane; i + 1 < ns; i += 64)
      if (near[i] != near[i + 1]) {
        const int c = near[i] ? i + 1 : i;
        const double dd = sqrt((anx - sx[c]) * (anx - sx[c]) + (any_ - sy[c]) * (any_ - sy[c]));
        if ((rl_class_at(v, sx[c], sy[c]) & 4) && dd < bestd) { bestd = dd; bc = c; bi = i; }   // ascending per lane: first minimum
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double d2 = __shfl_xor(bestd, off);
      const int c2 = __shfl_xor(bc, off), i2 = __shfl_xor(bi, off);
      if (d2 < bestd || (d2 == bestd && i2 < bi)) { bestd = d2; bc = c2; bi = i2; }
    }
    if (bc != 0x7fffffff) { spx = sx[bc]; spy = sy[bc]; found = true; }
  }
  okp = found;
  if (okp && lane == 0) {
    bool any, all;
    rl_disc(v, spx, spy, 0.15, 2, any, all);
    if (any) okp = false;                                                     // :440
    rl_disc(v, spx, spy, 0.15, 1, any, all);
    if (!all) okp = false;                                                    // :444
  }
  return okp;
}

// ---------------------------------------------------------------- pedestrian behind a static obstacle (two waves)
// rec: [0] distance to the ego, [1] role (1 static candidate, 2 dynamic candidate, 0 nothing), per line li = 0, 1:
// [2 + 6 li] valid, x, y, s, d, yaw
// Wave li of the workgroup takes cross line li (the rear and the front end of the obstacle's extent along the path): the two
// lines are independent chains of projections and class look-ups, a wave's worth of latency each.  Both waves work out the
// obstacle's extent for themselves (the same arithmetic: no exchange); sx, sy, near: this wave's scratch.
__device__ __forceinline__ void rl_static_rule(const RuleView &v, const RuleParams &pr, int o, int O, const double *ocorn, const double *ocen,
                               const uint8_t *oflags, const uint8_t *ovis, double *rec, double *sx, double *sy,
                               unsigned char *near, int li) {
  const int lane = threadIdx.x & 63;
  const double cx = ocen[2 * o], cy = ocen[2 * o + 1];
  const double *oc = ocorn + 8 * (size_t)o;
  if (lane == 0) rec[2 + 6 * li] = 0.0;
  if (sqrt((pr.ego_x - cx) * (pr.ego_x - cx) + (pr.ego_y - cy) * (pr.ego_y - cy)) > RL_MAX_DIST_OBST) return;   // :369
  // the centre and the four corners in one pass over the path (rl_to_curv_wave_n)
  const double p5x[5] = {cx, oc[0], oc[2], oc[4], oc[6]}, p5y[5] = {cy, oc[1], oc[3], oc[5], oc[7]};
  double p5s[5], p5d[5];
  const unsigned ok5 = rl_to_curv_wave_n<5>(v, p5x, p5y, p5s, p5d);
  if (!(ok5 & 1u)) return;
  const double ob_s = p5s[0];
  // :380 compares with ego s + s_threshold although s_threshold already contains ego s (kept as in the reference)
  if (pr.ego_s + pr.s_threshold < ob_s || ob_s < pr.ego_s + 3.0) return;
  if (ok5 != 31u) return;
  double s_min = INFINITY, s_max = -INFINITY, d_min = INFINITY, d_max = -INFINITY;
  for (int i = 1; i < 5; ++i) {
    s_min = fmin(s_min, p5s[i]); s_max = fmax(s_max, p5s[i]); d_min = fmin(d_min, p5d[i]); d_max = fmax(d_max, p5d[i]);
  }
  s_min -= 0.8; s_max += 0.8; d_min -= 0.8; d_max += 0.8;                          // :384-390
  double yaw_l = 0.0;
  const bool have_yaw = rl_lane_yaw_at(v, cx, cy, yaw_l);
  for (int once = 0; once < 1; ++once) {   // (this wave's line; `continue` = no point on it)
    const double s_line = li == 0 ? s_min : s_max;
    double ax, ay, bx, by;
    if (!rl_to_cart(v, s_line, d_min, ax, ay) || !rl_to_cart(v, s_line, d_max, bx, by)) continue;
    const double total = sqrt((bx - ax) * (bx - ax) + (by - ay) * (by - ay)), step = v.cs / 8.0;
    if (!(total > 0.0)) continue;
    const int ns = (int)ceil((total + 0.5 * step) / step);
    if (ns > RL_MAXSAMP) { if (lane == 0) rec[2 + 6 * li] = -1.0; continue; }       // (a cross line of > 64 m at 0.5 m cells: out of table space)
    const double b = pr.ped_length / 2.0 * 1.3;                                    // :414
    bool t_occ = false, t_vis = false;
    for (int i = lane; i < ns; i += 64) {
      const double q = fmin((double)i * step, total);
      double x = bx, y = by;
      if (q < total) { x = (bx - ax) / total * q + ax; y = (by - ay) / total * q + ay; }
      sx[i] = x; sy[i] = y;
      const int c = rl_class_at(v, x, y);
      t_occ = t_occ || (c & 4);
      t_vis = t_vis || (c & 2);
      near[i] = rl_disc_touches(v, x, y, b, 2) ? 1 : 0;
    }
    if (!__ballot(t_occ) || !__ballot(t_vis)) continue;                           // :406-408
    bool blocked = false;                                                         // :409-411: any VISIBLE obstacle within half a pedestrian width
    for (int j = lane; j < O; j += 64)
      if ((oflags[j] & 1) && ovis[j] && rl_seg_rect_distance(ax, ay, bx, by, ocorn + 8 * (size_t)j) <= pr.ped_width / 2.0) blocked = true;
    if (__ballot(blocked)) continue;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double spx = 0.0, spy = 0.0;
    const bool okp = rl_static_candidate(v, cx, cy, ns, sx, sy, near, spx, spy);
    // the point's curvilinear position: projected by the whole wave (lane 0 holds the point)
    const bool okw = __shfl((int)okp, 0) != 0;
    spx = __shfl(spx, 0);
    spy = __shfl(spy, 0);
    double ss = 0.0, sd = 0.0;
    const bool okc = okw && rl_to_curv_wave(v, spx, spy, ss, sd);
    if (lane == 0) {
      double *r = rec + 2 + 6 * li;
      r[0] = (okc && have_yaw) ? 1.0 : 0.0; r[1] = spx; r[2] = spy; r[3] = ss; r[4] = sd; r[5] = yaw_l + 1.5707963267948966;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
}

}  // namespace
