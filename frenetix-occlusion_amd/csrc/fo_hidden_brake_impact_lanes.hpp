// fo_hidden_brake_impact_lanes.hpp -- the hidden-traffic impact verdict by approach angle (fo_scene_hidden_brake_impact_lanes;
// DESIGN.md §5.10 "Impact verdict by approach angle"): the impact verdict of fo_hidden_brake_impact.hpp with every lane-bound class
// priced at the worst closing speed the lanes' driving directions allow at the cells where it meets the ego, instead of head-on.
// An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_brake_impact.hpp (same translation unit, same
// flags: -ffp-contract=off); it stages with hbu_stage, forms first[c] with hbu_first and walks with hbu_walk, whose hit hook hands it
// the pose at which a class is first hit.  The arithmetic of steps 3 - 4 is fo_hidden_approach.hpp's.
//
// Inputs are those of fo_hr_brake_impact_kernel, and the map's move table [rny][rnx], dir_mask (bit c: class c is lane-bound; the
// host hands over 0 where h >= pi) and cos_h, sin_h.  The definition stands in include/fo_hip.h.
//   hbil_moves           one further fo_hr_scan_pose_rows over a hit pose: per class of `cls` the OR of the move bytes of the cells
//                        whose key on that class's map is <= its threshold -- hbu_hits on the keys of ONE cell, so the class's map
//                        is picked by the class masks as everywhere in the family.  A cell off the raster gives 0xFF.
//   fo_hr_brake_impact_lanes_kernel<NC, NK>  the lanes, the grid and the LDS of the verdict kernel (brake_verdict_*).  Next to
//                        commit[c] a lane keeps (closing[c], at[c], cosine[c]).  A class first hit at a moving pose of the manoeuvre
//                        from b -- and not met by the candidate itself at fm[c] <= b -- is priced in the hook: a class is first hit
//                        at most once per manoeuvre, so the further scan runs at most C times per (m, b), and only for lane-bound
//                        classes.  The "met" case has ONE closing speed per class and trajectory (pose fm[c], speed v[fm[c]]) and
//                        its lowest start is fm[c]: the lanes of the trajectory split the classes after the loop over b -- where
//                        the walk's registers are free -- and merge it under the reduction's own rule (the larger closing speed, on
//                        equal closing speed the lower start).  Lane 0 prices with fo_hidden_impact_classes_closing.
// The class a hook or the met case prices is a run-time value: its scalars (threshold row, speed, move byte) are read at it, and its
// registers are reached by fully unrolled compare-and-select loops alone, never indexed.
// Bounds, next to fo_hidden_brake_users.hpp's: the move table is read at (gx, gy) tested against the raster alone, and only for a
// class of dir_mask -- with dir_mask = 0 it may be null; speed_of and the table are read at c < C.  Every byte of every output is
// written; of cost and safe only what the definition names.  Plain vector stores, no atomics.
#pragma once
#include <type_traits>
#include "fo_hidden_approach.hpp"
#include "fo_hidden_brake_impact.hpp"

namespace {

struct HrBrakeImpactLanesArgs {
  int M, T, G, P, C, B;                 // as HrBrakeImpactArgs
  const double *x, *y, *heading;
  const int32_t *len;
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;
  const int32_t *key0, *key1, *key2;
  const int32_t *qmin0, *qmin1, *qmin2;
  uint32_t map_of;
  const double *v, *arc;
  double a_brake, dt;
  const double *speed_of, *rows;        // [C], [C][4]
  double harm_limit;
  const uint8_t *moves;                 // [rny][rnx] the map's move table; may be null with dir_mask = 0
  uint32_t dir_mask;                    // bit c: class c is lane-bound
  double cos_h, sin_h;
  const uint8_t *finite;
  double *cost;
  uint8_t *safe;
  double *harm;                         // [M][2]
  int32_t *user;                        // [M]
  double *closing, *cosine;             // [C][M]
  int32_t *at, *commit, *first;         // [C][M]
};
static_assert(sizeof(HrBrakeImpactLanesArgs) + sizeof(HbThr) <= 4096, "the arguments, map_of and the table fit the kernel-argument segment");

// byte c: the OR of the move bytes of the cells under the pose (px, py, pc, ps) whose key on the map of class c is <= thr[c][i], for
// the classes c of `cls` (a subset of the classes that are there)
template <int NC, int NK, class Args>
__device__ __forceinline__ uint64_t hbil_moves(const Args &a, const int32_t *TH, int i, double px, double py, double pc, double ps,
                                               unsigned cls, const HbuMasks &mk, const HrBox &sb) {
  typename std::conditional<(NC <= 4), uint32_t, uint64_t>::type mv = 0;
  fo_hr_scan_pose_rows(a, px, py, pc, ps, a.key0, HC_NONE, sb.lox, sb.loy, sb.hix, sb.hiy, 0, 1, [&](int kv, int gx, int gy) {
    HbuKeys q{kv, kv, kv};              // outside the window: 0 or NONE, the same for every map
    if constexpr (NK > 1) {
      const int wx = gx - a.ix0, wy = gy - a.iy0;
      if (wx >= 0 && wx < a.nx && wy >= 0 && wy < a.ny) {
        q.q1 = a.key1[wy * a.nx + wx];
        if constexpr (NK > 2) q.q2 = a.key2[wy * a.nx + wx];
      }
    }
    const unsigned h = hbu_hits<NC, NK>(q, TH, a.T, i, cls, mk.cm1, mk.cm2);
    if (h) {
      const bool on = gx >= 0 && gx < a.rnx && gy >= 0 && gy < a.rny;
      const decltype(mv) byte = on ? a.moves[(size_t)gy * a.rnx + gx] : 0xFFu;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (h >> c & 1u) mv |= byte << (8 * c);
    }
  });
  return mv;
}

// dynamic LDS: brake_verdict_lds_bytes(T, K, C, B)
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_impact_lanes_kernel(const HrBrakeImpactLanesArgs a, const HbThr thr) {
  extern __shared__ double hbil_rows[]; // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin per map, then thr
  const int G = a.G, T = a.T, B = a.B, nc = a.C, per_block = a.P;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = sub < per_block && m < a.M;
  int32_t *QM = (int32_t *)(hbil_rows + (size_t)per_block * 6 * T);  // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  hbu_stage<NK>(a, hbil_rows, QM, TH, m0, per_block, [&](int t) { return thr.v[t]; });
  __syncthreads();
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hbil_rows + (size_t)row_of * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  int fm[NC];
  hbu_first<NC, NK>(QM + (size_t)row_of * T, (size_t)per_block * T, TH, T, Lm, kl, G, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  int32_t commit[NC], at[NC];           // at: 0x7fffffff = no hit start yet, so that the lower start wins among equal closing speeds
  double closing[NC], cosine[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    commit[c] = 0x7fffffff;
    at[c] = 0x7fffffff;
    closing[c] = -INFINITY;
    cosine[c] = 1.0;
  }
  const int ends = B < Lm ? B : Lm;     // brake starts with a manoeuvre (Lm = 0 on lanes without a trajectory)
  for (int b = kl; b < ends; b += G) {
    int bf[NC];
    const double vb = V[b];
    const int st = hb_stop_sample(vb, a.a_brake, a.dt, b, Lm);
    unsigned met = 0;                   // the classes the candidate itself meets no later than b: priced once, below
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (fm[c] >= 0 && fm[c] <= b) met |= 1u << c;
    hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a.a_brake, st, mk, sb, bf, [&](int i, const HbPose &p, unsigned h) {
      const unsigned hn = h & ~met;
      if (!hn) return;
      const unsigned hd = hn & a.dir_mask;
      const uint64_t mv = hd ? hbil_moves<NC, NK>(a, TH, i, p.x, p.y, p.c, p.s, hd, mk, sb) : 0;
      const double u = hb_speed(vb, a.a_brake, a.dt, i, b);          // positive: i < st
      for (unsigned r = hn; r; r &= r - 1u) {
        const int c = __builtin_ctz(r);
        const double cm = fo_hidden_approach_cosine((unsigned)(mv >> (8 * c)) & 0xffu, (hd >> c & 1u) != 0, p.c, p.s, a.cos_h, a.sin_h);
        const double w = fo_hidden_approach_closing(u, a.speed_of[c], cm);
#pragma unroll
        for (int cc = 0; cc < NC; ++cc)
          if (cc == c && w > closing[cc]) {      // (ascending b: strictly above keeps the lowest start; a NaN never wins)
            closing[cc] = w;
            at[cc] = b;
            cosine[cc] = cm;
          }
      }
    });
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (hb_unclear(fm[c], b, bf[c], st)) commit[c] = commit[c] < b ? commit[c] : b;
  }
  // the met case: every start b in [fm[c], ends) meets class c at the candidate's own pose fm[c] at v[fm[c]] -- one closing speed,
  // lowest start fm[c]; the lanes of the trajectory split the classes
  for (int c = kl; c < nc; c += G) {
    int f = -1;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
      if (cc == c) f = fm[cc];
    if (f >= 0 && f < ends) {
      const bool bound = (a.dir_mask >> c & 1u) != 0;
      const double pc = X[2 * T + f], ps = X[3 * T + f];
      const uint64_t mv = bound ? hbil_moves<NC, NK>(a, TH, f, X[f], X[T + f], pc, ps, 1u << c, mk, sb) : 0;
      const double cm = fo_hidden_approach_cosine((unsigned)(mv >> (8 * c)) & 0xffu, bound, pc, ps, a.cos_h, a.sin_h);
      const double w = fo_hidden_approach_closing(V[f], a.speed_of[c], cm);
#pragma unroll
      for (int cc = 0; cc < NC; ++cc)
        if (cc == c && (w > closing[cc] || (w == closing[cc] && f < at[cc]))) {
          closing[cc] = w;
          at[cc] = f;
          cosine[cc] = cm;
        }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hb_shfl_min(commit[c], 1, G);       // lanes of a trajectory are G consecutive lanes of one wave
    commit[c] = commit[c] == 0x7fffffff ? -1 : fo_hidden_verdict_commit(commit[c], B);
    for (int o = G >> 1; o >= 1; o >>= 1) {
      const double ws = __shfl_xor(closing[c], o), wc = __shfl_xor(cosine[c], o);
      const int wa = __shfl_xor(at[c], o);
      if (ws > closing[c] || (ws == closing[c] && wa < at[c])) {
        closing[c] = ws;
        at[c] = wa;
        cosine[c] = wc;
      }
    }
    if (at[c] == 0x7fffffff) {          // no hit start
      at[c] = -1;
      closing[c] = 0.0;
      cosine[c] = 1.0;
    }
  }
  if (live && kl == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        const size_t i = (size_t)c * a.M + (size_t)m;
        a.commit[i] = commit[c];
        a.first[i] = fm[c];
        a.closing[i] = closing[c];
        a.cosine[i] = cosine[c];
        a.at[i] = at[c];
      }
    const bool finite = a.finite ? a.finite[m] != 0 : true;
    const fo_hidden_impact_t r = fo_hidden_impact_classes_closing<NC>(closing, at, nc, a.rows, finite);
    a.harm[2 * (size_t)m] = r.obst_harm;
    a.harm[2 * (size_t)m + 1] = r.ego_harm;
    a.user[m] = r.user;
    if (a.cost) fo_hidden_impact_fold(r, a.harm_limit, a.cost + (size_t)m * FO_NC, a.safe + m);
  }
}

template <int NC>
void hbil_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeImpactLanesArgs &a, const HbThr &thr) {
  hbu_launch_maps(K, fo_hr_brake_impact_lanes_kernel<NC, 1>, fo_hr_brake_impact_lanes_kernel<NC, 2>, fo_hr_brake_impact_lanes_kernel<NC, 3>,
                  grid, block, lds, s, a, thr);
}

}  // namespace
