// fo_hidden_brake_harm_ladder_lanes.hpp -- the hidden-traffic harm ladder by approach angle (fo_scene_hidden_brake_harm_ladder_lanes;
// DESIGN.md §5.10 "Harm ladder by approach angle"): the harm ladder of fo_hidden_brake_harm_ladder.hpp with every lane-bound class
// priced at the worst closing speed the lanes' driving directions allow at the cells where it meets the ego, instead of head-on.  An
// EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_brake_harm_ladder.hpp and
// fo_hidden_brake_impact_lanes.hpp (same translation unit, same flags: -ffp-contract=off); it stages with hbu_stage, forms first[c]
// with hbu_first and walks with hbu_walk, whose hit hook hands it the pose at which a class is first hit; the further scan under a hit
// pose is hbil_moves, the arithmetic of the cosine and the closing speed fo_hidden_approach.hpp's, a harm fo_hidden_impact_logistic's,
// what counts as over and how the curve is kept fo_hidden_harm_ladder.hpp's, the ballot, the group's answers and the key the ladder
// verdict's.  None of them is edited.
//
// Inputs are those of fo_hr_brake_harm_ladder_kernel, and the map's move table [rny][rnx], dir_mask (bit c: class c is lane-bound; the
// host hands over 0 where h >= pi) and cos_h, sin_h.  The definition stands in include/fo_hip.h.
//   fo_hr_brake_harm_ladder_lanes_kernel<NC, NK>  the lanes, the grid, the rounds, the ballot, the key and the curve exchange of
//                        fo_hr_brake_harm_ladder_kernel.  Two facts of the definition shape it:
//                        - a class first hit at a moving pose of the manoeuvre -- and not met by the candidate itself at fm[c] <= b --
//                          is priced INSIDE the hook, on the spot: the scan for the lane-bound classes, cosine, closing speed, one
//                          exponential, the `over` bit and fo_hidden_harm_ladder_take, whose rule does not depend on the order of the
//                          classes.  A lane keeps no per-class closing / cosine / at registers: its state is the harm ladder's (one
//                          mask, one double, one int32).  A class is first hit at most once per manoeuvre, so the further scan runs at
//                          most C times per (m, b, l), and only for lane-bound classes;
//                        - the "met" case depends neither on the level nor on the brake start: ONE harm per class and trajectory
//                          (pose fm[c], speed v[fm[c]]).  Behind hbu_first the lanes of the trajectory split the classes -- the walk's
//                          registers are not live yet -- and leave it in LDS behind the harm ladder's layout
//                          (brake_harm_ladder_lanes_lds_bytes: [per_block][C] float64); a round reads it for the classes with
//                          fm[c] <= b.  It is never formed per (b, l).
// The class a hook or the met case prices is a run-time value: its scalars (threshold row, speed, harm row, move byte) are read at it;
// no register is selected by it.
// Bounds, next to fo_hidden_brake_users.hpp's: the move table is read at (gx, gy) tested against the raster alone, and only for a
// class of dir_mask -- with dir_mask = 0 it may be null; speed_of and the rows are read at c < C; the met harms are written and read
// at (trajectory of the workgroup < per_block, c < C) alone.  Every byte of every output is written; of cost and safe only what the
// definition names.  Plain vector stores, no atomics.
#pragma once
#include "fo_hidden_brake_harm_ladder.hpp"
#include "fo_hidden_brake_impact_lanes.hpp"

namespace {

struct HrBrakeHarmLadderLanesArgs {
  int M, T, B, L, C;                    // as HrBrakeHarmLadderArgs
  int Lp, G, P;
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
  double dt, a_limit;
  const double *speed_of, *rows;        // [C], [C][4]
  double harm_limit;
  const uint8_t *moves;                 // [rny][rnx] the map's move table; may be null with dir_mask = 0
  uint32_t dir_mask;                    // bit c: class c is lane-bound
  double cos_h, sin_h;
  const uint8_t *finite;
  double *cost;
  uint8_t *safe;
  int32_t *need, *at, *blocking, *user; // [M]
  double *decel;                        // [M]
  int32_t *need_of, *first;             // [C][M]
  double *harm_at;                      // [M][L]
  int32_t *user_at;                     // [M][L]
};
static_assert(sizeof(HrBrakeHarmLadderLanesArgs) + sizeof(HbluPack) <= 4096, "the arguments, the levels and the table fit the kernel-argument segment");

// dynamic LDS: brake_harm_ladder_lanes_lds_bytes(T, K, C, L, B).  The waves-per-SIMD hint is the head-on sibling's (DESIGN.md §5.10
// "Harm ladder by approach angle", the kernel table)
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) __attribute__((amdgpu_waves_per_eu(NC == 4 ? 4 : 3))) void fo_hr_brake_harm_ladder_lanes_kernel(const HrBrakeHarmLadderLanesArgs a, const HbluPack pk) {
  extern __shared__ double hbll_rows[]; // the harm ladder's layout; behind it the met harms [per_block][C]
  const int G = a.G, T = a.T, B = a.B, L = a.L, Lp = a.Lp, nc = a.C, per_block = a.P;
  const int sub = threadIdx.x / G, l = threadIdx.x & (G - 1);
  const int k = l & (Lp - 1), bq = l / Lp, nb = G / Lp;
  const int lane = threadIdx.x & 63;
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = sub < per_block && m < a.M, level = k < L;
  int32_t *QM = (int32_t *)(hbll_rows + (size_t)per_block * 6 * T);  // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  int32_t *EX = TH + (size_t)nc * T;                                 // [C + 1][BRAKE_LADDER_VERDICT_WAVES]
  const size_t ex_end = (size_t)(EX - (int32_t *)hbll_rows) + (size_t)(nc + 1) * BRAKE_LADDER_VERDICT_WAVES;     // in int32
  // behind the exchange, where G > 64, the curve's: [HB_THREADS] harm, [HB_THREADS] class (8-byte aligned); then the met harms
  double *MH = hbll_rows + (ex_end + 1) / 2 + (G > 64 ? HB_THREADS + HB_THREADS / 2 : 0);       // [per_block][C]
  hbu_stage<NK>(a, hbll_rows, QM, TH, m0, per_block, [&](int t) { return pk.w[2 * L + t]; });
  __syncthreads();
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hbll_rows + (size_t)row_of * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const double a_brake = level ? __hiloint2double(pk.w[2 * k + 1], pk.w[2 * k]) : 0.0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  const int in_wave = G < 64 ? G : 64;
  int fm[NC];                           // formed by every wave for itself, as in the ladder verdict
  hbu_first<NC, NK>(QM + (size_t)row_of * T, (size_t)per_block * T, TH, T, Lm, l & (in_wave - 1), in_wave, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  const int ends = B < Lm ? B : Lm;     // brake starts with a manoeuvre (Lm = 0 on lanes without a trajectory)
  // the met case: every start b in [fm[c], ends) at every level meets class c at the candidate's own pose fm[c] at v[fm[c]] -- one
  // harm; the lanes of the trajectory split the classes (fm[c] = -1 on lanes without a trajectory: they write nothing)
  for (int c = l; c < nc; c += G) {
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
      MH[(size_t)sub * nc + c] = fo_hidden_impact_logistic(a.rows[4 * c], a.rows[4 * c + 1], w);
    }
  }
  __syncthreads();
  const double *mh = MH + (size_t)row_of * nc;
  const HbluGroup grp = hblu_group(lane, Lp, L);
  int32_t key = FO_HIDDEN_LADDER_NO_KEY, need_of[NC];
  fo_hidden_harm_ladder_best_t best = fo_hidden_harm_ladder_none();   // of this lane's level, over its brake starts
#pragma unroll
  for (int c = 0; c < NC; ++c) need_of[c] = -1;
  for (int b0 = 0; b0 < B; b0 += nb) {  // the same rounds on every lane of the workgroup
    const int b = b0 + bq;
    const bool walk = level && b < ends;
    unsigned um = 0;                    // bit c: class c hits (m, b, this level) at a harm over the limit
    if (walk) {
      int bf[NC];
      const double vb = V[b];
      const int st = hb_stop_sample(vb, a_brake, a.dt, b, Lm);
      unsigned met = 0;                 // the classes the candidate itself meets no later than b: their harm stands in LDS
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (fm[c] >= 0 && fm[c] <= b) met |= 1u << c;
      // a hit the hook sees is a hit of the definition: a moving pose, 0 <= bf[c] = i < st
      hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a_brake, st, mk, sb, bf, [&](int i, const HbPose &p, unsigned h) {
        const unsigned hn = h & ~met;
        if (!hn) return;
        const unsigned hd = hn & a.dir_mask;
        const uint64_t mv = hd ? hbil_moves<NC, NK>(a, TH, i, p.x, p.y, p.c, p.s, hd, mk, sb) : 0;
        const double u = hb_speed(vb, a_brake, a.dt, i, b);          // positive: i < st
        for (unsigned r = hn; r; r &= r - 1u) {
          const int c = __builtin_ctz(r);
          const double cm = fo_hidden_approach_cosine((unsigned)(mv >> (8 * c)) & 0xffu, (hd >> c & 1u) != 0, p.c, p.s, a.cos_h, a.sin_h);
          const double w = fo_hidden_approach_closing(u, a.speed_of[c], cm);
          const double ho = fo_hidden_impact_logistic(a.rows[4 * c], a.rows[4 * c + 1], w);
          if (fo_hidden_harm_ladder_over(true, ho, a.harm_limit)) um |= 1u << c;
          fo_hidden_harm_ladder_take(best, ho, c);
        }
      });
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (met >> c & 1u) {            // (met is empty beyond C: fm[c] = -1 there)
          const double ho = mh[c];
          if (fo_hidden_harm_ladder_over(true, ho, a.harm_limit)) um |= 1u << c;
          fo_hidden_harm_ladder_take(best, ho, c);
        }
    }
    unsigned long long segs[NC];
    const unsigned long long any = hblu_ballot<NC>(um, grp, segs);
    if (b < ends) {                     // (the Lp lanes of (m, b) agree on it, and on everything below)
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) {
          const unsigned long long clear = ~segs[c] & grp.lv_mask;
          need_of[c] = fo_hidden_ladder_max(need_of[c], fo_hidden_ladder_rank(__builtin_ffsll((long long)clear) - 1, L));
        }
      const HbluReq rq = hblu_required<NC>(segs, any, grp, L, true);
      key = fo_hidden_ladder_max(key, fo_hidden_ladder_key(fo_hidden_ladder_rank(rq.req, L), b, (int32_t)rq.at_level));
    }
  }
  // the maxima over the lanes of the trajectory (the curve's: over those of equal level) -- within the wave ...
  for (int o = in_wave >> 1; o >= Lp; o >>= 1) {
    key = fo_hidden_ladder_max(key, __shfl_xor(key, o));
    const double wh = __shfl_xor(best.harm, o);
    const int32_t wc = __shfl_xor(best.cls, o);
    fo_hidden_harm_ladder_take(best, wh, wc);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    for (int o = in_wave >> 1; o >= Lp; o >>= 1) need_of[c] = fo_hidden_ladder_max(need_of[c], __shfl_xor(need_of[c], o));
  if (G > 64) {                         // ... and over the G / 64 waves of the trajectory (G is the workgroup's: no lane diverges)
    // (the lane's index, formed anew: left to itself the compiler keeps the staging loop's multiple of threadIdx.x alive over all
    // rounds for these two stores, and at width 4, NK >= 2 that one value goes to scratch under the 4-wave hint)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int wave = tid >> 6;
    double *HX = hbll_rows + (ex_end + 1) / 2;                       // [HB_THREADS] harm
    int32_t *HC = (int32_t *)(HX + HB_THREADS);                      // [HB_THREADS] class
    HX[tid] = best.harm;
    HC[tid] = best.cls;
    if (lane == 0) {
      EX[wave] = key;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) EX[(c + 1) * BRAKE_LADDER_VERDICT_WAVES + wave] = need_of[c];
    }
    __syncthreads();
    const int w0 = wave & ~(G / 64 - 1);
    for (int w = 0; w < G / 64; ++w) {
      key = fo_hidden_ladder_max(key, EX[w0 + w]);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) need_of[c] = fo_hidden_ladder_max(need_of[c], EX[(c + 1) * BRAKE_LADDER_VERDICT_WAVES + w0 + w]);
      fo_hidden_harm_ladder_take(best, HX[(w0 + w) * 64 + lane], HC[(w0 + w) * 64 + lane]);
    }
  }
  const bool finite = live && a.finite ? a.finite[m] != 0 : true;
  if (live && bq == 0 && level) {       // the curve: one lane per level
    double h;
    int32_t u;
    fo_hidden_harm_ladder_curve(best, finite, &h, &u);
    a.harm_at[(size_t)m * L + k] = h;
    a.user_at[(size_t)m * L + k] = u;
  }
  if (live && l == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        a.need_of[(size_t)c * a.M + (size_t)m] = need_of[c];
        a.first[(size_t)c * a.M + (size_t)m] = fm[c];
      }
    fo_hidden_ladder_verdict_t r = fo_hidden_ladder_verdict_of(key, L, finite);
    const int nl = r.need >= 0 && r.need < L ? r.need : 0;          // (the level index stays < L)
    r.decel = fo_hidden_ladder_decel(r.need, L, __hiloint2double(pk.w[2 * nl + 1], pk.w[2 * nl]));
    a.need[m] = r.need;
    a.at[m] = r.at;
    a.blocking[m] = r.blocking;
    a.user[m] = r.user;
    a.decel[m] = r.decel;
    if (a.cost) fo_hidden_ladder_verdict_fold(r, L, a.a_limit, a.cost + (size_t)m * FO_NC, a.safe + m);
  }
}

template <int NC>
void hbll_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeHarmLadderLanesArgs &a, const HbluPack &pk) {
  hbu_launch_maps(K, fo_hr_brake_harm_ladder_lanes_kernel<NC, 1>, fo_hr_brake_harm_ladder_lanes_kernel<NC, 2>,
                  fo_hr_brake_harm_ladder_lanes_kernel<NC, 3>, grid, block, lds, s, a, pk);
}

}  // namespace
