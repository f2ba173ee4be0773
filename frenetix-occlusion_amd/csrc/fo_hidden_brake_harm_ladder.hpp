// fo_hidden_brake_harm_ladder.hpp -- the hidden-traffic harm ladder (fo_scene_hidden_brake_harm_ladder; DESIGN.md §5.10 "Harm
// ladder"): the deceleration each candidate must be prepared for, from the worst of the brake starts up to the replanning interval, so
// that the harm of what still hits it stays within a limit -- the ladder verdict with "unclear" relaxed to "hit at a harm above
// harm_limit" -- and, per level, the greatest harm that level leaves.  An EXTENSION, not part of the reference.  Included by
// fo_scene.hip after fo_hidden_brake_ladder_verdict.hpp and fo_hidden_brake_impact.hpp (same translation unit, same flags:
// -ffp-contract=off); it stages with hbu_stage, forms first[c] with hbu_first and walks with hbu_walk (fo_hidden_brake_users.hpp,
// where the bounds reasoning stands), forms a round's answers with hblu_ballot and hblu_required and reduces with the ladder
// verdict's key (fo_hidden_ladder_verdict.hpp); a harm is fo_hidden_impact_logistic's, what counts as over and how the curve is kept
// is fo_hidden_harm_ladder.hpp's.
//
// Inputs are those of fo_hr_brake_ladder_verdict_kernel, and harm_limit, rows [C][4] and speed_of [C] (device buffers: the host
// builds them once per set of users).  The definition stands in include/fo_hip.h.
//   fo_hr_brake_harm_ladder_kernel<NC, NK>  the lanes, the grid and the rounds of fo_hr_brake_ladder_verdict_kernel
//                        (brake_ladder_verdict_group / _per_block / _blocks).  After its walk a lane prices the classes that hit it
//                        on the spot -- the ego speed at the hit as in fo_hr_brake_impact_kernel, one exponential per hit class --
//                        sets the class's bit where the harm is over the limit, and keeps the greatest harm of its level and the
//                        lowest class attaining it (one double, one int32).  The ballot, the group's answers and the key maximum
//                        are the ladder verdict's on that mask.  The curve is a maximum over the lanes of equal level: __shfl_xor
//                        at offsets >= Lp within the wave and, where G = 128, 256, one pair per lane of the workgroup through the
//                        exchange behind the ladder verdict's (brake_harm_ladder_lds_bytes).  The lanes bq == 0 write harm_at /
//                        user_at, lane 0 of each trajectory the rest, and folds the row.
// rows and speed_of are read at c < C alone, finite at m < M.  Every byte of every output is written; of cost and safe only what the
// definition names.
#pragma once
#include "fo_hidden_brake_ladder_verdict.hpp"
#include "fo_hidden_impact.hpp"
#include "fo_hidden_harm_ladder.hpp"

namespace {

struct HrBrakeHarmLadderArgs {
  int M, T, B, L, C;                    // B brake starts, L levels, C classes
  int Lp, G, P;                         // lanes per (m, b) and per trajectory: powers of two, L <= Lp <= G <= HB_THREADS; P trajectories per workgroup
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  const int32_t *len;                   // [M] or null
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;                 // the window
  const int32_t *key0, *key1, *key2;    // [ny][nx] each; those beyond K are null and never read (named members: see HrBrakeUsersArgs)
  const int32_t *qmin0, *qmin1, *qmin2; // [M][T] each
  uint32_t map_of;                      // hbu_map_of
  const double *v, *arc;                // [M][T]
  double dt, a_limit;
  const double *speed_of, *rows;        // [C], [C][4]
  double harm_limit;
  const uint8_t *finite;                // [M] or null (every candidate counts as finite)
  double *cost;                         // [M][FO_NC] or null (both or neither)
  uint8_t *safe;                        // [M] or null
  int32_t *need, *at, *blocking, *user; // [M]
  double *decel;                        // [M]
  int32_t *need_of, *first;             // [C][M]
  double *harm_at;                      // [M][L]
  int32_t *user_at;                     // [M][L]
};
static_assert(sizeof(HrBrakeHarmLadderArgs) + sizeof(HbluPack) <= 4096, "the arguments, the levels and the table fit the kernel-argument segment");

// dynamic LDS: brake_harm_ladder_lds_bytes(T, K, C, L, B).  The waves-per-SIMD hint: left to itself the allocator takes 131 - 134
// registers at width 4, one granule above the ladder verdict's 4 waves per SIMD; asked for 4 it stays within 128 without a private
// segment.  At width 8 (154 - 156 registers, 3 waves) the same request spills 11 - 13 registers to scratch: it keeps 3 (DESIGN.md
// §5.10 "Harm ladder", the kernel table).
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) __attribute__((amdgpu_waves_per_eu(NC == 4 ? 4 : 3))) void fo_hr_brake_harm_ladder_kernel(const HrBrakeHarmLadderArgs a, const HbluPack pk) {
  extern __shared__ double hbhl_rows[]; // the ladder verdict's layout; behind its exchange, where G > 64, the curve's (8-byte aligned)
  const int G = a.G, T = a.T, B = a.B, L = a.L, Lp = a.Lp, nc = a.C, per_block = a.P;
  const int sub = threadIdx.x / G, l = threadIdx.x & (G - 1);
  const int k = l & (Lp - 1), bq = l / Lp, nb = G / Lp;
  const int lane = threadIdx.x & 63;
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = sub < per_block && m < a.M, level = k < L;
  int32_t *QM = (int32_t *)(hbhl_rows + (size_t)per_block * 6 * T);  // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  int32_t *EX = TH + (size_t)nc * T;                                 // [C + 1][BRAKE_LADDER_VERDICT_WAVES]
  hbu_stage<NK>(a, hbhl_rows, QM, TH, m0, per_block, [&](int t) { return pk.w[2 * L + t]; });
  __syncthreads();
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hbhl_rows + (size_t)row_of * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const double a_brake = level ? __hiloint2double(pk.w[2 * k + 1], pk.w[2 * k]) : 0.0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  const int in_wave = G < 64 ? G : 64;
  int fm[NC];                           // formed by every wave for itself, as in the ladder verdict
  hbu_first<NC, NK>(QM + (size_t)row_of * T, (size_t)per_block * T, TH, T, Lm, l & (in_wave - 1), in_wave, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  const HbluGroup grp = hblu_group(lane, Lp, L);
  const int ends = B < Lm ? B : Lm;     // brake starts with a manoeuvre (Lm = 0 on lanes without a trajectory)
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
      hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a_brake, st, mk, sb, bf);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && hb_unclear(fm[c], b, bf[c], st)) {
          // the candidate itself is met at fm[c] <= b, before braking from b changes anything; else the manoeuvre's speed at its hit
          const bool met = fm[c] >= 0 && fm[c] <= b;
          const double u = met ? V[fm[c] < 0 ? 0 : fm[c]] : hb_speed(vb, a_brake, a.dt, bf[c], b);
          const double ho = fo_hidden_impact_logistic(a.rows[4 * c], a.rows[4 * c + 1], u + a.speed_of[c]);
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
    const int wave = threadIdx.x >> 6;
    const size_t ex_end = (size_t)(EX - (int32_t *)hbhl_rows) + (size_t)(nc + 1) * BRAKE_LADDER_VERDICT_WAVES;   // in int32
    double *HX = hbhl_rows + (ex_end + 1) / 2;                       // [HB_THREADS] harm
    int32_t *HC = (int32_t *)(HX + HB_THREADS);                      // [HB_THREADS] class
    HX[threadIdx.x] = best.harm;
    HC[threadIdx.x] = best.cls;
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
void hbhl_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeHarmLadderArgs &a, const HbluPack &pk) {
  hbu_launch_maps(K, fo_hr_brake_harm_ladder_kernel<NC, 1>, fo_hr_brake_harm_ladder_kernel<NC, 2>, fo_hr_brake_harm_ladder_kernel<NC, 3>,
                  grid, block, lds, s, a, pk);
}

}  // namespace
