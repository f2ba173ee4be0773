// fo_hidden_brake_ladder_verdict.hpp -- the hidden-traffic ladder verdict (fo_scene_hidden_brake_ladder_verdict; DESIGN.md §5.10
// "Ladder verdict"): the deceleration each candidate needs, from the worst of the brake starts up to the replanning interval, to stay
// clear of every class of hidden road user -- folded into the two reserved columns of the planning step's cost row and its safety
// flag.  An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_brake_ladder_users.hpp and
// fo_hidden_brake_verdict.hpp (same translation unit, same flags: -ffp-contract=off); it stages with hbu_stage, forms first[c] with
// hbu_first and walks with hbu_walk (fo_hidden_brake_users.hpp, where the bounds reasoning stands), forms a round's answers with
// hblu_ballot and hblu_required (fo_hidden_brake_ladder_users.hpp) and takes the levels and the table as the HbluPack argument.
// What the groups' answers mean per trajectory is fo_hidden_ladder_verdict.hpp's.
//
// Inputs are those of fo_hr_brake_ladder_users_kernel, a_limit, finite [M] and the cost / safe pair.  The definition stands in
// include/fo_hip.h.
//   fo_hr_brake_ladder_verdict_kernel<NC, NK>  the lanes of fo_hr_brake_ladder_users_kernel -- a lane per (m, b, l), l fastest, padded
//                        to Lp; G = brake_ladder_verdict_group(L, B) lanes per trajectory (a power of two in [Lp, 256]), the same
//                        rounds over b on every lane of the workgroup -- with the trajectories per workgroup of
//                        fo_hr_brake_verdict_kernel: P = brake_ladder_verdict_per_block, capped by LDS, so the lanes from P * G on
//                        stage rows and then have no trajectory.  LDS: the six rows and the K qmin rows of each trajectory, the
//                        table, and behind them the exchange (brake_ladder_verdict_lds_bytes).  first[c] is formed by every wave for
//                        itself, as in the ladder-users kernel.  After a round ONE wave ballot per class holds the unclear bits of
//                        every level of every (m, b) of the wave; every lane of a group shifts its group's Lp bits down and forms
//                        the group's rank, blocking mask and per-class ranks (the lanes of a group agree: no lane is singled out).
//                        Across the rounds a lane keeps the maximum of its groups' keys and per-class ranks; at the end the
//                        maximum over the lanes of the trajectory: __shfl_xor within the wave and, where G = 128, 256, one int32
//                        per wave through the exchange.  Lane 0 of each trajectory writes the outputs and folds the row.
// No [M][B] or [M][B][L] buffer exists.  The level index is < L, finite is read at m < M alone.  Every byte of every output is
// written; of cost and safe only what the definition names.
#pragma once
#include "fo_hidden_brake_ladder_users.hpp"
#include "fo_hidden_ladder_verdict.hpp"

namespace {

struct HrBrakeLadderVerdictArgs {
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
  const uint8_t *finite;                // [M] or null (every candidate counts as finite)
  double *cost;                         // [M][FO_NC] or null (both or neither)
  uint8_t *safe;                        // [M] or null
  int32_t *need, *at, *blocking, *user; // [M]
  double *decel;                        // [M]
  int32_t *need_of, *first;             // [C][M]
};
static_assert(sizeof(HrBrakeLadderVerdictArgs) + sizeof(HbluPack) <= 4096, "the arguments, the levels and the table fit the kernel-argument segment");
static_assert(FO_HIDDEN_BRAKE_MAX_LEVELS <= 64 && HR_MAX_J <= 254 && FO_HIDDEN_BRAKE_MAX_CLASSES <= 8, "rank, 255 - b and blocking fit the key");

// dynamic LDS: brake_ladder_verdict_lds_bytes(T, K, C, L, B)
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_ladder_verdict_kernel(const HrBrakeLadderVerdictArgs a, const HbluPack pk) {
  extern __shared__ double hblv_rows[]; // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin per map, thr, the exchange
  const int G = a.G, T = a.T, B = a.B, L = a.L, Lp = a.Lp, nc = a.C, per_block = a.P;
  const int sub = threadIdx.x / G, l = threadIdx.x & (G - 1);
  const int k = l & (Lp - 1), bq = l / Lp, nb = G / Lp;
  const int lane = threadIdx.x & 63;
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = sub < per_block && m < a.M, level = k < L;
  int32_t *QM = (int32_t *)(hblv_rows + (size_t)per_block * 6 * T);  // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  int32_t *EX = TH + (size_t)nc * T;                                 // [C + 1][BRAKE_LADDER_VERDICT_WAVES]
  hbu_stage<NK>(a, hblv_rows, QM, TH, m0, per_block, [&](int t) { return pk.w[2 * L + t]; });
  __syncthreads();
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hblv_rows + (size_t)row_of * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const double a_brake = level ? __hiloint2double(pk.w[2 * k + 1], pk.w[2 * k]) : 0.0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  const int in_wave = G < 64 ? G : 64;
  int fm[NC];                           // formed by every wave for itself, as in the ladder-users kernel
  hbu_first<NC, NK>(QM + (size_t)row_of * T, (size_t)per_block * T, TH, T, Lm, l & (in_wave - 1), in_wave, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  const HbluGroup grp = hblu_group(lane, Lp, L);
  const int ends = B < Lm ? B : Lm;     // brake starts with a manoeuvre (Lm = 0 on lanes without a trajectory)
  int32_t key = FO_HIDDEN_LADDER_NO_KEY, need_of[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) need_of[c] = -1;
  for (int b0 = 0; b0 < B; b0 += nb) {  // the same rounds on every lane of the workgroup
    const int b = b0 + bq;
    const bool walk = level && b < ends;
    unsigned um = 0;                    // bit c: class c is unclear at (m, b, this level)
    if (walk) {
      int bf[NC];
      const double vb = V[b];
      const int st = hb_stop_sample(vb, a_brake, a.dt, b, Lm);
      hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a_brake, st, mk, sb, bf);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && hb_unclear(fm[c], b, bf[c], st)) um |= 1u << c;
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
  // the maximum over the lanes of the trajectory -- within the wave ...
  for (int o = in_wave >> 1; o >= Lp; o >>= 1) key = fo_hidden_ladder_max(key, __shfl_xor(key, o));
#pragma unroll
  for (int c = 0; c < NC; ++c)
    for (int o = in_wave >> 1; o >= Lp; o >>= 1) need_of[c] = fo_hidden_ladder_max(need_of[c], __shfl_xor(need_of[c], o));
  if (G > 64) {                         // ... and over the G / 64 waves of the trajectory (G is the workgroup's: no lane diverges)
    const int wave = threadIdx.x >> 6;
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
    }
  }
  if (live && l == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        a.need_of[(size_t)c * a.M + (size_t)m] = need_of[c];
        a.first[(size_t)c * a.M + (size_t)m] = fm[c];
      }
    const bool finite = a.finite ? a.finite[m] != 0 : true;
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
void hblv_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeLadderVerdictArgs &a, const HbluPack &pk) {
  hbu_launch_maps(K, fo_hr_brake_ladder_verdict_kernel<NC, 1>, fo_hr_brake_ladder_verdict_kernel<NC, 2>, fo_hr_brake_ladder_verdict_kernel<NC, 3>,
                  grid, block, lds, s, a, pk);
}

}  // namespace
