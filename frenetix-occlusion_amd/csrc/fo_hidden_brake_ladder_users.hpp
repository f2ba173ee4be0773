// fo_hidden_brake_ladder_users.hpp -- hidden-traffic brake ladder for mixed road users in one walk
// (fo_scene_hidden_brake_ladder_users; DESIGN.md §5.10 "Brake ladder by road users"): per candidate and brake start the gentlest
// deceleration of a ladder of L levels that keeps the moving ego clear of EVERY class of hidden road user, each class held against
// the key map it names.  An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_brake_users.hpp and
// fo_hidden_brake_ladder.hpp (same translation unit, same flags: -ffp-contract=off); it stages with hbu_stage, forms first[c] with
// hbu_first and walks with hbu_walk (fo_hidden_brake_users.hpp, where the bounds reasoning stands).  The home of what the two ladder
// users kernels (this one and fo_hidden_brake_ladder_verdict.hpp) share: the ballot of a round (hblu_ballot) and what a group of
// levels requires (hblu_required).
//
// Inputs are those of fo_hr_brake_users_kernel with the L levels in place of a_brake, and B, the number of brake starts.  The levels
// and the threshold table travel together as ONE kernel argument of FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES (HbluPack: the levels'
// bit patterns in its first 2 L words, the table behind them).  The definition stands in include/fo_hip.h.
//   fo_hr_brake_ladder_users_kernel<NC, NK>  the lanes of fo_hr_brake_ladder_kernel: a lane per (m, b, l), lanes along (b, l) with l
//                        fastest, padded to Lp = the power of two >= L; G = brake_ladder_users_group lanes per trajectory (a power
//                        of two in [Lp, 256]), 256 / G trajectories per workgroup, the same rounds on every lane of the workgroup.
//                        Per lane the walk of fo_hr_brake_users_kernel.  LDS: the six rows and the K qmin rows of each trajectory,
//                        the table, and behind them the commit exchange, one int32 per class and lane of the workgroup (used
//                        where a trajectory has more than a wave).
//                        first[c] is formed by every wave for itself (its lanes split the samples), so that no wave waits for it.
//                        After a round every lane holds its unclear mask (bit c: class c is unclear at this lane's level).  The Lp
//                        lanes of one (m, b) are consecutive lanes of one wave, so ONE wave ballot per class holds the unclear bits of
//                        every level of every (m, b) of the wave; each lane shifts its group's Lp bits down: required is the lowest
//                        clear bit below L, last_unclear the highest set bit -- per class, and of the OR over the classes for
//                        required_all / last_unclear_all.  blocking reads bit required_all - 1 of each class's bits: no shuffle.
//                        (A __shfl_xor minimum / maximum per class costs 2 log2(Lp) shuffles per class and round; a ballot costs one
//                        compare.)  commit[c][l] is a minimum over the lanes with the same l: __shfl_xor within the wave and, where
//                        G = 128, 256, through the exchange.
// The level index is < L.  Every byte of every output handed over is written.
#pragma once
#include "fo_hidden_brake_users.hpp"
#include "fo_hidden_brake_ladder.hpp"

namespace {

// the levels and the table in one argument: words [0, 2 L) are the levels (low word, high word), words [2 L, 2 L + C T) the table
struct HbluPack { int32_t w[FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES / 4]; };

struct HrBrakeLadderUsersArgs {
  int M, T, B, L, C;                    // B brake starts, L levels, C classes
  int Lp, G;                            // lanes per (m, b) and per trajectory: powers of two, L <= Lp <= G <= HB_THREADS
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
  double dt;
  int32_t *required, *last_unclear;     // [C][M][B]
  int32_t *commit;                      // [C][M][L]
  int32_t *first;                       // [C][M]
  int32_t *required_all, *last_unclear_all, *blocking;   // [M][B]
  int32_t *brake_first;                 // [C][M][B][L] or null (the detail: both or neither)
  int32_t *stop;                        // [M][B][L] or null
};
static_assert(sizeof(HrBrakeLadderUsersArgs) + sizeof(HbluPack) <= 4096 && sizeof(HbluPack) == FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES,
              "the arguments, the levels and the table fit the kernel-argument segment");
static_assert(4 * FO_HIDDEN_BRAKE_MAX_TABLE <= FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES && 8 * FO_HIDDEN_BRAKE_MAX_LEVELS <= FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES,
              "a full table alone and a full ladder alone are possible");
static_assert(BRAKE_LADDER_USERS_MAX_ARG_BYTES == FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES && BRAKE_LADDER_USERS_MAX_CLASSES == FO_HIDDEN_BRAKE_MAX_CLASSES,
              "brake_ladder_users_lds_bound speaks of the header's limits");

// This lane's group of Lp lanes within the ballots of its wave, and the levels that exist
struct HbluGroup { int shift; unsigned long long seg_mask, lv_mask; };
__device__ __forceinline__ HbluGroup hblu_group(int lane, int Lp, int L) {
  return HbluGroup{lane & ~(Lp - 1), Lp == 64 ? ~0ull : (1ull << Lp) - 1ull, L == 64 ? ~0ull : (1ull << L) - 1ull};
}

// The ballot of a round, reached by every lane of the wave: um has bit c set where class c is unclear at this lane's (m, b, level).
// ONE wave ballot per class holds the unclear bits of every level of every (m, b) of the wave; segs[c] becomes the Lp bits of this
// lane's group (bit l: class c is unclear at level l), the return value their OR over the classes.
template <int NC>
__device__ __forceinline__ unsigned long long hblu_ballot(unsigned um, const HbluGroup &g, unsigned long long (&segs)[NC]) {
  unsigned long long any = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    segs[c] = (__builtin_amdgcn_ballot_w64((um >> c & 1u) != 0) >> g.shift) & g.seg_mask;
    any |= segs[c];
  }
  return any;
}

// What the group's levels require against all classes: req, the lowest clear level below L (-1: none, or no manoeuvre), and
// at_level, bit c: class c is unclear at the level below the required one (the last one where req < 0; req = 0: nothing blocks)
struct HbluReq { int req; unsigned at_level; };
template <int NC>
__device__ __forceinline__ HbluReq hblu_required(const unsigned long long (&segs)[NC], unsigned long long any, const HbluGroup &g, int L,
                                                 bool man) {
  const unsigned long long clear = ~any & g.lv_mask;
  const int req = man ? __builtin_ffsll((long long)clear) - 1 : -1;
  const int lvl = req < 0 ? L - 1 : req - 1;
  unsigned at_level = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (lvl >= 0 && (segs[c] >> lvl & 1ull)) at_level |= 1u << c;
  return HbluReq{req, at_level};
}

// dynamic LDS: brake_ladder_users_lds_bytes(T, K, C, L, B)
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_ladder_users_kernel(const HrBrakeLadderUsersArgs a, const HbluPack pk) {
  extern __shared__ double hblu_rows[]; // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin per map, thr, the exchange
  const int G = a.G, T = a.T, B = a.B, L = a.L, Lp = a.Lp, nc = a.C, per_block = HB_THREADS / G;
  const int sub = threadIdx.x / G, l = threadIdx.x & (G - 1);
  const int k = l & (Lp - 1), bq = l / Lp, nb = G / Lp;
  const int lane = threadIdx.x & 63;
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = m < a.M, level = k < L;
  int32_t *QM = (int32_t *)(hblu_rows + (size_t)per_block * 6 * T);  // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  int32_t *CM = TH + (size_t)nc * T;                                 // [C][HB_THREADS]
  hbu_stage<NK>(a, hblu_rows, QM, TH, m0, per_block, [&](int t) { return pk.w[2 * L + t]; });
  __syncthreads();
  const double *X = hblu_rows + (size_t)sub * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const double a_brake = level ? __hiloint2double(pk.w[2 * k + 1], pk.w[2 * k]) : 0.0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  const int in_wave = G < 64 ? G : 64;
  int fm[NC];                           // formed by every wave for itself: the lanes a trajectory has in THIS wave split its samples
  hbu_first<NC, NK>(QM + (size_t)sub * T, (size_t)per_block * T, TH, T, Lm, l & (in_wave - 1), in_wave, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  const HbluGroup grp = hblu_group(lane, Lp, L);
  int commit[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) commit[c] = 0x7fffffff;
  for (int b0 = 0; b0 < B; b0 += nb) {  // the same rounds on every lane of the workgroup
    const int b = b0 + bq;
    const bool mine = level && b < B, walk = mine && b < Lm;        // (Lm = 0 on lanes without a trajectory)
    int bf[NC], st = -1;
    unsigned um = 0;                    // bit c: class c is unclear at (m, b, this level)
#pragma unroll
    for (int c = 0; c < NC; ++c) bf[c] = -1;
    if (walk) {
      const double vb = V[b];
      st = hb_stop_sample(vb, a_brake, a.dt, b, Lm);
      hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a_brake, st, mk, sb, bf);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && hb_unclear(fm[c], b, bf[c], st)) {
          commit[c] = commit[c] < b ? commit[c] : b;
          um |= 1u << c;
        }
    }
    unsigned long long segs[NC];
    const unsigned long long any = hblu_ballot<NC>(um, grp, segs);
    const bool row = live && b < B;     // (the Lp lanes of (m, b) agree on it)
    const bool man = b < Lm;            // ... and on whether there is a manoeuvre
    if (row) {
      const size_t mb = (size_t)m * B + b;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && k == (c & (Lp - 1))) {        // the classes' rows are dealt to the lanes of the group
          const unsigned long long clear = ~segs[c] & grp.lv_mask;
          const size_t o = ((size_t)c * a.M + (size_t)m) * B + b;
          a.required[o] = man ? __builtin_ffsll((long long)clear) - 1 : -1;
          a.last_unclear[o] = segs[c] ? 63 - __builtin_clzll(segs[c]) : -1;
        }
      const HbluReq rq = hblu_required<NC>(segs, any, grp, L, man);
      if (k == 0) {
        a.required_all[mb] = rq.req;
        a.last_unclear_all[mb] = any ? 63 - __builtin_clzll(any) : -1;
        a.blocking[mb] = (int32_t)rq.at_level;
      }
      if (a.stop && level) {            // the detail (uniform: both buffers or neither)
        const size_t o = mb * L + k;
        a.stop[o] = st;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < nc) a.brake_first[(size_t)c * a.M * B * L + o] = bf[c];
      }
    }
  }
  // commit[c][m][l]: the minimum over the lanes of the trajectory with this l -- within the wave ...
#pragma unroll
  for (int c = 0; c < NC; ++c) hb_shfl_min(commit[c], Lp, in_wave);
  if (G > 64) {                         // ... and over the G / 64 waves of the trajectory (G is the workgroup's: no lane diverges)
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) CM[c * HB_THREADS + threadIdx.x] = commit[c];
    __syncthreads();
    const int w0 = wave & ~(G / 64 - 1);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc)
        for (int w = 0; w < G / 64; ++w) {
          const int f = CM[c * HB_THREADS + (w0 + w) * 64 + lane];
          commit[c] = commit[c] < f ? commit[c] : f;
        }
  }
  if (live && l < L) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        a.commit[((size_t)c * a.M + (size_t)m) * L + l] = commit[c] == 0x7fffffff ? -1 : commit[c];
        if (l == 0) a.first[(size_t)c * a.M + (size_t)m] = fm[c];
      }
  }
}

template <int NC>
void hblu_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeLadderUsersArgs &a, const HbluPack &pk) {
  hbu_launch_maps(K, fo_hr_brake_ladder_users_kernel<NC, 1>, fo_hr_brake_ladder_users_kernel<NC, 2>, fo_hr_brake_ladder_users_kernel<NC, 3>,
                  grid, block, lds, s, a, pk);
}

}  // namespace
