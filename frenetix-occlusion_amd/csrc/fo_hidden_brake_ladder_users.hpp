// fo_hidden_brake_ladder_users.hpp -- hidden-traffic brake ladder for mixed road users in one walk
// (fo_scene_hidden_brake_ladder_users; DESIGN.md §5.10 "Brake ladder by road users"): per candidate and brake start the gentlest
// deceleration of a ladder of L levels that keeps the moving ego clear of EVERY class of hidden road user, each class held against
// the key map it names.  An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_brake_users.hpp and
// fo_hidden_brake_ladder.hpp (same translation unit, same flags: -ffp-contract=off); it walks with hb_speed and hb_pose_step, scans
// with fo_hr_scan_pose_rows and decides with HbuKeys / hbu_hits, all unchanged: the arithmetic of a manoeuvre exists once.
//
// Inputs are those of fo_hr_brake_users_kernel with the L levels in place of a_brake, and B, the number of brake starts.  The levels
// and the threshold table travel together as ONE kernel argument of FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES (HbluPack: the levels'
// bit patterns in its first 2 L words, the table behind them).  The definition stands in include/fo_hip.h.
//   fo_hr_brake_ladder_users_kernel<NC, NK>  the lanes of fo_hr_brake_ladder_kernel: a lane per (m, b, l), lanes along (b, l) with l
//                        fastest, padded to Lp = the power of two >= L; G = brake_ladder_users_group lanes per trajectory (a power
//                        of two in [Lp, 256]), 256 / G trajectories per workgroup, the same rounds on every lane of the workgroup.
//                        Per lane the state of fo_hr_brake_users_kernel: one scan per braking pose over map 0 whose callback reads the
//                        other maps that still have an open class, the walk ends when every class has its hit or at the standing
//                        pose.  LDS: the six rows and the K qmin rows of each trajectory, the table, and behind them the commit
//                        exchange, one int32 per class and lane of the workgroup (used where a trajectory has more than a wave).
//                        first[c] is formed by every wave for itself (its lanes split the samples), so that no wave waits for it.
//                        After a round every lane holds its unclear mask (bit c: class c is unclear at this lane's level).  The Lp
//                        lanes of one (m, b) are consecutive lanes of one wave, so ONE wave ballot per class holds the unclear bits of
//                        every level of every (m, b) of the wave; each lane shifts its group's Lp bits down: required is the lowest
//                        clear bit below L, last_unclear the highest set bit -- per class, and of the OR over the classes for
//                        required_all / last_unclear_all.  blocking reads bit required_all - 1 of each class's bits: no shuffle.
//                        (A __shfl_xor minimum / maximum per class costs 2 log2(Lp) shuffles per class and round; a ballot costs one
//                        compare.)  commit[c][l] is a minimum over the lanes with the same l: __shfl_xor within the wave and, where
//                        G = 128, 256, through the exchange.
// The key maps are read through the caches and never written, so two of them may be the same buffer.  Every LDS index is clamped to
// [0, Lm) or bounded by c < C, the level index is < L, and a map is read only at a window index that was tested against the window:
// no content of v, arc, the keys, qmin, thr, map_of or the levels can make a lane read out of range.  No atomics, no scratch, plain
// vector stores; every byte of every output handed over is written.
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
  for (int t = threadIdx.x; t < per_block * T; t += HB_THREADS) {
    const int su = t / T, ks = t - su * T;
    if (m0 + su < a.M) {
      const size_t i = (size_t)(m0 + su) * T + ks;
      double *row = hblu_rows + (size_t)su * 6 * T + ks;
      row[0] = a.x[i];
      row[T] = a.y[i];
      row[2 * T] = a.heading[2 * i];
      row[3 * T] = a.heading[2 * i + 1];
      row[4 * T] = a.arc[i];
      row[5 * T] = a.v[i];
      QM[t] = a.qmin0[i];
      if constexpr (NK > 1) QM[(size_t)per_block * T + t] = a.qmin1[i];
      if constexpr (NK > 2) QM[(size_t)2 * per_block * T + t] = a.qmin2[i];
    }
  }
  for (int t = threadIdx.x; t < nc * T; t += HB_THREADS) TH[t] = pk.w[2 * L + t];   // (4 C T + 8 L <= the argument's bytes: the host's refusal)
  __syncthreads();
  const double *X = hblu_rows + (size_t)sub * 6 * T, *Y = X + T, *C = Y + T, *S = C + T, *ARC = S + T, *V = ARC + T;
  const int32_t *Q = QM + (size_t)sub * T;          // map k2: Q[k2 * per_block * T + j]
  int Lm = 0;
  if (live) {
    Lm = T;
    if (a.len) { const int ln = a.len[m]; Lm = ln < 0 ? 0 : (ln < T ? ln : T); }
  }
  const double a_brake = level ? __hiloint2double(pk.w[2 * k + 1], pk.w[2 * k]) : 0.0;
  const unsigned every = (1u << nc) - 1u;           // bit c: class c is there (c < C); in the walk: it has no first hit yet
  unsigned cm1 = 0, cm2 = 0;                        // bit c: class c is held against map 1 / map 2
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int mo = hbu_map_of(a.map_of, c);
    if (c < nc && mo == 1) cm1 |= 1u << c;
    if (c < nc && mo == 2) cm2 |= 1u << c;
  }
  // first[c] = min { j < Lm : qmin_map_of[c][m][j] <= thr[c][j] }: the lanes a trajectory has in THIS wave split its samples
  const int in_wave = G < 64 ? G : 64;
  int fm[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) fm[c] = 0x7fffffff;
  for (int j = l & (in_wave - 1); j < Lm; j += in_wave) {
    HbuKeys q{Q[j], 0, 0};
    if constexpr (NK > 1) q.q1 = Q[(size_t)per_block * T + j];
    if constexpr (NK > 2) q.q2 = Q[(size_t)2 * per_block * T + j];
    const unsigned h = hbu_hits<NC, NK>(q, TH, T, j, every, cm1, cm2);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (h >> c & 1u) fm[c] = fm[c] < j ? fm[c] : j;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    for (int o = in_wave >> 1; o > 0; o >>= 1) {
      const int f = __shfl_xor(fm[c], o);
      fm[c] = fm[c] < f ? fm[c] : f;
    }
    if (fm[c] == 0x7fffffff) fm[c] = -1;
  }
  // cells beyond the raster and the window have no key: the scan never leaves their union
  const int lox = a.ix0 < 0 ? a.ix0 : 0, loy = a.iy0 < 0 ? a.iy0 : 0;
  const int hix = (a.ix0 + a.nx > a.rnx ? a.ix0 + a.nx : a.rnx) - 1, hiy = (a.iy0 + a.ny > a.rny ? a.iy0 + a.ny : a.rny) - 1;
  // this lane's group of Lp lanes within the ballot of its wave, and the levels that exist
  const int seg_shift = lane & ~(Lp - 1);
  const unsigned long long seg_mask = Lp == 64 ? ~0ull : (1ull << Lp) - 1ull, lv_mask = L == 64 ? ~0ull : (1ull << L) - 1ull;
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
      const int last = Lm - 1;
      const double vb = V[b], arc_end = ARC[last];
      st = Lm;
      for (int i = b; i < Lm; ++i)
        if (hb_speed(vb, a_brake, a.dt, i, b) == 0.0) { st = i; break; }
      double s = ARC[b];
      int j = 0;
      unsigned open = every;
      for (int i = b + 1; i < Lm; ++i) {
        const HbPose p = hb_pose_step(X, Y, C, S, ARC, Lm, last, arc_end, vb, a_brake, a.dt, i, b, s, j);
        const bool open1 = (open & cm1) != 0, open2 = (open & cm2) != 0;   // maps 1, 2 still have an open class (map 0 is the scan's own)
        HbuKeys q{HC_NONE, HC_NONE, HC_NONE};
        fo_hr_scan_pose_rows(a, p.x, p.y, p.c, p.s, a.key0, HC_NONE, lox, loy, hix, hiy, 0, 1, [&](int kv, int gx, int gy) {
          q.q0 = q.q0 < kv ? q.q0 : kv;
          if constexpr (NK > 1) {
            const int wx = gx - a.ix0, wy = gy - a.iy0;
            const bool in = wx >= 0 && wx < a.nx && wy >= 0 && wy < a.ny;
            if (open1) {
              const int vk = in ? a.key1[wy * a.nx + wx] : kv;      // outside the window: 0 or NONE, the same for every map
              q.q1 = q.q1 < vk ? q.q1 : vk;
            }
            if constexpr (NK > 2) {
              if (open2) {
                const int vk = in ? a.key2[wy * a.nx + wx] : kv;
                q.q2 = q.q2 < vk ? q.q2 : vk;
              }
            }
          }
        });
        if (i >= st) {                  // the ego stands: this pose is the manoeuvre's last one, hit_c(i') for i' >= i iff q <= thr[c][i']
          for (int at = i; at <= last && open; ++at) {
            const unsigned h = hbu_hits<NC, NK>(q, TH, T, at, open, cm1, cm2);
#pragma unroll
            for (int c = 0; c < NC; ++c)
              if (h >> c & 1u) bf[c] = at;
            open &= ~h;
          }
          break;
        }
        const unsigned h = hbu_hits<NC, NK>(q, TH, T, i, open, cm1, cm2);
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (h >> c & 1u) bf[c] = i;
        open &= ~h;
        if (!open) break;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && ((fm[c] >= 0 && fm[c] <= b) || (bf[c] >= 0 && bf[c] < st))) {
          commit[c] = commit[c] < b ? commit[c] : b;
          um |= 1u << c;
        }
    }
    // every lane of the wave is here: one ballot per class holds the unclear bits of all its (m, b) groups
    unsigned long long any = 0;
    unsigned at_level = 0;              // bit c: class c is unclear at the level asked of it below (required_all - 1)
    unsigned long long segs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      segs[c] = (__builtin_amdgcn_ballot_w64((um >> c & 1u) != 0) >> seg_shift) & seg_mask;
      any |= segs[c];
    }
    const bool row = live && b < B;     // (the Lp lanes of (m, b) agree on it)
    const bool man = b < Lm;            // ... and on whether there is a manoeuvre
    if (row) {
      const size_t mb = (size_t)m * B + b;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && k == (c & (Lp - 1))) {        // the classes' rows are dealt to the lanes of the group
          const unsigned long long clear = ~segs[c] & lv_mask;
          const size_t o = ((size_t)c * a.M + (size_t)m) * B + b;
          a.required[o] = man ? __builtin_ffsll((long long)clear) - 1 : -1;
          a.last_unclear[o] = segs[c] ? 63 - __builtin_clzll(segs[c]) : -1;
        }
      const unsigned long long clear = ~any & lv_mask;
      const int req = man ? __builtin_ffsll((long long)clear) - 1 : -1;
      const int lvl = req < 0 ? L - 1 : req - 1;    // (req = 0: -1, nothing blocks)
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (lvl >= 0 && (segs[c] >> lvl & 1ull)) at_level |= 1u << c;
      if (k == 0) {
        a.required_all[mb] = req;
        a.last_unclear_all[mb] = any ? 63 - __builtin_clzll(any) : -1;
        a.blocking[mb] = (int32_t)at_level;
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
  for (int c = 0; c < NC; ++c)
    for (int o = in_wave >> 1; o >= Lp; o >>= 1) {
      const int f = __shfl_xor(commit[c], o);
      commit[c] = commit[c] < f ? commit[c] : f;
    }
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

// the instantiation of K maps at the class width NC
template <int NC>
void hblu_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeLadderUsersArgs &a, const HbluPack &pk) {
  switch (K) {
    case 1: hipLaunchKernelGGL((fo_hr_brake_ladder_users_kernel<NC, 1>), grid, block, lds, s, a, pk); break;
    case 2: hipLaunchKernelGGL((fo_hr_brake_ladder_users_kernel<NC, 2>), grid, block, lds, s, a, pk); break;
    default: hipLaunchKernelGGL((fo_hr_brake_ladder_users_kernel<NC, 3>), grid, block, lds, s, a, pk); break;
  }
}

}  // namespace
