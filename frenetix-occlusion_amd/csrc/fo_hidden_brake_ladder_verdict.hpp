// fo_hidden_brake_ladder_verdict.hpp -- the hidden-traffic ladder verdict (fo_scene_hidden_brake_ladder_verdict; DESIGN.md §5.10
// "Ladder verdict"): the deceleration each candidate needs, from the worst of the brake starts up to the replanning interval, to stay
// clear of every class of hidden road user -- folded into the two reserved columns of the planning step's cost row and its safety
// flag.  An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_brake_ladder_users.hpp and
// fo_hidden_brake_verdict.hpp (same translation unit, same flags: -ffp-contract=off); it walks with hb_speed and hb_pose_step, scans
// with fo_hr_scan_pose_rows, decides with HbuKeys / hbu_hits and takes the levels and the table as the HbluPack argument, all
// unchanged: the arithmetic of a manoeuvre exists once.  What the groups' answers mean per trajectory is fo_hidden_ladder_verdict.hpp's.
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
// No [M][B] or [M][B][L] buffer exists.  The key maps are read through the caches and never written, so two of them may be the same
// buffer.  Every LDS index is clamped to [0, Lm) or bounded by c < C, the level index is < L, and a map is read only at a window index
// that was tested against the window: no content of v, arc, the keys, qmin, thr, map_of, the levels or finite can make a lane read out
// of range.  No atomics, no scratch, plain vector stores; every byte of every output is written; of cost and safe only what the
// definition names.
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
  for (int t = threadIdx.x; t < per_block * T; t += HB_THREADS) {
    const int su = t / T, ks = t - su * T;
    if (m0 + su < a.M) {
      const size_t i = (size_t)(m0 + su) * T + ks;
      double *row = hblv_rows + (size_t)su * 6 * T + ks;
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
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hblv_rows + (size_t)row_of * 6 * T, *Y = X + T, *C = Y + T, *S = C + T, *ARC = S + T, *V = ARC + T;
  const int32_t *Q = QM + (size_t)row_of * T;       // map k2: Q[k2 * per_block * T + j]
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
#pragma unroll
      for (int c = 0; c < NC; ++c) bf[c] = -1;
      const int last = Lm - 1;
      const double vb = V[b], arc_end = ARC[last];
      int st = Lm;
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
        if (c < nc && ((fm[c] >= 0 && fm[c] <= b) || (bf[c] >= 0 && bf[c] < st))) um |= 1u << c;
    }
    // every lane of the wave is here: one ballot per class holds the unclear bits of all its (m, b) groups
    unsigned long long any = 0, segs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      segs[c] = (__builtin_amdgcn_ballot_w64((um >> c & 1u) != 0) >> seg_shift) & seg_mask;
      any |= segs[c];
    }
    if (b < ends) {                     // (the Lp lanes of (m, b) agree on it, and on everything below)
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) {
          const unsigned long long clear = ~segs[c] & lv_mask;
          need_of[c] = fo_hidden_ladder_max(need_of[c], fo_hidden_ladder_rank(__builtin_ffsll((long long)clear) - 1, L));
        }
      const unsigned long long clear = ~any & lv_mask;
      const int req = __builtin_ffsll((long long)clear) - 1;
      const int lvl = req < 0 ? L - 1 : req - 1;    // (req = 0: -1, nothing blocks)
      unsigned at_level = 0;            // bit c: class c is unclear at the level below the required one
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (lvl >= 0 && (segs[c] >> lvl & 1ull)) at_level |= 1u << c;
      key = fo_hidden_ladder_max(key, fo_hidden_ladder_key(fo_hidden_ladder_rank(req, L), b, (int32_t)at_level));
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

// the instantiation of K maps at the class width NC
template <int NC>
void hblv_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeLadderVerdictArgs &a, const HbluPack &pk) {
  switch (K) {
    case 1: hipLaunchKernelGGL((fo_hr_brake_ladder_verdict_kernel<NC, 1>), grid, block, lds, s, a, pk); break;
    case 2: hipLaunchKernelGGL((fo_hr_brake_ladder_verdict_kernel<NC, 2>), grid, block, lds, s, a, pk); break;
    default: hipLaunchKernelGGL((fo_hr_brake_ladder_verdict_kernel<NC, 3>), grid, block, lds, s, a, pk); break;
  }
}

}  // namespace
