// fo_hidden_brake_verdict.hpp -- the hidden-traffic fail-safe verdict (fo_scene_hidden_brake_verdict; DESIGN.md §5.10 "Fail-safe
// verdict"): is each candidate still fail-safe against every class of hidden road user from every brake start up to the replanning
// interval -- folded into the two reserved columns of the planning step's cost row and its safety flag.  An EXTENSION, not part of
// the reference.  Included by fo_scene.hip after fo_hidden_brake_users.hpp (same translation unit, same flags: -ffp-contract=off);
// it walks with hb_speed and hb_pose_step, scans with fo_hr_scan_pose_rows and decides with HbuKeys / hbu_hits, all unchanged: the
// arithmetic of a manoeuvre exists once.  What the lanes' commits mean per trajectory is fo_hidden_verdict.hpp's.
//
// Inputs are those of fo_hr_brake_users_kernel, B (the brake starts walked), commit_min, finite [M] and the cost / safe pair.  The
// definition stands in include/fo_hip.h.
//   fo_hr_brake_verdict_kernel<NC, NK>  the users kernel over b < B alone and without brake_first / stop: a lane per (m, b),
//                        G = brake_verdict_group(B) lanes per trajectory (a power of two <= 64: one wave holds them), P =
//                        brake_verdict_per_block(T, K, B) trajectories per workgroup -- LDS caps P, so the lanes from P * G on
//                        stage rows and then have no trajectory.  LDS as in the users kernel: the six rows and the K qmin rows of
//                        each trajectory, then the table (brake_verdict_lds_bytes).  first[c] runs over ALL samples k < Lm (it is
//                        the users entry's), the lanes of a trajectory split them.  commit[c] is the minimum over the G lanes by
//                        __shfl_xor; lane 0 of each trajectory forms the class minimum, writes the outputs and folds the row.
// The key maps are read through the caches and never written, so two of them may be the same buffer.  Every LDS index is clamped to
// [0, Lm) or bounded by c < C, and a map is read only at a window index that was tested against the window: no content of v, arc,
// the keys, qmin, thr, map_of or finite can make a lane read out of range.  No atomics, no scratch, plain vector stores; every byte
// of every output is written; of cost and safe only what the definition names.
#pragma once
#include "fo_hidden_brake_users.hpp"
#include "fo_hidden_verdict.hpp"

namespace {

struct HrBrakeVerdictArgs {
  int M, T, G, P, C, B;                 // G lanes per trajectory (power of two, <= 64), P trajectories per workgroup, C classes, B starts
  int commit_min;
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
  double a_brake, dt;
  const uint8_t *finite;                // [M] or null (every candidate counts as finite)
  double *cost;                         // [M][FO_NC] or null (both or neither)
  uint8_t *safe;                        // [M] or null
  int32_t *fail_safe, *user;            // [M]
  int32_t *commit, *first;              // [C][M]
};
static_assert(sizeof(HrBrakeVerdictArgs) + sizeof(HbThr) <= 4096, "the arguments, map_of and the table fit the kernel-argument segment");

// dynamic LDS: brake_verdict_lds_bytes(T, K, C, B)
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_verdict_kernel(const HrBrakeVerdictArgs a, const HbThr thr) {
  extern __shared__ double hbv_rows[];  // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin per map, then thr
  const int G = a.G, T = a.T, B = a.B, nc = a.C, per_block = a.P;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = sub < per_block && m < a.M;
  int32_t *QM = (int32_t *)(hbv_rows + (size_t)per_block * 6 * T);   // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  for (int t = threadIdx.x; t < per_block * T; t += HB_THREADS) {
    const int su = t / T, k = t - su * T;
    if (m0 + su < a.M) {
      const size_t i = (size_t)(m0 + su) * T + k;
      double *row = hbv_rows + (size_t)su * 6 * T + k;
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
  for (int t = threadIdx.x; t < nc * T; t += HB_THREADS) TH[t] = thr.v[t];     // (C * T <= FO_HIDDEN_BRAKE_MAX_TABLE: the host's refusal)
  __syncthreads();
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hbv_rows + (size_t)row_of * 6 * T, *Y = X + T, *C = Y + T, *S = C + T, *ARC = S + T, *V = ARC + T;
  const int32_t *Q = QM + (size_t)row_of * T;       // map k2: Q[k2 * per_block * T + k]
  int Lm = 0;
  if (live) {
    Lm = T;
    if (a.len) { const int l = a.len[m]; Lm = l < 0 ? 0 : (l < T ? l : T); }
  }
  const unsigned every = (1u << nc) - 1u;           // bit c: class c is there (c < C); in the walk: it has no first hit yet
  unsigned cm1 = 0, cm2 = 0;                        // bit c: class c is held against map 1 / map 2
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int mo = hbu_map_of(a.map_of, c);
    if (c < nc && mo == 1) cm1 |= 1u << c;
    if (c < nc && mo == 2) cm2 |= 1u << c;
  }
  // first[c] = min { k < Lm : qmin_map_of[c][m][k] <= thr[c][k] }: the lanes of the trajectory split its samples
  int fm[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) fm[c] = 0x7fffffff;
  for (int k = kl; k < Lm; k += G) {
    HbuKeys q{Q[k], 0, 0};
    if constexpr (NK > 1) q.q1 = Q[(size_t)per_block * T + k];
    if constexpr (NK > 2) q.q2 = Q[(size_t)2 * per_block * T + k];
    const unsigned h = hbu_hits<NC, NK>(q, TH, T, k, every, cm1, cm2);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (h >> c & 1u) fm[c] = fm[c] < k ? fm[c] : k;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    for (int o = G >> 1; o > 0; o >>= 1) {          // lanes of a trajectory are G consecutive lanes of one wave
      const int f = __shfl_xor(fm[c], o);
      fm[c] = fm[c] < f ? fm[c] : f;
    }
    if (fm[c] == 0x7fffffff) fm[c] = -1;
  }
  // cells beyond the raster and the window have no key: the scan never leaves their union
  const int lox = a.ix0 < 0 ? a.ix0 : 0, loy = a.iy0 < 0 ? a.iy0 : 0;
  const int hix = (a.ix0 + a.nx > a.rnx ? a.ix0 + a.nx : a.rnx) - 1, hiy = (a.iy0 + a.ny > a.rny ? a.iy0 + a.ny : a.rny) - 1;
  int32_t commit[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) commit[c] = 0x7fffffff;
  const int ends = B < Lm ? B : Lm;     // brake starts with a manoeuvre (Lm = 0 on lanes without a trajectory)
  for (int b = kl; b < ends; b += G) {
    int bf[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) bf[c] = -1;
    const int last = Lm - 1;
    const double vb = V[b], arc_end = ARC[last];
    int st = Lm;
    for (int i = b; i < Lm; ++i)
      if (hb_speed(vb, a.a_brake, a.dt, i, b) == 0.0) { st = i; break; }
    double s = ARC[b];
    int j = 0;
    unsigned open = every;
    for (int i = b + 1; i < Lm; ++i) {
      const HbPose p = hb_pose_step(X, Y, C, S, ARC, Lm, last, arc_end, vb, a.a_brake, a.dt, i, b, s, j);
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
      if (i >= st) {                    // the ego stands: this pose is the manoeuvre's last one, hit_c(i') for i' >= i iff q <= thr[c][i']
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
      if ((fm[c] >= 0 && fm[c] <= b) || (bf[c] >= 0 && bf[c] < st)) commit[c] = commit[c] < b ? commit[c] : b;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    for (int o = G >> 1; o > 0; o >>= 1) {
      const int f = __shfl_xor(commit[c], o);
      commit[c] = commit[c] < f ? commit[c] : f;
    }
    commit[c] = commit[c] == 0x7fffffff ? -1 : fo_hidden_verdict_commit(commit[c], B);
  }
  if (live && kl == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        a.commit[(size_t)c * a.M + (size_t)m] = commit[c];
        a.first[(size_t)c * a.M + (size_t)m] = fm[c];
      }
    const bool finite = a.finite ? a.finite[m] != 0 : true;
    const fo_hidden_verdict_t r = fo_hidden_verdict_classes<NC>(commit, nc, B, finite);
    a.fail_safe[m] = r.fail_safe;
    a.user[m] = r.user;
    if (a.cost) fo_hidden_verdict_fold(r, a.commit_min, a.cost + (size_t)m * FO_NC, a.safe + m);
  }
}

// the instantiation of K maps at the class width NC
template <int NC>
void hbv_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeVerdictArgs &a, const HbThr &thr) {
  switch (K) {
    case 1: hipLaunchKernelGGL((fo_hr_brake_verdict_kernel<NC, 1>), grid, block, lds, s, a, thr); break;
    case 2: hipLaunchKernelGGL((fo_hr_brake_verdict_kernel<NC, 2>), grid, block, lds, s, a, thr); break;
    default: hipLaunchKernelGGL((fo_hr_brake_verdict_kernel<NC, 3>), grid, block, lds, s, a, thr); break;
  }
}

}  // namespace
