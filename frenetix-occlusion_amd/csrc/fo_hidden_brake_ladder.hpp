// fo_hidden_brake_ladder.hpp -- hidden-traffic brake ladder (fo_scene_hidden_brake_ladder; DESIGN.md §5.10 "Brake ladder"): per
// candidate and brake start the gentlest deceleration of a ladder of K levels that still keeps the moving ego out of road hidden
// traffic may have reached -- the brake clearance at K decelerations from ONE launch.  An EXTENSION, not part of the reference.
// Included by fo_scene.hip after fo_hidden_brake.hpp (same translation unit, same flags: -ffp-contract=off); staging, length, stop
// sample, pose step, commit rule and shuffle minimum are fo_hidden_brake.hpp's, where the bounds reasoning of all of them stands.
//
// Inputs are those of fo_hr_brake_kernel with the K levels in place of a_brake (they travel as a kernel argument: 512 bytes, no
// transfer, no device buffer) and B, the number of brake starts.  The definition stands in include/fo_hip.h.
//   fo_hr_brake_ladder_kernel   a lane per (m, b, k), lanes along (b, k) with k fastest, padded to Kp = the power of two >= K: the
//                        Kp lanes of one (m, b) are consecutive lanes of one wave and walk the SAME path at neighbouring
//                        decelerations (their LDS reads of the trajectory's rows are mostly broadcasts, their footprints lie
//                        next to each other).  G = brake_ladder_group(T, K, B) lanes per trajectory (a power of two in
//                        [Kp, 256]), 256 / G trajectories per workgroup, whose rows x, y, cos, sin, arc, v are staged in LDS once
//                        by hb_stage_rows; a lane takes the brake starts b = l / Kp, l / Kp + G / Kp, ...  Every lane of
//                        the workgroup runs the same number of rounds, so the shuffles stand outside divergent code.
//                        required and last_unclear are a __shfl_xor minimum and maximum over the Kp lanes of a round; commit[k]
//                        is a minimum over the lanes with the same k: by __shfl_xor within a wave and, where a trajectory has
//                        more than a wave (G = 128, 256), through 1 KB of LDS behind the rows.
// The arrival map is read through the caches.  The level index is < K.  Every byte of every output is written.
#pragma once
#include "fo_hidden_brake.hpp"

namespace {

struct HbLevels { double v[FO_HIDDEN_BRAKE_MAX_LEVELS]; };   // entries beyond K are not read

struct HrBrakeLadderArgs {
  int M, T, B, K;                       // B brake starts, K levels
  int Kp, G;                            // lanes per (m, b) and per trajectory: powers of two, K <= Kp <= G <= HB_THREADS
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  const int32_t *len;                   // [M] or null
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;                 // the window
  const uint8_t *arrival;               // [ny][nx]
  const int32_t *first;                 // [M]
  const double *v, *arc;                // [M][T]
  double dt;
  int32_t *brake_first, *stop;          // [M][B][K]
  int32_t *required, *last_unclear;     // [M][B]
  int32_t *commit;                      // [M][K]
};
static_assert(sizeof(HrBrakeLadderArgs) + sizeof(HbLevels) <= 4096, "the arguments and the levels fit the kernel-argument segment");
static_assert(BRAKE_LADDER_MAX_LEVELS == FO_HIDDEN_BRAKE_MAX_LEVELS && BRAKE_LADDER_MAX_LEVELS <= 64,
              "the lanes of one (m, b) are consecutive lanes of one wave");

// dynamic LDS: brake_ladder_lds_bytes(T, K, B)
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_ladder_kernel(const HrBrakeLadderArgs a, const HbLevels lv) {
  extern __shared__ double hbl_rows[];  // per trajectory of the workgroup: x, y, cos, sin, arc, v, T entries each; then the commit rows
  const uint8_t *__restrict__ A = a.arrival;
  const int G = a.G, T = a.T, B = a.B, K = a.K, Kp = a.Kp, per_block = HB_THREADS / G;
  const int sub = threadIdx.x / G, l = threadIdx.x & (G - 1);
  const int k = l & (Kp - 1), bq = l / Kp, nb = G / Kp;
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = m < a.M, level = k < K;
  hb_stage_rows(a, hbl_rows, m0, per_block, [](int, size_t) {});
  __syncthreads();
  const double *X = hbl_rows + (size_t)sub * 6 * T, *Y = X + T, *C = Y + T, *S = C + T, *ARC = S + T, *V = ARC + T;
  int Lm = 0, fm = -1;
  if (live) {
    Lm = hb_length(a, m);
    fm = a.first[m];
  }
  const double a_brake = level ? lv.v[k] : 0.0;
  const HrBox sb = fo_hr_scan_box(a);
  int commit = 0x7fffffff;
  for (int b0 = 0; b0 < B; b0 += nb) {  // the same rounds on every lane of the workgroup
    const int b = b0 + bq;
    const bool mine = level && b < B;
    int bf = -1, st = -1, clear_k = 0x7fffffff, unclear_k = -1;
    if (mine && b < Lm) {               // (Lm = 0 on lanes without a trajectory)
      const int last = Lm - 1;
      const double vb = V[b], arc_end = ARC[last];
      st = hb_stop_sample(vb, a_brake, a.dt, b, Lm);
      double s = ARC[b];
      int j = 0;
      for (int i = b + 1; i < Lm; ++i) {
        const HbPose p = hb_pose_step(X, Y, C, S, ARC, Lm, last, arc_end, vb, a_brake, a.dt, i, b, s, j);
        // the ego stands from sample st on (vn = 0 adds nothing to s): this pose is the manoeuvre's last one
        const bool stands = i >= st;
        int amin = 255;
        fo_hr_scan_pose_rows(a, p.x, p.y, p.c, p.s, A, 255, sb.lox, sb.loy, sb.hix, sb.hiy, 0, 1,
                             [&](int av, int, int) { amin = amin < av ? amin : av; });
        if (stands) {                   // hit(i') for i' >= i iff amin <= i'
          const int at = amin > i ? amin : i;
          if (at < Lm) bf = at;
          break;
        }
        if (amin <= i) { bf = i; break; }
      }
      if (hb_unclear(fm, b, bf, st)) {
        commit = commit < b ? commit : b;
        unclear_k = k;
      } else {
        clear_k = k;
      }
    }
    for (int o = Kp >> 1; o > 0; o >>= 1) {           // the levels of (m, b) are Kp consecutive lanes of one wave
      const int c = __shfl_xor(clear_k, o), u = __shfl_xor(unclear_k, o);
      clear_k = clear_k < c ? clear_k : c;
      unclear_k = unclear_k > u ? unclear_k : u;
    }
    if (live && mine) {
      const size_t o = ((size_t)m * B + b) * K + k;
      a.brake_first[o] = bf;
      a.stop[o] = st;
      if (k == 0) {
        a.required[(size_t)m * B + b] = clear_k == 0x7fffffff ? -1 : clear_k;
        a.last_unclear[(size_t)m * B + b] = unclear_k;
      }
    }
  }
  // commit[m][k]: the minimum over the lanes of the trajectory with this k -- within the wave ...
  const int in_wave = G < 64 ? G : 64;
  hb_shfl_min(commit, Kp, in_wave);
  if (G > 64) {                         // ... and over the G / 64 waves of the trajectory (G is the workgroup's: no lane diverges)
    int32_t *CM = (int32_t *)(hbl_rows + (size_t)per_block * 6 * T);       // [HB_THREADS / 64][64]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    CM[wave * 64 + lane] = commit;
    __syncthreads();
    const int w0 = wave & ~(G / 64 - 1);
    for (int w = 0; w < G / 64; ++w) {
      const int c = CM[(w0 + w) * 64 + lane];
      commit = commit < c ? commit : c;
    }
  }
  if (live && l < K) a.commit[(size_t)m * K + l] = commit == 0x7fffffff ? -1 : commit;
}

}  // namespace
