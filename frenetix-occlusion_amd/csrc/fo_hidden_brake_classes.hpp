// fo_hidden_brake_classes.hpp -- hidden-traffic brake clearance for several road-user speeds in one pass
// (fo_scene_hidden_brake_classes; DESIGN.md §5.10 "Brake clearance by classes").  An EXTENSION, not part of the reference.
// Included by fo_scene.hip after fo_hidden_brake.hpp and fo_hidden_clearance.hpp (same translation unit, same flags:
// -ffp-contract=off); staging, length, stop sample, pose step, commit rule and shuffle minimum are fo_hidden_brake.hpp's, where the
// bounds reasoning of all of them stands.
//
// Inputs are the key map and qmin of ONE clearance call and a threshold table thr [C][T] = 169 R2_c[j], one row per class of hidden
// road user.  Per cell A_c(g) <= j iff key(g) <= thr[c][j], so the minimum key under a braking pose decides every class at once:
// the manoeuvre of (m, b) is walked once, not once per class.  The definition stands in include/fo_hip.h.
//   fo_hr_brake_classes_kernel<NC>  the lanes of fo_hr_brake_kernel; next to the six rows the trajectory's qmin row and the
//                        threshold table, staged from the kernel argument once per workgroup (brake_classes_lds_bytes).  Per pose the
//                        lane keeps the minimum key of the footprint and tests it against the classes still open; the walk ends
//                        when every class has its first hit, or at the standing pose, where ONE scan settles every open class by
//                        the first i' >= i with q <= thr[c][i'] (the rows do not decrease).  first[c] and commit[c] are shuffle
//                        minima over the G lanes.  NC = brake_classes_width(C) >= C is the compile-time class count: the
//                        per-class state (first hit, first, commit) is indexed by unrolled loops alone and stays in registers;
//                        classes c >= C are never open, read no threshold and are not stored.
// The key map is read through the caches.  Class indices into the table are bounded by c < C.  Every byte of every output is written.
#pragma once
#include "fo_hidden_brake.hpp"
#include "fo_hidden_clearance.hpp"

namespace {

struct HbThr { int32_t v[FO_HIDDEN_BRAKE_MAX_TABLE]; };   // [C][T], row c from v[c * T]; entries beyond C * T are not read

struct HrBrakeClassesArgs {
  int M, T, G, C;                       // G lanes per trajectory (power of two, <= 64), C classes
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  const int32_t *len;                   // [M] or null
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;                 // the window
  const int32_t *key;                   // [ny][nx]
  const int32_t *qmin;                  // [M][T]
  const double *v, *arc;                // [M][T]
  double a_brake, dt;
  int32_t *brake_first;                 // [C][M][T]
  int32_t *stop;                        // [M][T]
  int32_t *commit, *first;              // [C][M]
};
static_assert(sizeof(HrBrakeClassesArgs) + sizeof(HbThr) <= 4096, "the arguments and the table fit the kernel-argument segment");
static_assert(FO_HIDDEN_BRAKE_MAX_CLASSES == 8, "brake_classes_width and the instantiations below serve up to 8 classes");

// dynamic LDS: brake_classes_lds_bytes(T, C)
template <int NC>
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_classes_kernel(const HrBrakeClassesArgs a, const HbThr thr) {
  extern __shared__ double hbc_rows[];  // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin, then thr
  const int32_t *__restrict__ K = a.key;
  const int G = a.G, T = a.T, nc = a.C, per_block = HB_THREADS / G;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = m < a.M;
  int32_t *QM = (int32_t *)(hbc_rows + (size_t)per_block * 6 * T);   // [per_block][T]
  int32_t *TH = QM + (size_t)per_block * T;                          // [C][T]
  hb_stage_rows(a, hbc_rows, m0, per_block, [&](int t, size_t i) { QM[t] = a.qmin[i]; });
  for (int t = threadIdx.x; t < nc * T; t += HB_THREADS) TH[t] = thr.v[t];     // (C * T <= FO_HIDDEN_BRAKE_MAX_TABLE: the host's refusal)
  __syncthreads();
  const double *X = hbc_rows + (size_t)sub * 6 * T, *Y = X + T, *C = Y + T, *S = C + T, *ARC = S + T, *V = ARC + T;
  const int32_t *Q = QM + (size_t)sub * T;
  const int Lm = live ? hb_length(a, m) : 0;
  // first[c] = min { k < Lm : qmin[m][k] <= thr[c][k] }: the lanes of the trajectory split its samples
  int fm[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) fm[c] = 0x7fffffff;
  for (int k = kl; k < Lm; k += G) {
    const int q = Q[k];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc && q <= TH[c * T + k]) fm[c] = fm[c] < k ? fm[c] : k;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hb_shfl_min(fm[c], 1, G);               // lanes of a trajectory are G consecutive lanes of one wave
    if (fm[c] == 0x7fffffff) fm[c] = -1;
  }
  const HrBox sb = fo_hr_scan_box(a);
  const unsigned every = (1u << nc) - 1u;           // bit c: class c has no first hit yet
  int commit[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) commit[c] = 0x7fffffff;
  for (int b = kl; b < T; b += G) {
    int bf[NC], st = -1;
#pragma unroll
    for (int c = 0; c < NC; ++c) bf[c] = -1;
    if (b < Lm) {                       // (Lm = 0 on lanes without a trajectory)
      const int last = Lm - 1;
      const double vb = V[b], arc_end = ARC[last];
      st = hb_stop_sample(vb, a.a_brake, a.dt, b, Lm);
      double s = ARC[b];
      int j = 0;
      unsigned open = every;
      for (int i = b + 1; i < Lm; ++i) {
        const HbPose p = hb_pose_step(X, Y, C, S, ARC, Lm, last, arc_end, vb, a.a_brake, a.dt, i, b, s, j);
        int q = HC_NONE;
        fo_hr_scan_pose_rows(a, p.x, p.y, p.c, p.s, K, HC_NONE, sb.lox, sb.loy, sb.hix, sb.hiy, 0, 1,
                             [&](int kv, int, int) { q = q < kv ? q : kv; });
        if (i >= st) {                  // the ego stands: this pose is the manoeuvre's last one, hit_c(i') for i' >= i iff q <= thr[c][i']
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if ((open >> c & 1u) && q <= TH[c * T + last]) {
              int at = i;
              while (q > TH[c * T + at]) ++at;      // (ends at Lm - 1 at the latest, whatever the row holds)
              bf[c] = at;
            }
          break;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if ((open >> c & 1u) && q <= TH[c * T + i]) { bf[c] = i; open &= ~(1u << c); }
        if (!open) break;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (hb_unclear(fm[c], b, bf[c], st)) commit[c] = commit[c] < b ? commit[c] : b;
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) a.brake_first[((size_t)c * a.M + (size_t)m) * T + b] = bf[c];
      a.stop[(size_t)m * T + b] = st;
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hb_shfl_min(commit[c], 1, G);
    if (live && kl == 0 && c < nc) {
      a.commit[(size_t)c * a.M + (size_t)m] = commit[c] == 0x7fffffff ? -1 : commit[c];
      a.first[(size_t)c * a.M + (size_t)m] = fm[c];
    }
  }
}

}  // namespace
