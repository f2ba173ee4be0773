// fo_hidden_clearance.hpp -- hidden-traffic clearance (fo_scene_hidden_clearance; DESIGN.md §5.10 "Clearance and critical
// speed").  An EXTENSION, not part of the reference.  Included by fo_scene.hip after the two reach headers (same translation
// unit, same flags: -ffp-contract=off, which the shared footprint test needs); it uses their HrMapArgs, fo_hr_rows_kernel,
// fo_hr_cols_kernel, fo_hr_road_band_kernel, fo_hr_scan_footprint and HR_* constants.
//
// The arrival map of the reach forecast is a monotone function of one integer per cell, the key
//   euclid  169 D2(g)                     road  max(169 D2(g), d(g)^2)
// (A(g) <= j iff key(g) <= 169 R2[j] for every reach table with R2[J-1] <= r2_cap), so the key map and its minimum over the
// footprint of every pose answer the forecast for every hidden-user speed up to the cap.  The key map's column pass is the
// HrKeyOut instantiation of fo_hr_cols_kernel (fo_hidden_reach.hpp: 169 D2 on road cells with D2 <= r2_cap, NONE elsewhere, in
// place of the binary search of R2[]); the two kernels of this file:
//   fo_hc_road_merge_kernel  road metric, after the distance bands run to Lcap = isqrt(169 r2_cap): a thread per cell,
//                            key = max(key, d^2), NONE where d is 65535 (impassable or beyond Lcap)
//   fo_hc_traj_kernel        a thread per pose, poses of a trajectory on consecutive lanes (x, y, heading read contiguously):
//                            the bounding-box scan of fo_hr_traj_kernel (fo_hr_scan_footprint) with a running minimum of the
//                            key in place of the count -> qmin [M][T]; no cross-lane step: first / slack / the critical speed
//                            are derived from qmin afterwards
// No atomics, nothing waits for another workgroup, every output written with plain vector stores.
#pragma once
#include "fo_hidden_reach_road.hpp"

namespace {

constexpr int32_t HC_NONE = FO_HIDDEN_CLEARANCE_NONE;
static_assert((int64_t)169 * 2 * FO_HIDDEN_REACH_MAX_HALO * FO_HIDDEN_REACH_MAX_HALO < HC_NONE, "169 D2 within the cap fits an int32");
static_assert((int64_t)(13 * FO_HIDDEN_REACH_MAX_HALO + 12) * (13 * FO_HIDDEN_REACH_MAX_HALO + 12) < HC_NONE, "d^2 within the cap fits an int32");

struct HcMergeArgs {
  const uint16_t *dist;                 // [n]
  int32_t *key;                         // [n]: 169 D2 or NONE in, the key of the road metric out
  int n;
};

__global__ __launch_bounds__(HR_THREADS) void fo_hc_road_merge_kernel(const HcMergeArgs a) {
  const int i = blockIdx.x * HR_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const int32_t e = a.key[i];
  if (e == HC_NONE) return;             // not road, or D2 beyond the cap
  const int d = a.dist[i];              // <= Lcap or 65535: the bands never store a value above their cap
  a.key[i] = d == HRR_NONE ? HC_NONE : (d * d > e ? d * d : e);
}

struct HcTrajArgs {
  int M, T;
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  const int32_t *len;                   // [M] or null
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;
  const int32_t *key;                   // [ny][nx]
  int32_t *qmin;                        // [M][T]
};

__global__ __launch_bounds__(HR_THREADS) void fo_hc_traj_kernel(const HcTrajArgs a) {
  const int32_t *__restrict__ K = a.key;      // read through the caches, like the arrival map
  const size_t i = (size_t)blockIdx.x * HR_THREADS + threadIdx.x;
  if (i >= (size_t)a.M * a.T) return;
  const size_t m = i / a.T;
  const int k = (int)(i - m * a.T);
  int Lm = a.T;
  if (a.len) { const int l = a.len[m]; Lm = l < 0 ? 0 : (l < a.T ? l : a.T); }
  int q = HC_NONE;
  if (k < Lm) {
    const HrBox sb = fo_hr_scan_box(a);
    fo_hr_scan_footprint(a, i, K, HC_NONE, sb.lox, sb.loy, sb.hix, sb.hiy, [&](int v) { q = q < v ? q : v; });
  }
  a.qmin[i] = q;
}

}  // namespace
