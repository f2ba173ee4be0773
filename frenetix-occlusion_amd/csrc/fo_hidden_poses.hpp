// fo_hidden_poses.hpp -- the device pose preparation of the hidden-traffic answers (fo_scene_hidden_poses; DESIGN.md §5.10
// "Fail-safe verdict"): what the host did around every brake call -- (cos, sin) of the headings, the travelled arc -- and whether a
// candidate's poses are numbers at all.  An EXTENSION, not part of the reference.  Included by fo_scene.hip (same translation unit,
// same flags: -ffp-contract=off).  The forecast and the walks still take no trigonometry: they read `heading` as data.
//   fo_hidden_poses_kernel  POSES_THREADS trajectories per workgroup.  Phase 1: the lanes split the workgroup's samples, which are
//                        contiguous in memory: ONE sincos(theta, &s, &c) per sample, as fo_prep_traj_block does, stored as (cos, sin).
//                        Phase 2: a lane per trajectory -- arc is be.py's insert(cumsum(sqrt(diff(x)^2 + diff(y)^2)), 0, 0) as a
//                        SEQUENTIAL float64 sum in index order (numpy's cumsum on a host array; a parallel scan would round
//                        otherwise), over all T samples whatever len says, as travelled_arc does; finite[m] = 1 iff every x, y, theta, v
//                        of the samples k < Lm is finite (Lm = T clipped by len[m]).
// No atomics, no scratch, no LDS, plain vector stores; every byte of every output is written.  Every index is m * T + k with
// m < M, k < T.
#pragma once
#include "fo_scene_plan.hpp"

namespace {

struct HiddenPosesArgs {
  int M, T;
  const double *x, *y, *theta, *v;      // [M][T]
  const int32_t *len;                   // [M] or null
  double *heading;                      // [M][T][2]
  double *arc;                          // [M][T]
  uint8_t *finite;                      // [M]
};

__global__ __launch_bounds__(POSES_THREADS) void fo_hidden_poses_kernel(const HiddenPosesArgs a) {
  const int T = a.T;
  const long long m0 = (long long)blockIdx.x * POSES_THREADS;
  const long long left = (long long)a.M - m0;
  const int n = left < POSES_THREADS ? (int)left : POSES_THREADS;   // (>= 1: the grid is poses_blocks(M))
  const size_t base = (size_t)m0 * T;
  for (int i = threadIdx.x; i < n * T; i += POSES_THREADS) {
    double sn, cs;
    sincos(a.theta[base + i], &sn, &cs);
    a.heading[2 * (base + i)] = cs;
    a.heading[2 * (base + i) + 1] = sn;
  }
  if ((int)threadIdx.x >= n) return;
  const long long m = m0 + threadIdx.x;
  const size_t row = (size_t)m * T;
  int Lm = T;
  if (a.len) { const int l = a.len[m]; Lm = l < 0 ? 0 : (l < T ? l : T); }
  bool ok = true;
  double s = 0.0, px = a.x[row], py = a.y[row];
  a.arc[row] = 0.0;
  if (0 < Lm) ok = isfinite(px) && isfinite(py) && isfinite(a.theta[row]) && isfinite(a.v[row]);
  for (int k = 1; k < T; ++k) {
    const double qx = a.x[row + k], qy = a.y[row + k];
    const double dx = qx - px, dy = qy - py;
    s += sqrt(dx * dx + dy * dy);
    a.arc[row + k] = s;
    if (k < Lm) ok = ok && isfinite(qx) && isfinite(qy) && isfinite(a.theta[row + k]) && isfinite(a.v[row + k]);
    px = qx;
    py = qy;
  }
  a.finite[m] = ok ? 1 : 0;
}

}  // namespace
