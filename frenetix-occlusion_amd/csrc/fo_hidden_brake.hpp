// fo_hidden_brake.hpp -- hidden-traffic brake clearance (fo_scene_hidden_brake; DESIGN.md §5.10 "Brake clearance"): from which
// sample on "follow the candidate until here, then brake" no longer keeps the moving ego out of road hidden traffic may have
// reached.  An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_reach.hpp (same translation unit,
// same flags: -ffp-contract=off, which the pose arithmetic and the footprint test need).
//
// The home of what all seven brake kernels (this one and fo_hidden_brake_{classes,ladder,users,verdict,ladder_users,ladder_verdict}
// .hpp) share, each piece stated once: the staging of a workgroup's rows (hb_stage_rows), the length clamp (hb_length), the speed
// profile, the stop sample and the pose step of a manoeuvre (hb_speed, hb_stop_sample, hb_pose_step), the commit rule (hb_unclear)
// and the shuffle minimum (hb_shfl_min); the box of the scan is fo_hidden_reach.hpp's (fo_hr_scan_box), like the scan itself.
// What keeps every one of them in range: every LDS index is clamped to [0, Lm) before it is used (hb_pose_step), Lm <= T, the rows
// are staged under m < M, and fo_hr_scan_pose_rows tests every cell against the window and the raster first: no content of v, arc
// or a map can make a lane read out of range.  No atomics, no scratch, plain vector stores.
//
// Inputs are the arrival map A and d_first of one forecast call (any of the three entries) and, next to its trajectories, the
// speed v and the travelled chord length arc per sample, handed over as data.  The definition stands in include/fo_hip.h.
//   fo_hr_brake_kernel   a lane per brake start (m, b), lanes along b; G = the power of two >= min(T, 64) lanes per trajectory,
//                        256 / G trajectories per workgroup, whose rows x, y, cos, sin, arc, v are staged in LDS once (48 T
//                        bytes each).  The lane walks its manoeuvre's samples i = b + 1 .. in order: the running length s is a
//                        serial float64 sum by definition, and the segment index j only ever moves forward (the first index
//                        with arc[j] >= sc is non-decreasing in sc, whatever arc holds).  The walk ends at the first hit, and
//                        once the ego stands (i >= stop) the pose no longer changes: ONE scan that keeps the smallest arrival
//                        step of the footprint answers every remaining sample.  commit is a shuffle minimum over the G lanes.
// The arrival map is read through the caches (the access pattern of fo_hr_traj_kernel).  Every byte of every output is written.
#pragma once
#include "fo_hidden_reach.hpp"

namespace {

static_assert(HB_THREADS == HR_THREADS && HB_THREADS % 64 == 0, "the lanes of a trajectory are consecutive lanes of one wave");

struct HrBrakeArgs {
  int M, T, G;                          // G lanes per trajectory (power of two, <= 64)
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
  double a_brake, dt;
  int32_t *brake_first, *stop;          // [M][T]
  int32_t *commit;                      // [M]
};

// The rows x, y, cos, sin, arc, v (T float64 each, in this order) of the per_block trajectories from m0 on, into `rows`; the
// workgroup's lanes split the elements.  each(t, i) runs once per staged element, t its index in [per_block][T], i in [M][T]: a
// caller stages its qmin rows in the same pass.  The caller's __syncthreads() follows.
template <class Args, class F>
__device__ __forceinline__ void hb_stage_rows(const Args &a, double *rows, long long m0, int per_block, F &&each) {
  const int T = a.T;
  for (int t = threadIdx.x; t < per_block * T; t += HB_THREADS) {
    const int su = t / T, k = t - su * T;
    if (m0 + su < a.M) {
      const size_t i = (size_t)(m0 + su) * T + k;
      double *row = rows + (size_t)su * 6 * T + k;
      row[0] = a.x[i];
      row[T] = a.y[i];
      row[2 * T] = a.heading[2 * i];
      row[3 * T] = a.heading[2 * i + 1];
      row[4 * T] = a.arc[i];
      row[5 * T] = a.v[i];
      each(t, i);
    }
  }
}

// Lm, the samples of trajectory m < M that count: len[m] clamped to [0, T].  (Lanes without a trajectory take Lm = 0 and walk nothing.)
template <class Args>
__device__ __forceinline__ int hb_length(const Args &a, long long m) {
  int Lm = a.T;
  if (a.len) { const int l = a.len[m]; Lm = l < 0 ? 0 : (l < a.T ? l : a.T); }
  return Lm;
}

// vn(i) of a manoeuvre that brakes from sample b at speed vb: be.py's profile, the speed held over a step
__device__ __forceinline__ double hb_speed(double vb, double a_brake, double dt, int i, int b) {
  return fmax(vb - a_brake * ((double)(i - b) * dt), 0.0);
}

// the stop sample of the manoeuvre: the first i in [b, Lm) with vn(i) == 0, Lm if the ego never stands
__device__ __forceinline__ int hb_stop_sample(double vb, double a_brake, double dt, int b, int Lm) {
  int st = Lm;
  for (int i = b; i < Lm; ++i)
    if (hb_speed(vb, a_brake, dt, i, b) == 0.0) { st = i; break; }
  return st;
}

// The commit rule: brake start b is unclear when the candidate itself is hit no later than b (fm = first) or the manoeuvre is hit
// while the ego still moves (bf = its first hit, st = its stop sample)
__device__ __forceinline__ bool hb_unclear(int fm, int b, int bf, int st) { return (fm >= 0 && fm <= b) || (bf >= 0 && bf < st); }

// v becomes the minimum over the lanes whose index differs in the bits [lo, hi) alone (powers of two, hi <= 64: lanes of one wave).
// In place on purpose: taking v by value and returning it, the loop over b of fo_hr_brake_kernel kept one more induction variable,
// the kernel took 66 registers instead of 64 and lost its eighth wave per SIMD (two classes instantiations lost one as well).
__device__ __forceinline__ void hb_shfl_min(int &v, int lo, int hi) {
  for (int o = hi >> 1; o >= lo; o >>= 1) {
    const int w = __shfl_xor(v, o);
    v = v < w ? v : w;
  }
}

// The pose step of a manoeuvre, the ONE statement of step 3's arithmetic on the device: the running length s gains vn(i - 1) dt, the
// segment index j moves forward to the first sample with arc >= the clamped length, the position is interpolated between the
// segment's ends and the heading is the nearer end's.  X .. ARC: the trajectory's rows (LDS), Lm >= 2 its length (i = b + 1 < Lm),
// last = Lm - 1 and arc_end = ARC[last] from the caller; every index is clamped to [0, Lm) before it is used.  (`last` is the
// caller's value on purpose: with Lm - 1 formed in here as well, fo_hr_brake_kernel's address of ARC[Lm - 1] was selected
// differently and the kernel, an instruction longer, took 1.4 % more time.)
struct HbPose { double x, y, c, s; };
__device__ __forceinline__ HbPose hb_pose_step(const double *X, const double *Y, const double *C, const double *S, const double *ARC,
                                               int Lm, int last, double arc_end, double vb, double a_brake, double dt, int i, int b, double &s,
                                               int &j) {
  s = s + hb_speed(vb, a_brake, dt, i - 1, b) * dt;
  const double sc = fmin(s, arc_end);
  while (j < Lm && !(ARC[j] >= sc)) ++j;
  int idx = j < 1 ? 1 : j;
  idx = idx < last ? idx : last;
  const double xlo = ARC[idx - 1], xhi = ARC[idx];
  double xn = X[idx - 1], yn = Y[idx - 1];
  int hd = idx - 1;
  if (xhi != xlo) {
    const double w = sc - xlo, inv = xhi - xlo;
    xn = (X[idx] - X[idx - 1]) / inv * w + X[idx - 1];
    yn = (Y[idx] - Y[idx - 1]) / inv * w + Y[idx - 1];
    if (!(w + w <= inv)) hd = idx;
  }
  return HbPose{xn, yn, C[hd], S[hd]};
}

// dynamic LDS: brake_lds_bytes(T)
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_kernel(const HrBrakeArgs a) {
  extern __shared__ double hb_rows[];   // per trajectory of the workgroup: x, y, cos, sin, arc, v, T entries each
  const uint8_t *__restrict__ A = a.arrival;
  const int G = a.G, T = a.T, per_block = HB_THREADS / G;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = m < a.M;
  hb_stage_rows(a, hb_rows, m0, per_block, [](int, size_t) {});
  __syncthreads();
  const double *X = hb_rows + (size_t)sub * 6 * T, *Y = X + T, *C = Y + T, *S = C + T, *ARC = S + T, *V = ARC + T;
  int Lm = 0, fm = -1;
  if (live) {
    Lm = hb_length(a, m);
    fm = a.first[m];
  }
  const HrBox sb = fo_hr_scan_box(a);
  int commit = 0x7fffffff;
  for (int b = kl; b < T; b += G) {
    int bf = -1, st = -1;
    if (b < Lm) {                       // (Lm = 0 on lanes without a trajectory)
      const int last = Lm - 1;
      const double vb = V[b], arc_end = ARC[last];
      st = hb_stop_sample(vb, a.a_brake, a.dt, b, Lm);
      double s = ARC[b];
      int j = 0;
      for (int i = b + 1; i < Lm; ++i) {
        const HbPose p = hb_pose_step(X, Y, C, S, ARC, Lm, last, arc_end, vb, a.a_brake, a.dt, i, b, s, j);
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
      if (hb_unclear(fm, b, bf, st)) commit = commit < b ? commit : b;
    }
    if (live) {
      a.brake_first[(size_t)m * T + b] = bf;
      a.stop[(size_t)m * T + b] = st;
    }
  }
  hb_shfl_min(commit, 1, G);   // lanes of a trajectory are G consecutive lanes of one wave
  if (live && kl == 0) a.commit[m] = commit == 0x7fffffff ? -1 : commit;
}

}  // namespace
