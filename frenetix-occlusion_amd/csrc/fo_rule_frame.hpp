// fo_rule_frame.hpp -- the curvilinear frames the spawn rule families project through: the polyline frame of the ego's reference
// path (rl_pl_*, rl_to_curv) and the caller's own frame sampled into a table (rl_cf_*), each by a thread, by a wave and for N
// points at once, and rl_to_curv_wave / rl_to_curv_wave_n / rl_to_cart, which pick by RuleView::frame.
#pragma once
#include "fo_rule_cells.hpp"

namespace {

// ---- polyline frame (utils/curvilinear.PolylineCS): d positive to the left; false outside the projection domain
// the projection by a whole wave (every lane must call it with the same point): lane l takes the segments l, l + 64,
// ...; the wave keeps the smallest (distance, segment index) -- the first minimum of a sequential scan -- and every
// lane returns it.  (One thread scanning is a chain of ~n_path dependent trips to the table in HBM.)
__device__ inline bool rl_pl_to_curv_wave(const RuleView &v, double x, double y, double &s, double &d) {
  const int ns = v.n_path - 1, lane = threadIdx.x & 63;
  double best = INFINITY, bt = 0.0, btc = 0.0;
  int k = 0x7fffffff;
  for (int i = lane; i < ns; i += 64) {
    const double *q = v.path + 6 * (size_t)i;
    const double t = (x - q[0]) * q[4] + (y - q[1]) * q[5];
    const double tc = fmin(fmax(t, 0.0), q[3]);
    const double fx = q[0] + tc * q[4], fy = q[1] + tc * q[5];
    const double d2 = (x - fx) * (x - fx) + (y - fy) * (y - fy);
    if (d2 < best) { best = d2; k = i; bt = t; btc = tc; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double b2 = __shfl_xor(best, off), t2 = __shfl_xor(bt, off), c2 = __shfl_xor(btc, off);
    const int k2 = __shfl_xor(k, off);
    if (b2 < best || (b2 == best && k2 < k)) { best = b2; k = k2; bt = t2; btc = c2; }
  }
  if (k == 0x7fffffff) return false;
  const double *q = v.path + 6 * (size_t)k;
  if ((k == 0 && bt < 0.0) || (k == ns - 1 && bt > q[3])) return false;
  const double fx = q[0] + btc * q[4], fy = q[1] + btc * q[5];
  s = q[2] + btc;
  d = (x - fx) * (-q[5]) + (y - fy) * q[4];
  return true;
}
// N points at once (every lane calls with the same points): the N searches share the pass over the segments and their
// exchanges overlap -- the arithmetic per point is rl_to_curv_wave's (same bits); ok bit n = point n projects onto the path.
// (A projection alone is six exchange steps of LDS-crossbar latency: one after the other, the five of an obstacle's centre
// and corners cost the static rule 10 us.)
template <int N>
__device__ inline unsigned rl_pl_to_curv_wave_n(const RuleView &v, const double *x, const double *y, double *s, double *d) {
  const int ns = v.n_path - 1, lane = threadIdx.x & 63;
  double best[N], bt[N], btc[N];
  int k[N];
#pragma unroll
  for (int n = 0; n < N; ++n) { best[n] = INFINITY; bt[n] = 0.0; btc[n] = 0.0; k[n] = 0x7fffffff; }
  for (int i = lane; i < ns; i += 64) {
    const double *q = v.path + 6 * (size_t)i;
    const double q0 = q[0], q1 = q[1], q3 = q[3], q4 = q[4], q5 = q[5];
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const double t = (x[n] - q0) * q4 + (y[n] - q1) * q5;
      const double tc = fmin(fmax(t, 0.0), q3);
      const double fx = q0 + tc * q4, fy = q1 + tc * q5;
      const double d2 = (x[n] - fx) * (x[n] - fx) + (y[n] - fy) * (y[n] - fy);
      if (d2 < best[n]) { best[n] = d2; k[n] = i; bt[n] = t; btc[n] = tc; }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const double b2 = __shfl_xor(best[n], off);
      const int k2 = __shfl_xor(k[n], off);
      if (b2 < best[n] || (b2 == best[n] && k2 < k[n])) { best[n] = b2; k[n] = k2; }
    }
  }
  unsigned ok = 0u;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    if (k[n] == 0x7fffffff) continue;
    // (segment i lives in lane i mod 64: its parameters from there instead of through the six exchange steps)
    const double t_ = __shfl(bt[n], k[n] & 63), tc_ = __shfl(btc[n], k[n] & 63);
    const double *q = v.path + 6 * (size_t)k[n];
    if ((k[n] == 0 && t_ < 0.0) || (k[n] == ns - 1 && t_ > q[3])) continue;
    const double fx = q[0] + tc_ * q[4], fy = q[1] + tc_ * q[5];
    s[n] = q[2] + tc_;
    d[n] = (x[n] - fx) * (-q[5]) + (y[n] - fy) * q[4];
    ok |= 1u << n;
  }
  return ok;
}
__device__ inline bool rl_pl_to_cart(const RuleView &v, double s, double d, double &x, double &y) {
  const int n = v.n_path;
  if (s < v.path[2] || s > v.path[6 * (size_t)(n - 1) + 2]) return false;
  int lo = 0, hi = n;   // searchsorted(s_table, s, side = 'right'): first index with table > s
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v.path[6 * (size_t)mid + 2] <= s) lo = mid + 1; else hi = mid;
  }
  const int k = min(lo - 1, n - 2);
  const double *q = v.path + 6 * (size_t)k;
  x = q[0] + (s - q[2]) * q[4] + d * (-q[5]);
  y = q[1] + (s - q[2]) * q[5] + d * q[4];
  return true;
}

// ---- the caller's frame (fo_spawn_rule_params_t::frame = 1; DESIGN.md section 6, "The caller's frame"): a row per vertex
// x, y (the base point b_i), the caller's s_i, the polyline arc length of the vertex (read by the turn rule only), the caller's
// normal n_i (not unit); the step of segment i is s_{i+1} - s_i of column 2.  On segment i, lambda in
// [0, 1]: b = b_i + lambda (b_{i+1} - b_i), n = n_i + lambda (n_{i+1} - n_i), the point b + d n.  Same operations in the same
// order as tests/test_caller_frame_cpu.py's InterpolatedNormalFrame (the scene stage builds with -ffp-contract=off).
// rl_cf_segment: the roots of cross(q - b(lambda), n(lambda)) = 0 in [-1e-12, 1 + 1e-12], clamped to [0, 1], on segment i (row r, the next row r + 6); a root
// nearer to the point than `best` (squared distance to b) becomes the candidate -- the smaller root first, so that ties keep it
__device__ __forceinline__ void rl_cf_segment(const double *r, int i, double x, double y, double &best, double &blam, int &k) {
  const double wx = x - r[0], wy = y - r[1];
  const double ex = r[6] - r[0], ey = r[7] - r[1], fx = r[10] - r[4], fy = r[11] - r[5];
  const double a = fx * ey - fy * ex;                                  // cross(dn, db)
  const double b = (wx * fy - wy * fx) - (ex * r[5] - ey * r[4]);      // cross(w, dn) - cross(db, n_i)
  const double c = wx * r[5] - wy * r[4];                              // cross(w, n_i)
  double l0, l1 = NAN;
  if (fabs(a) <= 1e-12 * fabs(b)) {
    l0 = -c / b;
  } else {
    const double disc = b * b - 4.0 * a * c;
    if (!(disc >= 0.0)) return;
    const double sq = sqrt(disc);
    const double t = -0.5 * (b + (b >= 0.0 ? sq : -sq));
    l0 = t / a;
    l1 = c / t;
    if (l1 < l0) { const double u = l0; l0 = l1; l1 = u; }
  }
  // (a root within 1e-12 of [0, 1] counts, clamped: a vertex that ends the path comes out at 1 + a rounding error)
  if (l0 >= -1e-12 && l0 <= 1.0 + 1e-12) {
    l0 = fmin(fmax(l0, 0.0), 1.0);
    const double px = x - (r[0] + l0 * ex), py = y - (r[1] + l0 * ey), d2 = px * px + py * py;
    if (d2 < best) { best = d2; blam = l0; k = i; }
  }
  if (l1 >= -1e-12 && l1 <= 1.0 + 1e-12) {
    l1 = fmin(fmax(l1, 0.0), 1.0);
    const double px = x - (r[0] + l1 * ex), py = y - (r[1] + l1 * ey), d2 = px * px + py * py;
    if (d2 < best) { best = d2; blam = l1; k = i; }
  }
}
// (s, d) of the point at lambda on segment k
__device__ __forceinline__ void rl_cf_sd(const RuleView &v, int k, double lam, double x, double y, double &s, double &d) {
  const double *r = v.path + 6 * (size_t)k;
  const double bx = r[0] + lam * (r[6] - r[0]), by = r[1] + lam * (r[7] - r[1]);
  const double nx = r[4] + lam * (r[10] - r[4]), ny = r[5] + lam * (r[11] - r[5]);
  const double px = x - bx, py = y - by;
  d = (px * nx + py * ny) / (nx * nx + ny * ny);
  s = r[2] + lam * (r[8] - r[2]);
}
// rl_pl_to_curv_wave's shape: lane l takes the segments l, l + 64, ...; the smallest (distance, segment) over the wave
__device__ inline bool rl_cf_to_curv_wave(const RuleView &v, double x, double y, double &s, double &d) {
  const int ns = v.n_path - 1, lane = threadIdx.x & 63;
  double best = INFINITY, blam = 0.0;
  int k = 0x7fffffff;
  for (int i = lane; i < ns; i += 64) rl_cf_segment(v.path + 6 * (size_t)i, i, x, y, best, blam, k);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double b2 = __shfl_xor(best, off), l2 = __shfl_xor(blam, off);
    const int k2 = __shfl_xor(k, off);
    if (b2 < best || (b2 == best && k2 < k)) { best = b2; k = k2; blam = l2; }
  }
  if (k == 0x7fffffff) return false;   // no segment has a root: outside the projection domain
  rl_cf_sd(v, k, blam, x, y, s, d);
  return true;
}
// rl_pl_to_curv_wave_n's shape: N points share the pass over the segments
template <int N>
__device__ inline unsigned rl_cf_to_curv_wave_n(const RuleView &v, const double *x, const double *y, double *s, double *d) {
  const int ns = v.n_path - 1, lane = threadIdx.x & 63;
  double best[N], blam[N];
  int k[N];
#pragma unroll
  for (int n = 0; n < N; ++n) { best[n] = INFINITY; blam[n] = 0.0; k[n] = 0x7fffffff; }
  for (int i = lane; i < ns; i += 64) {
    const double *r = v.path + 6 * (size_t)i;
#pragma unroll
    for (int n = 0; n < N; ++n) rl_cf_segment(r, i, x[n], y[n], best[n], blam[n], k[n]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const double b2 = __shfl_xor(best[n], off);
      const int k2 = __shfl_xor(k[n], off);
      if (b2 < best[n] || (b2 == best[n] && k2 < k[n])) { best[n] = b2; k[n] = k2; }
    }
  }
  unsigned ok = 0u;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    if (k[n] == 0x7fffffff) continue;
    const double lam = __shfl(blam[n], k[n] & 63);   // (segment i's candidate lives in lane i mod 64)
    rl_cf_sd(v, k[n], lam, x[n], y[n], s[n], d[n]);
    ok |= 1u << n;
  }
  return ok;
}
__device__ inline bool rl_cf_to_cart(const RuleView &v, double s, double d, double &x, double &y) {
  const int n = v.n_path;
  if (s < v.path[2] || s > v.path[6 * (size_t)(n - 1) + 2]) return false;
  int lo = 0, hi = n;   // the segment as in rl_pl_to_cart
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v.path[6 * (size_t)mid + 2] <= s) lo = mid + 1; else hi = mid;
  }
  const int k = min(lo - 1, n - 2);
  const double *r = v.path + 6 * (size_t)k;
  const double lam = (s - r[2]) / (r[8] - r[2]);
  const double bx = r[0] + lam * (r[6] - r[0]), by = r[1] + lam * (r[7] - r[1]);
  const double nx = r[4] + lam * (r[10] - r[4]), ny = r[5] + lam * (r[11] - r[5]);
  x = bx + d * nx;
  y = by + d * ny;
  return true;
}

// the frame the rules project through: v.frame is a kernel argument, the branch is uniform over the wave
__device__ inline bool rl_to_curv_wave(const RuleView &v, double x, double y, double &s, double &d) {
  if (v.frame) return rl_cf_to_curv_wave(v, x, y, s, d);
  return rl_pl_to_curv_wave(v, x, y, s, d);
}
template <int N>
__device__ inline unsigned rl_to_curv_wave_n(const RuleView &v, const double *x, const double *y, double *s, double *d) {
  if (v.frame) return rl_cf_to_curv_wave_n<N>(v, x, y, s, d);
  return rl_pl_to_curv_wave_n<N>(v, x, y, s, d);
}
__device__ inline bool rl_to_cart(const RuleView &v, double s, double d, double &x, double &y) {
  if (v.frame) return rl_cf_to_cart(v, s, d, x, y);
  return rl_pl_to_cart(v, s, d, x, y);
}

}  // namespace
