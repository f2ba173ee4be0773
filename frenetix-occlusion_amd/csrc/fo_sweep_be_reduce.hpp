// fo_sweep_be_reduce.hpp -- the optional brake evaluation (fo_be_prep_kernel, fo_be_kernel), the reduction of the sweep's
// partial rows to cost vectors and safe flags (fo_reduce_kernel) and the metric dependency closure.
// A part of the fo_sweep.hip translation unit, included after fo_sweep_queue.hpp; not a header to include on its own.
#pragma once

namespace {

// ================================================================================================ BE (optional)
// Brake evaluation (metrics/be.py:31-193), active only with FO_M_BE: for every pair that collides at ttc > 0 the minimum
// constant deceleration found by the reference's bisection (<= 10 iterations on [round(|min(a_min, 0)|, 2), 5] m/s^2,
// stop below 0.1) and the brake threat number decel / a_max.  For one candidate deceleration the ego keeps its path,
// the speed profile becomes [v0, max(v1 - decel j dt, 0) ...], poses are re-sampled by linear interpolation over the
// travelled chord length (scipy interp1d semantics: searchsorted-left segment, clipped), rectangles are tested for
// intersection (SAT, touching counts) at every step the agent exists.  Two deviations from the reference: where the
// re-sampled arc length exceeds the path length the reference raises ValueError; here it is clamped to the end of the
// path.  On a path segment of zero length (two samples at one place: an ego that stands) scipy divides by zero and returns
// NaN; here the segment gives its left knot -- the pose, heading included, of the earlier of the two samples.
__global__ void fo_be_prep_kernel(int M, int Mp, int T, const double *__restrict__ x, const double *__restrict__ y,
                                  const double *__restrict__ acc, double *__restrict__ dist, double *__restrict__ mina) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= Mp) return;
  const int ms = min(m, M - 1);
  const double *xs = x + (size_t)ms * T, *ys = y + (size_t)ms * T, *as = acc + (size_t)ms * T;
  double d = 0.0, mn = 0.0;
  dist[m] = 0.0;
  for (int i = 0; i < T; ++i) {
    if (i > 0) {
      const double dx = xs[i] - xs[i - 1], dy = ys[i] - ys[i - 1];
      d += sqrt(dx * dx + dy * dy);
      dist[(size_t)i * Mp + m] = d;
    }
    mn = fmin(mn, as[i]);
  }
  mina[m] = mn;
}

__global__ __launch_bounds__(256) void fo_be_kernel(int M, int Mp, int T, int A, int Ta, const double *__restrict__ traj,
                                                    const double *__restrict__ dist, const double *__restrict__ mina,
                                                    const double *__restrict__ atab, const double *__restrict__ acst,
                                                    const int32_t *__restrict__ aint,
                                                    const signed char *__restrict__ be_mask, double hlA, double hwA,
                                                    double wb, double a_max, double dt, double *__restrict__ be_btn,
                                                    double *__restrict__ pair_f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x, k = blockIdx.y * 4 + wave;
  if (k >= A) return;
  const int m = tile * TILE + lane;
  const int L = aint[2 * k + 1];
  const double hlB = acst[(size_t)k * NAC + 0], hwB = acst[(size_t)k * NAC + 1];
  const double *tjl = traj + (size_t)tile * T * NEF * TILE + 2 * lane;  // this lane's pairs of the tile
  const double *G = atab + (size_t)k * Ta * NAF;
  const bool active = m < M && L > 0 && T >= 2 && be_mask[(size_t)k * Mp + m];
  double decel = 0.0, btn = 0.0;
  if (active) {
    const double v0 = tjl[EF(5)], v1 = tjl[(size_t)NEF * TILE + EF(5)];
    const double dend = dist[(size_t)(T - 1) * Mp + m];
    double min_d = __builtin_rint(fabs(mina[m]) * 100.0) / 100.0, max_d = 5.0;  // np.round(abs(min(min(a), 0)), 2)
    for (int it = 0; it < 10; ++it) {
      const double cur = (min_d + max_d) / 2.0;
      decel = cur;
      bool hit = false;
      double s = 0.0;
      int j = 0;
      for (int i = 0; i < T && !hit; ++i) {
        if (i < L) {
          const double sc = fmin(s, dend);
          while (j < T && dist[(size_t)j * Mp + m] < sc) ++j;  // searchsorted (left); s never decreases
          const int idx = min(max(j, 1), T - 1);
          const double xlo = dist[(size_t)(idx - 1) * Mp + m], xhi = dist[(size_t)idx * Mp + m];
          const double *r0 = tjl + (size_t)(idx - 1) * NEF * TILE, *r1 = tjl + (size_t)idx * NEF * TILE;
          double xn = r0[EF(0)], yn = r0[EF(1)], tn = r0[EF(4)];
          if (xhi != xlo) {
            const double w = sc - xlo, inv = xhi - xlo;
            xn = (r1[EF(0)] - xn) / inv * w + xn;
            yn = (r1[EF(1)] - yn) / inv * w + yn;
            tn = (r1[EF(4)] - tn) / inv * w + tn;
          }
          double es, ec;
          sincos(tn, &es, &ec);
          const double *g = G + (size_t)i * NAF;
          const double px = g[0], py = g[1], pc = g[2], ps = g[3];
          const double cr = pc * ec + ps * es, sr = ps * ec - pc * es;
          const double dx = px - (xn + wb * ec), dy = py - (yn + wb * es);
          const double ax = ec * dx + es * dy, ay = ec * dy - es * dx;
          const double bx = -(pc * dx + ps * dy), by = -(pc * dy - ps * dx);
          const double s1 = fabs(ax) - (hlA + fabs(hlB * cr) + fabs(hwB * sr)), s2 = fabs(ay) - (hwA + fabs(hlB * sr) + fabs(hwB * cr));
          const double s3 = fabs(bx) - (hlB + fabs(hlA * cr) + fabs(hwA * sr)), s4 = fabs(by) - (hwB + fabs(hlA * sr) + fabs(hwA * cr));
          if (!(fmax(fmax(s1, s2), fmax(s3, s4)) > 0.0)) hit = true;  // shapely intersects
        }
        const double vn = (i == 0) ? v0 : fmax(v1 - cur * ((double)(i - 1) * dt), 0.0);
        s += vn * dt;
      }
      if (!hit) max_d = cur; else min_d = cur;
      if (max_d - min_d < 0.1) break;
    }
    btn = decel / a_max;
  }
  if (m < Mp) be_btn[(size_t)k * Mp + m] = btn;
  if (pair_f && m < M && L > 0) {
    const size_t ps_ = (size_t)A * M;
    pair_f[FO_PF_BE_DECEL * ps_ + (size_t)k * M + m] = decel;
    pair_f[FO_PF_BE_BTN * ps_ + (size_t)k * M + m] = btn;
  }
}

// fold the per-chunk partials into the cost vector + safety flag (metric.py:50-100, hr.py:101-114, wttc.py:32-42)
// 64 trajectories per workgroup, eight waves: wave w folds its eighth of the chunk rows (in chunk order), the eight
// partial results meet in LDS and wave 0 folds them in the same order -- ties keep the earliest chunk, exactly like one
// sequential pass, with an eighth of the dependent-load chain.
constexpr int RED_WAVES = 8;
__global__ __launch_bounds__(64 * RED_WAVES) void fo_reduce_kernel(int M, int Mp, int A, int n_chunks,
                                                                   const double *__restrict__ partial,
                                                                   fo_thresholds_t thr, uint32_t mask,
                                                                   const double *__restrict__ be_btn,
                                                                   double *__restrict__ cost,
                                                                   uint8_t *__restrict__ safe,
                                                                   const int *__restrict__ status, int gen) {
  __shared__ double sh[RED_WAVES][NPS + 1][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * 64 + lane;
  const bool live = m < M;
  double max_btn = 0.0;
  double min_dce = INFINITY, arg_dce = -1, min_ttc = INFINITY, arg_ttc = -1, min_ttce = INFINITY;
  double max_er = 0, max_or = 0, arg_or = -1, max_eh = 0, max_oh = 0, max_cp = 0, max_hwc = 0, flag = 0;
  if (live) {
    if (be_btn)
      for (int k = wave; k < A; k += RED_WAVES) max_btn = fmax(max_btn, be_btn[(size_t)k * Mp + m]);
    const int per = (n_chunks + RED_WAVES - 1) / RED_WAVES;
    const int c0 = wave * per, c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
      const double *p = partial + (size_t)c * NPS * Mp + m;
      if (p[PS_MIN_DCE * (size_t)Mp] < min_dce) { min_dce = p[PS_MIN_DCE * (size_t)Mp]; arg_dce = p[PS_ARG_DCE * (size_t)Mp]; }
      if (p[PS_MIN_TTC * (size_t)Mp] < min_ttc) { min_ttc = p[PS_MIN_TTC * (size_t)Mp]; arg_ttc = p[PS_ARG_TTC * (size_t)Mp]; }
      min_ttce = fmin(min_ttce, p[PS_MIN_TTCE * (size_t)Mp]);
      max_er = fmax(max_er, p[PS_MAX_ER * (size_t)Mp]);
      if (p[PS_MAX_OR * (size_t)Mp] > max_or) { max_or = p[PS_MAX_OR * (size_t)Mp]; arg_or = p[PS_ARG_OR * (size_t)Mp]; }
      max_eh = fmax(max_eh, p[PS_MAX_EH * (size_t)Mp]);
      max_oh = fmax(max_oh, p[PS_MAX_OH * (size_t)Mp]);
      max_cp = fmax(max_cp, p[PS_MAX_CP * (size_t)Mp]);
      max_hwc = fmax(max_hwc, p[PS_MAX_HWC * (size_t)Mp]);
      flag = fmax(flag, p[PS_DCE_FLAG * (size_t)Mp]);
    }
  }
  double *q = &sh[wave][0][lane];
  q[PS_MIN_DCE * 64] = min_dce; q[PS_ARG_DCE * 64] = arg_dce; q[PS_MIN_TTC * 64] = min_ttc; q[PS_ARG_TTC * 64] = arg_ttc;
  q[PS_MIN_TTCE * 64] = min_ttce; q[PS_MAX_ER * 64] = max_er; q[PS_MAX_OR * 64] = max_or; q[PS_ARG_OR * 64] = arg_or;
  q[PS_MAX_EH * 64] = max_eh; q[PS_MAX_OH * 64] = max_oh; q[PS_MAX_CP * 64] = max_cp; q[PS_MAX_HWC * 64] = max_hwc;
  q[PS_DCE_FLAG * 64] = flag; q[NPS * 64] = max_btn;
  __syncthreads();
  if (wave != 0 || !live) return;
  for (int w = 1; w < RED_WAVES; ++w) {
    const double *p = &sh[w][0][lane];
    if (p[PS_MIN_DCE * 64] < min_dce) { min_dce = p[PS_MIN_DCE * 64]; arg_dce = p[PS_ARG_DCE * 64]; }
    if (p[PS_MIN_TTC * 64] < min_ttc) { min_ttc = p[PS_MIN_TTC * 64]; arg_ttc = p[PS_ARG_TTC * 64]; }
    min_ttce = fmin(min_ttce, p[PS_MIN_TTCE * 64]);
    max_er = fmax(max_er, p[PS_MAX_ER * 64]);
    if (p[PS_MAX_OR * 64] > max_or) { max_or = p[PS_MAX_OR * 64]; arg_or = p[PS_ARG_OR * 64]; }
    max_eh = fmax(max_eh, p[PS_MAX_EH * 64]);
    max_oh = fmax(max_oh, p[PS_MAX_OH * 64]);
    max_cp = fmax(max_cp, p[PS_MAX_CP * 64]);
    max_hwc = fmax(max_hwc, p[PS_MAX_HWC * 64]);
    flag = fmax(flag, p[PS_DCE_FLAG * 64]);
    max_btn = fmax(max_btn, p[NPS * 64]);
  }
  // the status words of this agent set (fo_ctx.hpp; wave-uniform addresses: scalar loads, once per workgroup): [0] an unusable
  // covariance, [2] a refused rule list -- what they take away from the row: fo_verdict.hpp
  const bool cov_unusable = gen > 0 && status[0] == gen, refused = gen > 0 && status[2] == gen;
  fo_folded_t f{min_ttc, min_dce, max_er, max_or, max_eh, max_oh, max_cp, max_hwc, min_ttce, arg_dce, arg_ttc, arg_or, max_btn, flag};
  const bool ok = fo_verdict(A, mask, thr, cov_unusable, refused, f);
  double *c = cost + (size_t)m * FO_NC;
  c[FO_C_WTTC] = f.min_ttc; c[FO_C_MIN_DCE] = f.min_dce; c[FO_C_MAX_EGO_RISK] = f.max_er; c[FO_C_MAX_OBST_RISK] = f.max_or;
  c[FO_C_MAX_EGO_HARM] = f.max_eh; c[FO_C_MAX_OBST_HARM] = f.max_oh; c[FO_C_MAX_CP] = f.max_cp;
  c[FO_C_HARM_WITH_CP] = f.max_hwc; c[FO_C_MIN_TTCE] = f.min_ttce; c[FO_C_ARGMIN_DCE] = f.arg_dce;
  c[FO_C_ARGMIN_TTC] = f.arg_ttc; c[FO_C_ARGMAX_RISK] = f.arg_or; c[FO_C_SAFE] = ok ? 1.0 : 0.0; c[FO_C_MAX_BTN] = f.max_btn;
  c[FO_C_RES0] = 0.0; c[FO_C_RES1] = 0.0;
  safe[m] = ok ? 1 : 0;
}

uint32_t required_metrics(uint32_t m) {  // metric.py:125-147
  if (m & FO_M_WTTC) m |= FO_M_TTC;
  if (m & FO_M_BE) m |= FO_M_TTC;  // be.py:39 reads results['ttc'] (the reference raises KeyError without it)
  if (m & (FO_M_TTC | FO_M_TTCE | FO_M_BE)) m |= FO_M_DCE;
  if (m & FO_M_HR) m |= FO_M_CP;
  return m;
}

}  // namespace
