// fo_spawn_predict.hpp -- the phantom predictions: the evenly spaced pick of the candidate cells, the heading, one prediction
// slot per wave (straight or along a route; spawn_write_slot, shared with the rule agents of fo_spawn_rules.hpp) and
// fo_spawn_predict_kernel.  Part of the one translation unit fo_scene.hip.
#pragma once
#include "fo_agent_rows.hpp"
#include "fo_scene_rays.hpp"   // PRED_TICK

namespace {

struct SpawnTypes {  // per pattern slot (j % 4): type code, speed, raw dims, inflated dims
  int32_t type[4];
  double speed[4], raw_l[4], raw_w[4], infl_l[4], infl_w[4];
};

// unit normal from (px, py) towards the closest point of the polyline path [N][2], as an angle in [0, 2 pi)
// (agent.py:475-481 + helper_functions.py:38-64); the whole wave calls this, the lanes share the search for the closest
// segment (per lane ascending i, first minimum; across lanes the smallest (d2, i)), the result is wave-uniform
__device__ __forceinline__ double heading_to_curve(int lane, int N, const double *__restrict__ path, double px, double py) {
  double best = INFINITY, qx = px, qy = py;
  int bi = 0x7fffffff;
  for (int i = lane; i + 1 < N; i += 64) {
    const double ax = path[2 * i], ay = path[2 * i + 1], bx = path[2 * i + 2], by = path[2 * i + 3];
    const double ex = bx - ax, ey = by - ay;
    const double l2 = ex * ex + ey * ey;
    double t = 0.0;
    if (l2 > 0.0) {
      t = ((px - ax) * ex + (py - ay) * ey) / l2;
      if (t < 0.0) t = 0.0;
      if (t > 1.0) t = 1.0;
    }
    const double cx = ax + t * ex, cy = ay + t * ey;
    const double d2 = (px - cx) * (px - cx) + (py - cy) * (py - cy);
    if (d2 < best) { best = d2; qx = cx; qy = cy; bi = i; }   // per lane: ascending i, first minimum
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {                    // across lanes: smallest (d2, i) = first minimum
    const double b2 = __shfl_xor(best, off);
    const int i2 = __shfl_xor(bi, off);
    if (b2 < best || (b2 == best && i2 < bi)) { best = b2; bi = i2; }
  }
  // (the winner's closest point from the lane that holds it -- segment i lives in lane i mod 64 -- instead of carrying it
  // through the six exchange steps)
  qx = __shfl(qx, bi & 63);
  qy = __shfl(qy, bi & 63);
  const double vx = qx - px, vy = qy - py;
  const double nn = sqrt(vx * vx + vy * vy);
  double ux = 1.0, uy = 0.0;
  if (nn > 0.0) { ux = vx / nn; uy = vy / nn; }
  double a = atan2(uy, ux);
  if (a < 0.0) a += 2.0 * M_PI;
  return a;
}

// evenly spaced pick of the candidates + heading per phantom: pedestrians -> unit vector to the closest point of the
// ego reference path (agent.py:475-481 + helper_functions.py:38-76); vehicles -> lane heading raster at their cell
// Phantom slot j of the step (the whole wave calls this; every result is wave-uniform): which candidate cell it takes
// -- the candidates at ranks floor(j n / max_agents) when there are more than slots -- its centre and its heading:
// vehicles on a lane follow the lane-heading raster, everything else heads for the closest point of the reference path
// (agent.py:475-481), the lanes sharing the search for the closest path segment.  Returns false for an unused slot.
__device__ __forceinline__ bool spawn_pick(int j, int lane, const int32_t *__restrict__ cand, int n, int nx, double rx0,
                                           double ry0, double cs, int ix0, int iy0, int max_agents, const SpawnTypes &st,
                                           int N, const double *__restrict__ path,
                                           const double *__restrict__ lane_yaw, int rnx, int rny, int &ci, double &px,
                                           double &py, double &a) {
  const int m = n < max_agents ? n : max_agents;
  ci = -1; px = 0.0; py = 0.0; a = 0.0;
  if (j >= m) return false;
  const int pick = (n <= max_agents) ? j : (int)(((long long)j * n) / max_agents);
  ci = cand[pick];
  const int wx = ix0 + ci % nx, wy = iy0 + ci / nx;
  px = rx0 + ((double)wx + 0.5) * cs;
  py = ry0 + ((double)wy + 0.5) * cs;
  const int type = st.type[j & 3];
  a = NAN;
  if (type != FO_TYPE_PEDESTRIAN && lane_yaw && wx >= 0 && wx < rnx && wy >= 0 && wy < rny)
    a = lane_yaw[(size_t)wy * rnx + wx];
  if (isnan(a)) a = heading_to_curve(lane, N, path, px, py);  // wave-uniform
  return true;
}

// route tables of the static map as the prediction kernels read them (fo_scene_set_routes)
struct RouteView {
  int RT = 0;                       // routes per lanelet in the table (0 = no table)
  const int32_t *first = nullptr, *count = nullptr;
  const double *xy = nullptr, *s = nullptr;
};

// where the prediction kernels write: the arrays fo_sweep_set_agents consumes (whole arrays; `slot` indexes them)
struct PredOut {
  double *pos, *yaw, *v, *cov, *shape, *raw;
  int32_t *type, *len;
};

// One prediction slot, written by one wave (every argument wave-uniform):
//   on && ll >= 0 && the lanelet ll has routes -> route r of that lanelet: the reference's min-var(v) Frenet sample (speed
//     held along the route, quintic lateral move to the nearest of d1 in {-0.5, 0, 0.5}; replaces route_planner.py:31-90
//     + frenetix_handler.py + agent.py:283-426); the prediction ends where the route ends;
//   on, otherwise -> r = 0: straight constant velocity along heading a0 (agent.py:451-536), r > 0 empty;
//   !on -> inactive (len = 0).
// table_on (fo_step_run): the slot's rows of the sweep's agent table as well, instead of a launch of fo_prep_agents_kernel
// (same function, same bits: fo_agent_rows.hpp).
__device__ __forceinline__ void spawn_write_slot(int lane, int slot, int r, bool on, double p0x, double p0y, double a0,
                                                 int atype, double spd, double raw_l, double raw_w, double infl_l,
                                                 double infl_w, int ll, const RouteView &rv, int T, double dt, double var0,
                                                 double factor, const PredOut &o, int table_on, const fo_agent_table_t &at, double vpow, double m_obs) {
  double *P = o.pos + (size_t)slot * T * 2, *Y = o.yaw + (size_t)slot * T, *V = o.v + (size_t)slot * T;
  double *C = o.cov + (size_t)slot * T * 4;
  // (what lane k < 64 writes for sample k, kept for the table rows at the end: r_*)
  double r_var = 0.0, r_px = 0.0, r_py = 0.0, r_yaw = 0.0, r_v = 0.0;
  for (int k = lane; k < T; k += 64) {
    const double var = var0 * (k == lane ? vpow : pow(factor, (double)k));  // agent.py:273; vpow = pow(factor, lane), worked out by the caller
    C[4 * k] = var; C[4 * k + 1] = 0.0; C[4 * k + 2] = 0.0; C[4 * k + 3] = var;
    if (k == lane) r_var = var;
  }
  if (lane == 0) {
    o.shape[2 * slot] = infl_l; o.shape[2 * slot + 1] = infl_w;
    o.raw[2 * slot] = raw_l; o.raw[2 * slot + 1] = raw_w;
    o.type[slot] = atype;
  }
  const int RT = rv.RT;
  const bool routed = on && ll >= 0 && r < RT && rv.count[(size_t)ll * RT] > 0;
  int L = 0;
  if (on && !routed && r == 0) {  // straight constant velocity
    const double a = a0;
    const double vx = __builtin_rint(spd * cos(a) * 1000.0) / 1000.0;  // round(v cos psi, 3)  (agent.py:492, Q12)
    const double vy = __builtin_rint(spd * sin(a) * 1000.0) / 1000.0;
    for (int k = lane; k < T; k += 64) {
      const double t = (double)k * dt;
      const double x_ = p0x + t * vx, y_ = p0y + t * vy;
      P[2 * k] = x_; P[2 * k + 1] = y_; Y[k] = a; V[k] = spd;
      if (k == lane) { r_px = x_; r_py = y_; r_yaw = a; r_v = spd; }
    }
    L = T;
  } else if (routed && rv.count[(size_t)ll * RT + r] >= 2) {
    const int nv = rv.count[(size_t)ll * RT + r];
    const double *qg = rv.xy + 2 * (size_t)rv.first[(size_t)ll * RT + r];
    const double *sg = rv.s + rv.first[(size_t)ll * RT + r];
    // a route of up to ROUTE_LDS vertices is read once, into LDS: the per-sample binary search below is then a chain of LDS
    // reads instead of global ones (the kernel is one chain of dependent round trips; this one had six links)
    constexpr int ROUTE_LDS = 256;
    __shared__ double rt_q[2 * ROUTE_LDS], rt_s[ROUTE_LDS];
    const bool staged = nv <= ROUTE_LDS;
    if (staged) {
      for (int i = lane; i < nv; i += 64) { rt_q[2 * i] = qg[2 * i]; rt_q[2 * i + 1] = qg[2 * i + 1]; rt_s[i] = sg[i]; }
      __syncthreads();
    }
    const double px = p0x, py = p0y;
    double s0 = 0.0, d0 = 0.0, d1 = -0.5, s_end = 0.0;
    const double t1 = 3.0;
    auto follow = [&](const double *q, const double *sq) {
    double best = INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i + 1 < nv; i += 64) {  // closest point of the route: per lane ascending i, first minimum
      const double ax = q[2 * i], ay = q[2 * i + 1], ex = q[2 * i + 2] - ax, ey = q[2 * i + 3] - ay;
      const double l2 = ex * ex + ey * ey;
      double t = ((px - ax) * ex + (py - ay) * ey) / l2;
      if (t < 0.0) t = 0.0;
      if (t > 1.0) t = 1.0;
      const double cx = ax + t * ex, cy = ay + t * ey;
      const double d2 = (px - cx) * (px - cx) + (py - cy) * (py - cy);
      if (d2 < best) {
        const double l = sqrt(l2);
        best = d2; bi = i;
        s0 = sq[i] + t * l;
        d0 = ((px - cx) * (-ey) + (py - cy) * ex) / l;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {  // across lanes: smallest (d2, i)
      const double b2 = __shfl_xor(best, off);
      const int i2 = __shfl_xor(bi, off);
      if (b2 < best || (b2 == best && i2 < bi)) { best = b2; bi = i2; }
    }
    s0 = __shfl(s0, bi & 63);   // (from the lane that holds the winning segment)
    d0 = __shfl(d0, bi & 63);
    // the Frenet sample the reference keeps (agent.py:349-379 on the nine samples of frenetix_handler.py:82-105): end speed
    // v0, lateral target d1 = the one of {-0.5, 0, 0.5} nearest to d0 (first of equally near ones), quintic d(t) over 3 s
    d1 = -0.5;
    if (fabs(0.0 - d0) < fabs(d1 - d0)) d1 = 0.0;
    if (fabs(0.5 - d0) < fabs(d1 - d0)) d1 = 0.5;
    s_end = sq[nv - 1];
    for (int k = lane; k < T; k += 64) {
      const double tk = (double)k * dt, sk = s0 + spd * tk;
      if (sk > s_end) continue;
      int lo = 0, hi = nv - 2;  // largest m <= nv-2 with sq[m] <= sk
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sq[mid] <= sk) lo = mid; else hi = mid - 1;
      }
      const int m = lo;
      const double ex = q[2 * m + 2] - q[2 * m], ey = q[2 * m + 3] - q[2 * m + 1];
      const double l = sqrt(ex * ex + ey * ey), ux = ex / l, uy = ey / l, loc = sk - sq[m];
      const double tau = tk < t1 ? tk / t1 : 1.0;
      const double dk = d0 + (d1 - d0) * (tau * tau * tau * (10.0 + tau * (-15.0 + 6.0 * tau)));
      const double dd = (d1 - d0) * (30.0 * tau * tau * (1.0 + tau * (-2.0 + tau))) / t1;
      const double x_ = q[2 * m] + loc * ux + dk * (-uy), y_ = q[2 * m + 1] + loc * uy + dk * ux;
      const double yw_ = atan2(uy, ux) + atan2(dd, spd), v_ = sqrt(spd * spd + dd * dd);
      P[2 * k] = x_; P[2 * k + 1] = y_; Y[k] = yw_; V[k] = v_;
      if (k == lane) { r_px = x_; r_py = y_; r_yaw = yw_; r_v = v_; }
    }
    };
    PRED_TICK(6);
    if (staged) follow(rt_q, rt_s);
    else follow(qg, sg);
    // number of samples on the route: sk is non-decreasing in k, so the valid samples are a prefix
    int cnt = 0;
    for (int k = 0; k < T; ++k) cnt += (s0 + spd * ((double)k * dt) > s_end) ? 0 : 1;
    L = cnt;
  }
  for (int k = lane; k < T; k += 64)
    if (k >= L) { P[2 * k] = 0.0; P[2 * k + 1] = 0.0; Y[k] = 0.0; V[k] = 0.0; }
  if (lane == 0) o.len[slot] = L;
  PRED_TICK(7);
  if (table_on && T <= 64) {
    // the slot's rows of the sweep's agent table from the values just written, a lane per sample (no read-back through
    // memory, one atomic for the agent's longest step)
    fo_agent_sample_t q;
    q.px = r_px; q.py = r_py; q.ppx = __shfl_up(r_px, 1); q.ppy = __shfl_up(r_py, 1); q.yaw = r_yaw; q.v = r_v;
    q.sxx = r_var; q.sxy = 0.0; q.syx = 0.0; q.syy = r_var;
    fo_agent_row_core<true>(lane < T, slot, lane, T, L, q, infl_l, infl_w, raw_l, raw_w, atype, at.ego_mass, at.hlA, at.hwA, at.hc, at.tab,
                            at.cst, at.aint, at.status, at.gen, m_obs);
  } else if (table_on) {
    __threadfence_block();
    __syncthreads();
    for (int k = lane; k < T; k += 64)
      fo_agent_row(slot * T + k, T, o.pos, o.yaw, o.v, o.cov, o.shape, o.raw, o.type, o.len, at.ego_mass, at.hlA, at.hwA, at.hc, at.tab,
                   at.cst, at.aint, at.status, at.gen);
  }
}

// Phantoms sampled in the occluded cells: one wave per prediction slot (j, r), r < R.  A vehicle whose cell lies on a
// lanelet with routes gets one prediction per candidate route; pedestrians / off-lane vehicles / no route table: one
// straight prediction in r = 0.  Slots of agents j >= n are inactive (len = 0).
__global__ __launch_bounds__(64) void fo_spawn_predict_kernel(
    int max_agents, int R, const int32_t *__restrict__ cand, const int32_t *__restrict__ n_cand, double rx0, double ry0,
    double cs, int n_path, const double *__restrict__ path, const double *__restrict__ lane_yaw, SpawnTypes st, int T,
    double dt, double var0, double factor, int nx, int ix0, int iy0, int rnx, int rny,
    const int32_t *__restrict__ lanelet_raster, RouteView rv, int32_t *__restrict__ cell, double *__restrict__ pos0,
    double *__restrict__ yaw0, int32_t *__restrict__ n_out, PredOut o, int table_on, fo_agent_table_t at) {
  const int lane = threadIdx.x;
  const int slot = blockIdx.x, j = slot / R, r = slot % R;
  // the pick of agent j (repeated by each of its R route slots: a few dozen path segments; saves a launch)
  PRED_TICK(0);
  const int n_c = *n_cand;
  // (the covariance growth factor of this lane's sample: a page of arithmetic with no input from memory -- here, under the
  // first round trip of the chain that follows)
  const double vpow = pow(factor, (double)lane);
  const double m_obs = table_on ? fo_obstacle_mass(st.type[j & 3], st.infl_l[j & 3] * st.infl_w[j & 3]) : -1.0;   // (as well)
  int ci;
  double p0x, p0y, a0;
  const bool on = spawn_pick(j, lane, cand, n_c, nx, rx0, ry0, cs, ix0, iy0, max_agents, st, n_path, path, lane_yaw, rnx,
                             rny, ci, p0x, p0y, a0);
  PRED_TICK(4);
  if (r == 0 && lane == 0) {
    cell[j] = ci; pos0[2 * j] = p0x; pos0[2 * j + 1] = p0y; yaw0[j] = a0;
    if (j == 0) *n_out = n_c < max_agents ? n_c : max_agents;
  }
  const int sdx = j & 3;
  int ll = -1;
  if (on && lanelet_raster && st.type[sdx] != FO_TYPE_PEDESTRIAN) {
    const int wx = ix0 + ci % nx, wy = iy0 + ci / nx;
    if (wx >= 0 && wx < rnx && wy >= 0 && wy < rny) ll = lanelet_raster[(size_t)wy * rnx + wx];
  }
  PRED_TICK(5);
  spawn_write_slot(lane, slot, r, on, p0x, p0y, a0, st.type[sdx], st.speed[sdx], st.raw_l[sdx], st.raw_w[sdx], st.infl_l[sdx],
                   st.infl_w[sdx], ll, rv, T, dt, var0, factor, o, table_on, at, vpow, m_obs);
  PRED_TICK(9);
}

}  // namespace
