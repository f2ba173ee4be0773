// fo_rule_cells.hpp -- what the spawn rule families ask of the step's cell classes and of the lanelet polygons: RuleView (the
// window of class bits, the raster, the map's polygon / topology tables, the frame table) and RuleParams, the class and disc
// predicates, the lane heading, the crossing-number test with its "which lanelet holds this point" queries for a thread, a wave
// and a workgroup, and the small segment / quadrilateral / polyline-sample helpers.  Device code; part of fo_spawn_rules.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "fo_rule_plan.hpp"

namespace {

constexpr double RL_MAX_DIST_OBST = 30.0;          // spawn_locator.py:69
constexpr double RL_MIN_DIST_PED = 5.0;            // :73
constexpr double RL_TOL_SAME_DIR = 20.0 / 180.0 * 3.14159265358979323846;   // :68
constexpr double RL_BUFFER_SIDE = 12.0;            // :70
constexpr double RL_MIN_AREA = 10.0;               // :71
constexpr double RL_AREA_CAR = 9.0, RL_AREA_BIKE = 1.7;   // :72
constexpr int RL_PATHV = 512;                      // vertices of the reference path table held in LDS (longer paths: read from HBM)
constexpr int RL_PVERT = 1024;                     // vertices of a dynamic obstacle's <= 8 candidate lanelet polygons held in LDS

enum { RL_TYPE_CAR = 0, RL_TYPE_BICYCLE = 3, RL_TYPE_PED = 4 };
enum { RL_SRC_DYNAMIC = 1, RL_SRC_STATIC = 2, RL_SRC_LEFT = 3, RL_SRC_RIGHT = 4 };

struct RuleView {
  const uint8_t *cls;       // [ny][nx] class bits of the step (1 road, 2 visible, 4 occluded)
  int ix0, iy0, nx, ny;     // window inside the raster
  double x0, y0, cs;        // raster origin, cell size
  const double *lane_yaw;   // [rny][rnx] or null
  int rnx, rny;
  int P;
  const int32_t *poly_off;
  const double *poly_xy, *poly_box;
  const double *left0;      // [P][2] or null
  const int32_t *pred0, *adj_left;
  int n_inter;
  const int32_t *inter_off, *inter_lanelet;
  const uint8_t *inter_kind;
  const double *path;       // [n_path][6] x, y, s, segment length, tangent x, tangent y (frame 0) | x, y, s, arc length, normal x, y (frame 1)
  int n_path;
  int frame;                // 0 polyline frame, 1 the caller's frame (fo_spawn_rule_params_t::frame)
};

__device__ inline int rl_class_at(const RuleView &v, double x, double y) {
  const int ix = (int)floor((x - v.x0) / v.cs) - v.ix0, iy = (int)floor((y - v.y0) / v.cs) - v.iy0;
  return (ix >= 0 && ix < v.nx && iy >= 0 && iy < v.ny) ? (int)v.cls[(size_t)iy * v.nx + ix] : 0;
}

// classes of the cell squares a disc touches: any has `bit` / all have `bit` (cells outside the window count as class 0)
__device__ inline void rl_disc(const RuleView &v, double x, double y, double rad, int bit, bool &any, bool &all) {
  const int ix0 = (int)floor((x - rad - v.x0) / v.cs) - v.ix0, iy0 = (int)floor((y - rad - v.y0) / v.cs) - v.iy0;
  const int ix1 = (int)floor((x + rad - v.x0) / v.cs) - v.ix0, iy1 = (int)floor((y + rad - v.y0) / v.cs) - v.iy0;
  any = false;
  all = true;
  for (int iy = iy0; iy <= iy1; ++iy)
    for (int ix = ix0; ix <= ix1; ++ix) {
      const double xl = v.x0 + (double)(v.ix0 + ix) * v.cs, yl = v.y0 + (double)(v.iy0 + iy) * v.cs;
      const double qx = fmin(fmax(x, xl), xl + v.cs), qy = fmin(fmax(y, yl), yl + v.cs);
      if ((qx - x) * (qx - x) + (qy - y) * (qy - y) <= rad * rad) {
        const int c = (ix >= 0 && ix < v.nx && iy >= 0 && iy < v.ny) ? (int)v.cls[(size_t)iy * v.nx + ix] : 0;
        if (c & bit) any = true; else all = false;
      }
    }
}
__device__ inline bool rl_disc_touches(const RuleView &v, double x, double y, double rad, int bit) {
  bool any, all;
  rl_disc(v, x, y, rad, bit, any, all);
  return any;
}

__device__ inline bool rl_lane_yaw_at(const RuleView &v, double x, double y, double &yaw) {
  if (!v.lane_yaw) return false;
  const int ix = (int)floor((x - v.x0) / v.cs), iy = (int)floor((y - v.y0) / v.cs);
  if (ix < 0 || ix >= v.rnx || iy < 0 || iy >= v.rny) return false;
  yaw = v.lane_yaw[(size_t)iy * v.rnx + ix];
  return yaw == yaw;
}

// crossing-number test, the rule of the road raster (half-open in y).
// rl_crossing_parity: vertices b .. e-1 of one ring through `get(k)`; the edge arithmetic of the plain loop (xc = xi + (y - yi)
// (xj - xi) / (yj - yi) on the edges that straddle y), with the vertices fetched EIGHT at a time in front of their tests: the
// loop used to be a chain of dependent round trips -- a load, a test, a branch per vertex, ~30 of them per lanelet polygon at
// 0.2-0.5 us each from the L2 -- and every "which lanelet holds this point" of the rule families waited for it (round 6)
// x < xi + (y - yi) (xj - xi) / (yj - yi) for an edge that straddles y (yi != yj) -- the quotient form is the checker's and
// decides whenever it is close; everywhere else the sign of s = (x - xi) d - (y - yi)(xj - xi) against the sign of d = yj - yi
// says the same without the ~40 instructions of a float64 quotient (the listed edges of a band are nearly all straddled by
// some lane of a wave).  The bound: the computed crossing differs from the real one of the rounded differences by
// < 2.01 u |m / d| + u |xc| (u = 2^-53; product, quotient and sum round once each), i.e. |s_real| > 3.01 u |m| + u |d xi|
// decides, and the computed s is within 3.02 u (|t2| + |m|) of s_real; 2^-48 (|t2| + |m| + |d xi|) = 32 u (...) covers both
// with room.  NaNs fail the comparison and take the quotient.
__device__ __forceinline__ bool rl_left_of_crossing(double x, double y, double xi, double yi, double xj, double yj) {
  const double d = yj - yi, m = (y - yi) * (xj - xi), t2 = (x - xi) * d, s = t2 - m;
  if (fabs(s) > 0x1p-48 * (fabs(t2) + fabs(m) + fabs(d * xi))) return (s < 0.0) != (d < 0.0);
  return x < xi + m / d;
}
template <class GET>
__device__ __forceinline__ int rl_crossing_parity(int b, int e, double x, double y, GET get) {
  int c = 0;
  if (e <= b) return 0;   // (an empty ring holds nothing -- and has no last vertex to start from)
  double2 pj = get(e - 1);
  for (int i0 = b; i0 < e; i0 += 8) {
    double2 pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pv[u] = get(i0 + u < e ? i0 + u : e - 1);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + u < e) {
        const double xi = pv[u].x, yi = pv[u].y, xj = pj.x, yj = pj.y;
        if ((yi > y) != (yj > y)) {
          const double xc = xi + (y - yi) * (xj - xi) / (yj - yi);
          if (x < xc) c ^= 1;
        }
        pj = pv[u];
      }
  }
  return c;
}
__device__ inline bool rl_in_polygon(const RuleView &v, int p, double x, double y) {
  const double *bb = v.poly_box + 4 * (size_t)p;
  if (x < bb[0] || x > bb[2] || y < bb[1] || y > bb[3]) return false;
  const int b = v.poly_off[p], e = v.poly_off[p + 1];
  const double2 *xy = (const double2 *)v.poly_xy;
  return rl_crossing_parity(b, e, x, y, [&](int k) { return xy[k]; }) != 0;
}
// the same test by a whole wave (uniform arguments): a lane per edge -- bounding box, offsets and vertices are one round trip each,
// where a thread on its own walks the ring in chunks (1 + 1 + 1 + ceil(n / 8) trips); the edge arithmetic is that of
// rl_crossing_parity, the parity comes from a ballot
__device__ inline bool rl_in_polygon_wave(const RuleView &v, int p, double x, double y) {
  const int lane = threadIdx.x & 63;
  const int b = v.poly_off[p], e = v.poly_off[p + 1];
  const double2 *xy = (const double2 *)v.poly_xy;
  int c = 0;
  for (int i0 = b; i0 < e; i0 += 64) {
    const int i = i0 + lane;
    bool cross = false;
    if (i < e) {
      const double2 pi = xy[i], pj = xy[i == b ? e - 1 : i - 1];
      if ((pi.y > y) != (pj.y > y)) {
        const double xc = pi.x + (y - pi.y) * (pj.x - pi.x) / (pj.y - pi.y);
        cross = x < xc;
      }
    }
    c ^= (int)(__popcll(__ballot(cross)) & 1);
  }
  return c != 0;
}

// "Which lanelets hold these points?" for a workgroup (round 6): nq query points x P lanelets.  Pass A, a thread per (point,
// lanelet): the bounding box -- one round trip -- and the survivors (a handful: a point lies in two or three boxes) go to a list
// in LDS; pass B, a WAVE per survivor: the crossing-number test a lane per edge.  Three round trips and a barrier, where the
// thread-per-pair form took seven trips per test and ran the tests of one thread one after the other (the dynamic rule's set-up
// spent 7 of its 9 us there).  `keep(q, p)`: pairs worth asking at all;
// `act(q, p)`: called by lane 0 of the wave that found point q inside lanelet p -- the callers combine with atomics, so the
// order of the list does not matter.  *n_hits must be 0 on entry (and a barrier passed since); more survivors than the list
// holds: the thread-per-pair form.  Every thread of the workgroup must call; ends with a barrier.
template <class PT, class KEEP, class ACT>
__device__ __forceinline__ void rl_which_lanelets(const RuleView &v, int nq, PT point, KEEP keep, ACT act, int *hits, int cap, int *n_hits) {
  const int tid = threadIdx.x, nth = blockDim.x, wave = tid >> 6, lane = tid & 63, nw = nth >> 6;
  const unsigned total = (unsigned)nq * (unsigned)v.P;
  for (unsigned w = tid; w < total; w += nth) {
    const int q = (int)(w / (unsigned)v.P), p = (int)(w - (unsigned)q * (unsigned)v.P);
    if (!keep(q, p)) continue;
    double x, y;
    point(q, x, y);
    const double *bb = v.poly_box + 4 * (size_t)p;
    if (x < bb[0] || x > bb[2] || y < bb[1] || y > bb[3]) continue;
    const int h = atomicAdd(n_hits, 1);
    if (h < cap) hits[h] = (q << 16) | p;
  }
  __syncthreads();
  const int nh = *n_hits;
  if (nh <= cap && v.P < 65536) {
    for (int h = wave; h < nh; h += nw) {
      const int q = hits[h] >> 16, p = hits[h] & 0xffff;
      double x, y;
      point(q, x, y);
      const bool in = rl_in_polygon_wave(v, p, x, y);
      if (in && lane == 0) act(q, p);
    }
  } else {
    for (unsigned w = tid; w < total; w += nth) {
      const int q = (int)(w / (unsigned)v.P), p = (int)(w - (unsigned)q * (unsigned)v.P);
      if (!keep(q, p)) continue;
      double x, y;
      point(q, x, y);
      if (rl_in_polygon(v, p, x, y)) act(q, p);
    }
  }
  __syncthreads();
}

__device__ inline int rl_lanelet_of(const RuleView &v, double x, double y) {   // first lanelet (list order) holding the point
  for (int p = 0; p < v.P; ++p)
    if (rl_in_polygon(v, p, x, y)) return p;
  return -1;
}

// the same by a whole wave (every lane calls with the same point): lane l tests the lanelets l, l + 64, ...; the first group
// with a hit decides, its lowest lane = the first lanelet in list order.  (One lane walking the list is a chain of dependent
// round trips: bounding box after bounding box.)
__device__ inline int rl_lanelet_of_wave(const RuleView &v, double x, double y) {
  const int lane = threadIdx.x & 63;
  for (int p0 = 0; p0 < v.P; p0 += 64) {
    const int p = p0 + lane;
    const unsigned long long hit = __ballot(p < v.P && rl_in_polygon(v, p, x, y));
    if (hit) return p0 + __builtin_ctzll(hit);
  }
  return -1;
}

// distance between segment ab and a convex quadrilateral c [4][2] (0 if they touch or the segment starts / ends inside)
__device__ inline double rl_pt_seg(double px, double py, double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay, l2 = dx * dx + dy * dy;
  double t = 0.0;
  if (l2 != 0.0) t = fmin(1.0, fmax(0.0, ((px - ax) * dx + (py - ay) * dy) / l2));
  const double qx = px - (ax + t * dx), qy = py - (ay + t * dy);
  return sqrt(qx * qx + qy * qy);
}
__device__ inline bool rl_inside_quad(double px, double py, const double *c) {
  int sgn = 0;
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3;
    const double cr = (c[2 * j] - c[2 * i]) * (py - c[2 * i + 1]) - (c[2 * j + 1] - c[2 * i + 1]) * (px - c[2 * i]);
    if (fabs(cr) > 1e-12) {
      if (sgn == 0) sgn = cr > 0 ? 1 : -1;
      else if ((cr > 0) != (sgn > 0)) return false;
    }
  }
  return true;
}
__device__ inline double rl_seg_rect_distance(double ax, double ay, double bx, double by, const double *c) {
  if (rl_inside_quad(ax, ay, c) || rl_inside_quad(bx, by, c)) return 0.0;
  double best = INFINITY;
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3;
    const double p3x = c[2 * i], p3y = c[2 * i + 1], p4x = c[2 * j], p4y = c[2 * j + 1];
    const double d1x = bx - ax, d1y = by - ay, d2x = p4x - p3x, d2y = p4y - p3y;
    const double den = d1x * d2y - d1y * d2x;
    if (fabs(den) > 1e-14) {
      const double wx = p3x - ax, wy = p3y - ay;
      const double t = (wx * d2y - wy * d2x) / den, u = (wx * d1y - wy * d1x) / den;
      if (t >= 0.0 && t <= 1.0 && u >= 0.0 && u <= 1.0) return 0.0;
    }
    best = fmin(best, fmin(fmin(rl_pt_seg(ax, ay, p3x, p3y, p4x, p4y), rl_pt_seg(bx, by, p3x, p3y, p4x, p4y)),
                           fmin(rl_pt_seg(p3x, p3y, ax, ay, bx, by), rl_pt_seg(p4x, p4y, ax, ay, bx, by))));
  }
  return best;
}

struct RuleParams {
  double ego_x, ego_y, ego_yaw, ego_s, ego_d, s_threshold;
  double ped_width, ped_length;
  int intention;                 // 0 straight ahead, 1 left turn, 2 right turn
  int win_i0, win_i1;            // reference window = path vertices [i0, i1)
  int behind_static, behind_turn, behind_dynamic, max_static, max_dynamic;
  int label_nodes;               // tests (FO_SCENE_RULE_NODES=1): the dynamic rule's connected parts on the lattice nodes, not on the row runs
};

// sample i of a polyline with cumulative lengths cum[] (np.interp on both coordinates); n_s samples, step apart, the
// last one clamped to the end
__device__ inline void rl_sample(const double *px, const double *py, const double *cum, int n, double q, double &x, double &y) {
  if (q >= cum[n - 1]) { x = px[n - 1]; y = py[n - 1]; return; }
  int lo = 0, hi = n - 1;   // largest j with cum[j] <= q
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= q) lo = mid; else hi = mid - 1;
  }
  const double w = cum[lo + 1] - cum[lo];
  x = (px[lo + 1] - px[lo]) / w * (q - cum[lo]) + px[lo];
  y = (py[lo + 1] - py[lo]) / w * (q - cum[lo]) + py[lo];
}

}  // namespace
