// fo_scene_rays.hpp -- the ray half of the scene stage's chain: ray / segment test, the chunked scan of the occluder soup,
// the fan (directions, sector search), fo_fan_kernel, fo_rays_kernel and the choice of its <SKIP, NW> form (launch_rays).
// Also the trace macros of the tuning builds (FO_PRED_TRACE).  Part of the one translation unit fo_scene.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "fo_ctx.hpp"
#include "fo_prep_traj.hpp"
#include "fo_scene_plan.hpp"
#include "fo_scene_state.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ ray casting
// Ray o + t d against segment a + u (b - a):  denom = d x e,  tn = w x e,  un = w x d  (w = a - o).
// Hit iff denom != 0 and 0 <= tn/denom and 0 <= un/denom <= 1, decided on the signs of the numerators (no division
// on the rejection path); t = tn / denom is formed for hits only.  Same predicate, same operation order as the CPU
// restatement used by the tests, compiled without FMA contraction on both sides.
__device__ __forceinline__ double ray_segment(double ox, double oy, double dx, double dy, double ax, double ay,
                                              double bx, double by) {
  const double ex = bx - ax, ey = by - ay;
  const double denom = dx * ey - dy * ex;
  if (denom == 0.0) return INFINITY;
  const double wx = ax - ox, wy = ay - oy;
  const double tn = wx * ey - wy * ex;
  const double un = wx * dy - wy * dx;
  const bool hit = denom > 0.0 ? (tn >= 0.0 && un >= 0.0 && un <= denom) : (tn <= 0.0 && un <= 0.0 && un >= denom);
  return hit ? tn / denom : INFINITY;
}

// lexicographic (t, id) minimum across the wave
__device__ __forceinline__ void wave_min_hit(double &t, int &id) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double t2 = __shfl_xor(t, off);
    const int id2 = __shfl_xor(id, off);
    if (t2 < t || (t2 == t && id2 < id)) { t = t2; id = id2; }
  }
}

// A wave's share of the occluder soup.  Static pieces come in chunks of 64 consecutive table entries (a lane each, 2 KB
// contiguous per chunk, L2 resident); wave w takes chunks [64 w, 64 w + 64), [64 (w + n_waves), ...).  A chunk is skipped
// -- decided a lane per chunk box, then shared by ballot -- when the box misses the bounding box of the ray segment [o, o + tmax d] or lies
// entirely on one side of the ray's line; both tests carry a margin far above rounding (1e-7 m), so culling never
// changes a result, it only saves the reads (the maps are hundreds of metres wide, a ray reaches tens).
// Obstacle o contributes its four sides with id E + o when it is present and occludes (bicycles do not, Q10).
// SKIP: eskip[e] != 0 marks boundary pieces that cast no shadow this step (rings of the road union enclosed by the
// sensor footprint: the reference walks exterior rings of road ∩ footprint only, sensor_model.py:126-131).
__device__ __forceinline__ bool chunk_culled(const double *__restrict__ box, double ox, double oy, double dx, double dy,
                                             double tmax) {
  const double m = 1e-7;
  const double px = ox + tmax * dx, py = oy + tmax * dy;
  const double sx0 = fmin(ox, px) - m, sx1 = fmax(ox, px) + m, sy0 = fmin(oy, py) - m, sy1 = fmax(oy, py) + m;
  const double bx0 = box[0], by0 = box[1], bx1 = box[2], by1 = box[3];
  if (bx0 > sx1 || bx1 < sx0 || by0 > sy1 || by1 < sy0) return true;
  // signed offsets of the four box corners from the ray's line, scaled by |d| (<= 1.5 r for the settle kernel)
  const double mm = m * (fabs(dx) + fabs(dy)) * 1.0e2;
  const double c00 = dx * (by0 - oy) - dy * (bx0 - ox), c10 = dx * (by0 - oy) - dy * (bx1 - ox);
  const double c01 = dx * (by1 - oy) - dy * (bx0 - ox), c11 = dx * (by1 - oy) - dy * (bx1 - ox);
  if (c00 > mm && c10 > mm && c01 > mm && c11 > mm) return true;
  if (c00 < -mm && c10 < -mm && c01 < -mm && c11 < -mm) return true;
  return false;
}

#ifndef FO_PRED_TRACE
#define FO_PRED_TRACE 0   // tuning builds: wall-clock stamps of one prediction workgroup's phases (fo_debug_pred_ticks, tools/pred_trace.py)
#endif
#if FO_PRED_TRACE
__device__ long long g_pred_ticks[16], g_ray_ticks[16];
#define PRED_TICK(i) do { if (blockIdx.x == FO_PRED_TRACE && threadIdx.x == 0) g_pred_ticks[i] = wall_clock64(); } while (0)
#define RAY_TICK(i) do { if (blockIdx.x == FO_PRED_TRACE && threadIdx.x == 0) g_ray_ticks[i] = wall_clock64(); } while (0)
#define FO_PRED_TRACE_BLOCK FO_PRED_TRACE
#define RAY_NOTE(i, v) do { g_ray_ticks[i] = (long long)(v); } while (0)
#else
#define PRED_TICK(i) do { } while (0)
#define RAY_TICK(i) do { } while (0)
#define FO_PRED_TRACE_BLOCK (-1)
#define RAY_NOTE(i, v) do { } while (0)
#endif

template <bool SKIP>
__device__ __forceinline__ void scan_soup(int E, const double *__restrict__ edges, const double *__restrict__ chunk_box,
                                          const uint8_t *__restrict__ eskip, int O, const double *__restrict__ ocorn,
                                          const uint8_t *__restrict__ oflags, int wave, int n_waves, int lane, double ox,
                                          double oy, double dx, double dy, double tmax, int skip_id, double &best,
                                          int &best_id) {
  const int nc = (E + 63) >> 6;
  for (int cb = wave * 64; cb < nc; cb += n_waves * 64) {
    // a lane per chunk box: one round trip culls 64 chunks; the survivors are then scanned a lane per piece
    const int cc = cb + lane;
    unsigned long long live = __ballot(cc < nc && !chunk_culled(chunk_box + 4 * (size_t)(cc < nc ? cc : 0), ox, oy, dx, dy, tmax));
    if (cb == 0) { RAY_TICK(5); if (threadIdx.x == 0 && blockIdx.x == FO_PRED_TRACE_BLOCK) RAY_NOTE(12, __popcll(live)); }
    while (live) {
      const int c = cb + __builtin_ctzll(live);
      live &= live - 1;
      const int gi = (c << 6) + lane;
      if (gi >= E) continue;
      if (SKIP && eskip[gi]) continue;
      const double *p = edges + 4 * (size_t)gi;
      const double t = ray_segment(ox, oy, dx, dy, p[0], p[1], p[2], p[3]);
      if (t < best || (t == best && gi < best_id)) { best = t; best_id = gi; }
    }
  }
  RAY_TICK(6);
  // obstacle sides, interleaved over the whole workgroup
  for (int k = wave * 64 + lane; k < 4 * O; k += 64 * n_waves) {
    const int o = k >> 2, sd = k & 3, s2 = (sd + 1) & 3;
    if (!((oflags[o] & 1) && (oflags[o] & 2)) || E + o == skip_id) continue;
    const double *c = ocorn + 8 * (size_t)o;
    const int id = E + o;
    const double t = ray_segment(ox, oy, dx, dy, c[2 * sd], c[2 * sd + 1], c[2 * s2], c[2 * s2 + 1]);
    if (t < best || (t == best && id < best_id)) { best = t; best_id = id; }
  }
}

// ------------------------------------------------------------------------------------------------ fan sector
// (DIR: where the unit direction of ray i comes from -- the table the fan kernel wrote, or, inside the launch that is
// still writing that table, the fan's own arithmetic: FanDirs below)
struct TableDirs {
  const double *__restrict__ dirs;
  __device__ __forceinline__ void get(int i, double &cx, double &cy) const { cx = dirs[2 * (size_t)i]; cy = dirs[2 * (size_t)i + 1]; }
};
template <class DIR>
__device__ __forceinline__ int fan_ccw_t(int n_rays, const DIR &D, int i, double rx, double ry) {
  double d0, d1;
  D.get(i == n_rays ? 0 : i, d0, d1);
  const double c = d0 * ry - d1 * rx;
  if (c > 0.0) return 1;
  if (c < 0.0) return 0;
  return (d0 * rx + d1 * ry) > 0.0;
}
template <class DIR>
__device__ int fan_search_t(int n_rays, const DIR &D, int a, int b, double rx, double ry) {
  if (!fan_ccw_t(n_rays, D, a, rx, ry) || fan_ccw_t(n_rays, D, b, rx, ry)) return -1;
  int lo = a, hi = b;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (fan_ccw_t(n_rays, D, mid, rx, ry)) lo = mid; else hi = mid;
  }
  return lo;
}
template <class DIR>
__device__ int fan_sector_t(int n_rays, const DIR &D, int full, double rx, double ry) {
  if (full) {  // thirds: each part spans < pi for every n >= 4 (halves exceed pi by a ray pitch when n is odd)
    const int a = n_rays / 3, b = (2 * n_rays) / 3;
    int s = fan_search_t(n_rays, D, 0, a, rx, ry);
    if (s >= 0) return s;
    s = fan_search_t(n_rays, D, a, b, rx, ry);
    if (s >= 0) return s;
    return fan_search_t(n_rays, D, b, n_rays, rx, ry);
  }
  const int m = (n_rays - 1) / 2;
  const int s = fan_search_t(n_rays, D, 0, m, rx, ry);
  if (s >= 0) return s;
  return fan_search_t(n_rays, D, m, n_rays - 1, rx, ry);
}
__device__ __forceinline__ int fan_ccw(int n_rays, const double *__restrict__ dirs, int i, double rx, double ry) {
  return fan_ccw_t(n_rays, TableDirs{dirs}, i, rx, ry);
}
__device__ int fan_search(int n_rays, const double *__restrict__ dirs, int a, int b, double rx, double ry) {
  return fan_search_t(n_rays, TableDirs{dirs}, a, b, rx, ry);
}
__device__ int fan_sector(int n_rays, const double *__restrict__ dirs, int full, double rx, double ry) {
  return fan_sector_t(n_rays, TableDirs{dirs}, full, rx, ry);
}

// ------------------------------------------------------------------------------------------------ ray fan
// Directions and footprint ranges of the fan about the ego heading, written where the ray and cell kernels read them
// (no host trigonometry, no per-step upload).  Full circle: angle_i = yaw + 2 pi i / n; open fan: n rays from
// yaw - fov/2 to yaw + fov/2 inclusive (sensor_model.py:115-124).  rmax: range of the reference's polygonal footprint
// along the ray -- regular 64-gon with a vertex at world angle 0 (Point.buffer(r)) or the 100-point fan of
// _calc_relevant_sector (:201-209): r cos(d/2) / cos(rel mod d - d/2) with d the angular pitch of the arc points.
// ray i of the fan: unit direction and (want_rmax) the footprint range along it
__device__ __forceinline__ void fan_ray(int i, int n, double yaw, double fov, int full, double r, int polygon, double &cs,
                                        double &sn, double &rm) {
  const double two_pi = 6.283185307179586476925286766559;
  double ang, rel, d;
  if (full) {
    ang = yaw + two_pi * (double)i / (double)n;
    rel = ang;
    d = two_pi / 64.0;
  } else {
    rel = i == n - 1 ? fov : fov * (double)i / (double)(n - 1);
    ang = yaw - 0.5 * fov + rel;
    d = fov / 99.0;
  }
  sincos(ang, &sn, &cs);
  rm = r;
  if (polygon) {
    const double m = rel - d * floor(rel / d);
    rm = r * cos(0.5 * d) / cos(m - 0.5 * d);
  }
}
// unit direction i < 100 of the 100-point half fan (radius 1.5 r) of sensor_model.py:85-87
__device__ __forceinline__ void fan_half_dir(int i, double yaw, double &cs, double &sn) {
  const double two_pi = 6.283185307179586476925286766559;
  const double a = i == 99 ? yaw + 0.25 * two_pi : yaw - 0.25 * two_pi + 0.5 * two_pi * (double)i / 99.0;
  sincos(a, &sn, &cs);
}
__global__ void fo_fan_kernel(int n, double yaw, double fov, int full, double r, int polygon,
                              double *__restrict__ dirs, double *__restrict__ rmax, double *__restrict__ half) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (half && i < 100) {
    double sn, cs;
    fan_half_dir(i, yaw, cs, sn);
    half[2 * i] = cs;
    half[2 * i + 1] = sn;
  }
  if (i >= n) return;
  double sn, cs, rm;
  fan_ray(i, n, yaw, fov, full, r, polygon, cs, sn, rm);
  dirs[2 * i] = cs;
  dirs[2 * i + 1] = sn;
  if (rmax) rmax[i] = rm;
}
// the fan computed inside the ray kernel (fo_step_run: one launch less): every ray workgroup works out its own direction
// and range and leaves them where the later kernels of the step read them
struct FanArgs {
  int on = 0, full = 0, polygon = 0;
  double yaw = 0, fov = 0;
  double *dirs = nullptr, *rmax = nullptr, *half = nullptr;
  // fo_step_t::h_mirror as the device sees it (pinned host memory is mapped): the hit ids and the obstacles' visibility
  // flags are ALSO stored there by the launches that produce them -- posted writes over PCIe, no copy command behind the step
  // (a device-to-host copy of 3 KB is a blit launch of ~5 us); null: no mirror, or one the step copies
  int32_t *hit_host = nullptr;
  uint8_t *vis_host = nullptr;
};
struct FanDirs {   // the direction of ray i by the fan's arithmetic (bit-identical to the table entry)
  int n;
  double yaw, fov;
  int full;
  __device__ __forceinline__ void get(int i, double &cx, double &cy) const {
    double rm;
    fan_ray(i, n, yaw, fov, full, 1.0, 0, cx, cy, rm);
  }
};

// Sector of a uniform full fan (ray i at angle yaw + 2 pi i / n, ray 0 = dirs[0]): a float atan2 of the direction
// rotated back by ray 0 proposes the index, the exact predicate of fan_sector (ccw(i) and not ccw(i + 1)) confirms it
// or moves it by a step -- same answer as the binary search, a fraction of its dependent loads.
__device__ __forceinline__ int fan_sector_uniform(int n_rays, const double *__restrict__ dirs, double rx, double ry) {
  const float c0 = (float)dirs[0], s0 = (float)dirs[1];
  const float fx = (float)rx, fy = (float)ry;
  const float ang = atan2f(fy * c0 - fx * s0, fx * c0 + fy * s0);
  int i = (int)floorf(ang * ((float)n_rays * 0.15915494309189535f));
  if (i < 0) i += n_rays;
  if (i >= n_rays) i -= n_rays;
#pragma unroll 1
  for (int it = 0; it < 3; ++it) {
    const int j = i + 1 == n_rays ? 0 : i + 1;
    const bool a = fan_ccw(n_rays, dirs, i, rx, ry), b = fan_ccw(n_rays, dirs, j, rx, ry);
    if (a && !b) return i;
    if (!a) i = i == 0 ? n_rays - 1 : i - 1; else i = j;
  }
  return fan_sector(n_rays, dirs, 1, rx, ry);
}

// ------------------------------------------------------------------------------------------------ rays + probes
// One launch for the ray fan and the obstacle-visibility probes.  Workgroups [0, n_rays): one ray each, its five
// waves scan interleaved fifths of the soup and the (t, id) minima are combined through LDS.  Workgroups
// [n_rays, n_rays + 5 O): one visibility probe each (obstacle o, probe p: 4 corners + centre; sensor_model.py:59-76
// restated) against the soup with the obstacle itself left out; a visible probe sets vis32[o], which the cell-grid
// kernel turns into the byte flag and clears again for the next step.
// NW: waves per workgroup -- RAY_WAVES, or 1 for maps whose boundary soup is a single group of chunk boxes (<= 64 chunks = 4 096
// pieces: only the first wave of five would have pieces to scan; one-wave workgroups are dispatched five times faster and
// meet no barrier)
template <bool SKIP, int NW>
__global__ __launch_bounds__(64 * NW) void fo_rays_kernel(int E, const double *__restrict__ edges,
                                                                 const double *__restrict__ chunk_box,
                                                                 const uint8_t *__restrict__ eskip, int O,
                                                                 const double *__restrict__ ocorn,
                                                                 const double *__restrict__ ocen,
                                                                 const uint8_t *__restrict__ oflags, double ex, double ey,
                                                                 int n_rays, const double *__restrict__ dirs, double r,
                                                                 const double *__restrict__ rmax, int full,
                                                                 double *__restrict__ range,
                                                                 int32_t *__restrict__ hit_id, double *__restrict__ ring,
                                                                 int32_t *__restrict__ vis32,
                                                                 int32_t *__restrict__ n_amb, FanArgs fan,
                                                                 const fo_prep_args_t prep) {
  __shared__ double sh_t[NW];
  __shared__ int sh_id[NW];
  // Workgroups past the rays and probes (fo_step_run): the sweep's tile table of the candidate trajectories -- independent
  // of the scene, written while this launch leaves most of the chip idle instead of by a launch of its own before the sweep.
  if ((int)blockIdx.x >= n_rays + (vis32 ? 5 * O : 0)) {
    __shared__ double prep_sh[2 * FO_PREP_TZ * (FO_PREP_TILE + 1)];
    const int e = (int)blockIdx.x - (n_rays + (vis32 ? 5 * O : 0));
    fo_prep_traj_block(prep, e % prep.n_tiles, (e / prep.n_tiles) & 1, e / (2 * prep.n_tiles), prep_sh);
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0 && n_amb) *n_amb = 0;  // list of undecided cells of this step (grid kernel)
  if ((int)blockIdx.x < n_rays) {
    const int i = blockIdx.x;
    double dx, dy, rm;
    RAY_TICK(0);
    if (fan.on) {   // (wave-uniform; the same arithmetic as fo_fan_kernel)
      fan_ray(i, n_rays, fan.yaw, fan.fov, fan.full, r, fan.polygon, dx, dy, rm);
      if (!fan.rmax) rm = r;
      if (threadIdx.x == 0) {
        fan.dirs[2 * i] = dx;
        fan.dirs[2 * i + 1] = dy;
        if (fan.rmax) fan.rmax[i] = rm;
      }
      if (fan.half && i == 0)
        for (int k = threadIdx.x; k < 100; k += 64 * NW) {   // (a workgroup may be a single wave)
          double hs, hc;
          fan_half_dir(k, fan.yaw, hc, hs);
          fan.half[2 * k] = hc;
          fan.half[2 * k + 1] = hs;
        }
    } else {
      dx = dirs[2 * i];
      dy = dirs[2 * i + 1];
      rm = rmax ? rmax[i] : r;  // range of the sensor footprint along this ray
    }
    double best = INFINITY;
    int id = 0x7fffffff;
    RAY_TICK(1);
    scan_soup<SKIP>(E, edges, chunk_box, eskip, O, ocorn, oflags, wave, NW, lane, ex, ey, dx, dy, rm, -3, best, id);
    RAY_TICK(2);
    wave_min_hit(best, id);
    RAY_TICK(3);
    if (lane == 0) { sh_t[wave] = best; sh_id[wave] = id; }
    __syncthreads();
    RAY_TICK(4);
    if (threadIdx.x == 0) {
      for (int w = 1; w < NW; ++w)
        if (sh_t[w] < best || (sh_t[w] == best && sh_id[w] < id)) { best = sh_t[w]; id = sh_id[w]; }
      if (!(best <= rm)) { best = rm; id = -1; }
      range[i] = best;
      hit_id[i] = id;
      if (fan.hit_host) fan.hit_host[i] = id;
      // a ray that stops at an obstacle has reached a lit point of its boundary: the obstacle touches the visible area
      // (sensor_model.py:59-76); the probe workgroups below add the obstacles that slip between two rays
      if (id >= E && vis32) atomicOr(&vis32[id - E], 1);
      if (ring) {
        ring[2 * i] = ex + best * dx;
        ring[2 * i + 1] = ey + best * dy;
      }
      RAY_TICK(7);
    }
    return;
  }
  // probe workgroup: obstacle o, probe p (4 corners + centre); all five waves share the soup like a ray workgroup
  const int o = (blockIdx.x - n_rays) / 5, p = (blockIdx.x - n_rays) % 5;
  const bool exists = oflags[o] & 1;
  const double qx = p < 4 ? ocorn[8 * (size_t)o + 2 * p] : ocen[2 * o];
  const double qy = p < 4 ? ocorn[8 * (size_t)o + 2 * p + 1] : ocen[2 * o + 1];
  const double rx = qx - ex, ry = qy - ey;
  const double dist = sqrt(rx * rx + ry * ry);
  bool cand = exists && !(dist > r + 0.01);
  if (cand && dist == 0.0) {
    if (threadIdx.x == 0) atomicOr(&vis32[o], 1);
    return;
  }
  if (cand) {   // (in the fused launch the table of directions is still being written by the ray workgroups)
    const int sec = fan.on ? fan_sector_t(n_rays, FanDirs{n_rays, fan.yaw, fan.fov, fan.full}, full, rx, ry)
                           : fan_sector(n_rays, dirs, full, rx, ry);
    if (sec < 0) cand = false;
  }
  if (!cand) return;  // uniform over the workgroup
  const double dx = rx / dist, dy = ry / dist;
  double best = INFINITY;
  int id = 0x7fffffff;
  scan_soup<SKIP>(E, edges, chunk_box, eskip, O, ocorn, oflags, wave, NW, lane, ex, ey, dx, dy, dist, E + o, best, id);
  wave_min_hit(best, id);
  if (lane == 0) sh_t[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; ++w) best = fmin(best, sh_t[w]);
    double t = best;
    if (!(t <= dist)) t = dist;  // first_hit(..., rmax = dist)
    if (t >= dist - 0.01) atomicOr(&vis32[o], 1);
  }
}

// SKIP: the step passes a hole-skip table; nw: ray_waves() of the step (fo_scene_plan.hpp).  vis32 / n_amb: the probe words
// (null: no probes) and the counter of undecided cells of the workspace
void launch_rays(const StaticMap *m, const fo_step_t &p, int nw, int32_t *vis32, int32_t *n_amb, const FanArgs &fan,
                 const fo_prep_args_t &prep, hipStream_t s) {
  const dim3 grid(p.n_rays + (vis32 ? 5 * p.O : 0) + prep.blocks()), block(64 * nw);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, m->E, m->d_edges, m->d_chunk_box, p.d_edge_skip, p.O, p.d_ocorn, p.d_ocen, p.d_oflags,
                       p.ego_x, p.ego_y, p.n_rays, p.d_dirs, p.r, p.d_rmax, p.full_circle, p.d_range, p.d_hit_id, p.d_ring, vis32, n_amb,
                       fan, prep);
  };
  if (p.d_edge_skip) { if (nw == 1) go(fo_rays_kernel<true, 1>); else go(fo_rays_kernel<true, RAY_WAVES>); }
  else { if (nw == 1) go(fo_rays_kernel<false, 1>); else go(fo_rays_kernel<false, RAY_WAVES>); }
}

}  // namespace
