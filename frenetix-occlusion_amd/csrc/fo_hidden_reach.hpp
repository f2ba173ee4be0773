// fo_hidden_reach.hpp -- hidden-traffic reach forecast (fo_scene_hidden_reach).  An EXTENSION, not part of
// the reference.  Included by fo_scene.hip (same translation unit: the kernels read the static map; same flags:
// -ffp-contract=off, which the footprint test of the trajectory kernel needs).
//
// The hidden set S of this step (the occlusion memory's H_k inside the window, or "not visible and road or occluded" when the
// memory did not run; the road raster outside the window; nothing off the raster) is propagated over the planning horizon
// as a Euclidean reach: sample j of the horizon is reached where the squared cell distance D2 to the nearest source is
// <= R2[j].  Three kernels, integers only in the first two:
//   fo_hr_rows_kernel      a workgroup per row of the window grown by h = isqrt(R2[J-1]) cells: the row's sources as bits of
//                          64-bit words in LDS (one ballot per 64 cells), then a thread per window column finds the nearest
//                          set bit to either side with ctz / clz -> G [ny + 2h][nx] uint8, the distance along the row,
//                          h + 1 where there is no source within h (so that G^2 alone exceeds R2[J-1])
//   fo_hr_cols_kernel      64 columns x 16 rows per workgroup, the tile's G rows with their halo of h rows staged in LDS
//                          (lanes along x: coalesced loads, conflict-free byte reads); a road cell takes
//                          min over |dy| <= h of dy^2 + G(x, y + dy)^2, walking outwards and stopping once dy^2 alone is no
//                          improvement; the arrival step is a binary search of R2[] (LDS copy of the kernel argument)
//   fo_hr_traj_kernel      a lane per pose, lanes along the sample index k (x, y, heading are read contiguously), 64 / G
//                          trajectories per wave with G = the power of two >= min(T, 64); a pose scans the cells of its
//                          rectangle's bounding box (one cell of slack: the float64 point-in-rectangle test decides) and
//                          looks their arrival step up; first / slack are shuffle reductions over the G lanes
// No atomics, no float arithmetic outside the footprint test, every output written with plain vector stores.
// Two pieces are shared with the clearance (fo_hidden_clearance.hpp): fo_hr_cols_kernel is a template whose second instantiation
// stores 169 D2 in place of the arrival step, and the footprint scan of the trajectory kernel is the function fo_hr_scan_footprint.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "fo_hip.h"
#include "fo_scene_state.hpp"

namespace {

constexpr int HR_MAX_J = 254;         // arrival steps are bytes, 255 = never within the horizon
constexpr int HR_THREADS = 256;
constexpr int HR_TX = 64, HR_TY = 16;  // tile of the column pass
constexpr int HR_MAX_EXTENT = FO_HIDDEN_REACH_MAX_HALF_EXTENT;   // cells: bounds the box a pose scans
static_assert(FO_HIDDEN_REACH_MAX_HALO + 1 <= 255, "the row distance (h + 1 = none) is stored in a byte");

struct HrR2 { int32_t v[HR_MAX_J]; };   // the reach table travels as a kernel argument: no transfer, no device buffer

struct HrMapArgs {
  const uint8_t *raster;                // world road raster [rny][rnx]
  int rnx, rny;
  int ix0, iy0, nx, ny;                 // the window
  const uint8_t *cls;                   // [ny][nx] class bytes
  const uint8_t *hidden;                // [ny][nx] H_k or null
  int h, J;
  uint8_t *g;                           // [ny + 2h][nx] row distances (workspace)
  uint8_t *arrival;                     // [ny][nx]
};

// S(q) of world-raster cell (qx, qy)
__device__ __forceinline__ bool fo_hr_source(const HrMapArgs &a, int qx, int qy) {
  const int wx = qx - a.ix0, wy = qy - a.iy0;
  if (wx >= 0 && wx < a.nx && wy >= 0 && wy < a.ny) {
    const size_t i = (size_t)wy * a.nx + wx;
    if (a.hidden) return a.hidden[i] != 0;
    const uint8_t c = a.cls[i];
    return !(c & 2) && (c & 5) != 0;
  }
  if (qx >= 0 && qx < a.rnx && qy >= 0 && qy < a.rny) return a.raster[(size_t)qy * a.rnx + qx] != 0;
  return false;
}

// dynamic LDS: ceil((nx + 2h) / 64) words
__global__ __launch_bounds__(HR_THREADS) void fo_hr_rows_kernel(const HrMapArgs a) {
  extern __shared__ unsigned long long hr_words[];
  const int tid = threadIdx.x, h = a.h;
  const int gw = a.nx + 2 * h, n_words = (gw + 63) >> 6;
  const int row = blockIdx.x;                       // row of the grown window
  const int qy = a.iy0 - h + row;
  for (int p0 = (tid >> 6) << 6; p0 < n_words * 64; p0 += HR_THREADS) {   // (wave-uniform bounds: every lane reaches the ballot)
    const int p = p0 + (tid & 63);
    const bool s = p < gw && fo_hr_source(a, a.ix0 - h + p, qy);
    const unsigned long long m = __ballot(s);
    if ((tid & 63) == 0) hr_words[p0 >> 6] = m;
  }
  __syncthreads();
  for (int x = tid; x < a.nx; x += HR_THREADS) {
    const int p = x + h, wi = p >> 6, b = p & 63;
    int d = h + 1;
    unsigned long long m = hr_words[wi] >> b;       // this cell and the cells to its right in its own word
    if (m) d = __builtin_ctzll(m);
    else
      for (int wj = wi + 1; wj < n_words && (wj << 6) - p <= h; ++wj)
        if ((m = hr_words[wj])) { d = (wj << 6) + __builtin_ctzll(m) - p; break; }
    m = hr_words[wi] << (63 - b);                   // ... and to its left
    int dl = h + 1;
    if (m) dl = __builtin_clzll(m);
    else
      for (int wj = wi - 1; wj >= 0 && p - (wj << 6) - 63 <= h; --wj)
        if ((m = hr_words[wj])) { dl = p - (wj << 6) - 63 + __builtin_clzll(m); break; }
    d = d < dl ? d : dl;
    a.g[(size_t)row * a.nx + x] = (uint8_t)(d > h ? h + 1 : d);
  }
}

struct HrKeyOut {                       // what the clearance's instantiation of the column pass takes in place of the table
  int32_t r2_cap;
  int32_t *key;                         // [ny][nx]: 169 D2 on road cells with D2 <= r2_cap, INT32_MAX elsewhere
};

// The column pass.  Two instantiations: Out = HrR2, the arrival map (binary search of R2[]), and Out = HrKeyOut, the key map
// of fo_hidden_clearance.hpp (169 D2 itself, no table).
// s_r2, J, out (table path) and kout (key path) stay declared at function scope although each instantiation uses only its own:
// written so, Out = HrR2 compiles to the instructions fo_hr_cols_kernel had before it became a template (compared in the
// gfx950 assembly); moving them into the `if constexpr` branches changes its register allocation.  The unused ones are removed
// by the compiler (HrKeyOut: no static LDS).
// dynamic LDS: (HR_TY + 2h) * HR_TX bytes
template <class Out>
__global__ __launch_bounds__(HR_THREADS) void fo_hr_cols_kernel(const HrMapArgs a, const Out r2) {
  constexpr bool KEY = !std::is_same<Out, HrR2>::value;
  extern __shared__ uint8_t hr_tile[];
  __shared__ int32_t s_r2[KEY ? 1 : HR_MAX_J];
  const int tid = threadIdx.x, lane = tid & 63, h = a.h, J = a.J;
  const int x0 = blockIdx.x * HR_TX, y0 = blockIdx.y * HR_TY;
  const int rows = HR_TY + 2 * h;                   // grown rows y0 .. y0 + rows - 1 = window rows y0 - h .. y0 + HR_TY - 1 + h
  const int grows = a.ny + 2 * h;
  if constexpr (!KEY)
    for (int t = tid; t < J; t += HR_THREADS) s_r2[t] = r2.v[t];
  for (int t = tid; t < rows * HR_TX; t += HR_THREADS) {
    const int r = t >> 6, x = x0 + (t & 63);
    hr_tile[t] = (x < a.nx && y0 + r < grows) ? a.g[(size_t)(y0 + r) * a.nx + x] : (uint8_t)(h + 1);
  }
  __syncthreads();
  const int x = x0 + lane;
  if (x >= a.nx) return;
  int r2max;
  if constexpr (KEY) r2max = r2.r2_cap; else r2max = s_r2[J - 1];
  for (int ty = tid >> 6; ty < HR_TY; ty += HR_THREADS / 64) {
    const int y = y0 + ty;
    if (y >= a.ny) break;
    const size_t i = (size_t)y * a.nx + x;
    uint8_t out = 255;
    int32_t kout = 0x7fffffff;
    if (a.cls[i] & 1) {
      const uint8_t *col = hr_tile + (ty + h) * HR_TX + lane;   // G(x, y)
      int best = (int)col[0] * (int)col[0];
      for (int d = 1; d <= h && d * d < best; ++d) {
        const int g0 = col[-d * HR_TX], g1 = col[d * HR_TX];
        const int v0 = d * d + g0 * g0, v1 = d * d + g1 * g1;
        best = best < v0 ? best : v0;
        best = best < v1 ? best : v1;
      }
      if (best <= r2max) {
        if constexpr (KEY) {
          kout = 169 * best;
        } else {                // first j with D2 <= R2[j] (R2 is non-decreasing)
          int lo = 0, hi = J - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (best <= s_r2[mid]) hi = mid; else lo = mid + 1;
          }
          out = (uint8_t)lo;
        }
      }
    }
    if constexpr (KEY) r2.key[i] = kout; else a.arrival[i] = out;
  }
}

struct HrTrajArgs {
  int M, T, G;                          // G lanes per trajectory (power of two, <= 64)
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  const int32_t *len;                   // [M] or null
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;
  const uint8_t *arrival;               // [ny][nx]
  int32_t *cells, *first, *slack;       // [M][T], [M], [M]
};

// The box every footprint scan is clipped to: cells beyond the raster and the window have no arrival step and no key, so a scan
// never leaves their union.  The ONE statement of it: every kernel that scans footprints takes its box from here.
struct HrBox { int lox, loy, hix, hiy; };
template <class Args>
__device__ __forceinline__ HrBox fo_hr_scan_box(const Args &a) {
  const int lox = a.ix0 < 0 ? a.ix0 : 0, loy = a.iy0 < 0 ? a.iy0 : 0;
  const int hix = (a.ix0 + a.nx > a.rnx ? a.ix0 + a.nx : a.rnx) - 1, hiy = (a.iy0 + a.ny > a.rny ? a.iy0 + a.ny : a.rny) - 1;
  return HrBox{lox, loy, hix, hiy};
}

// The footprint of pose i of the trajectory arrays of `a` (HrTrajArgs, or the clearance's / the witness' arguments: the same field
// names): every world-raster cell of the rectangle's bounding box (one cell of slack, clipped to [lox, hix] x [loy, hiy]) whose
// centre passes the float64 point-in-rectangle test gets f(v, gx, gy), v = map[cell] inside the window, outside it 0 on raster
// road and `none` elsewhere, (gx, gy) the cell's raster indices.  Of the box's rows a caller takes row0, row0 + row_step, ...:
// the lanes that share a pose split its rows (fo_hidden_witness.hpp).  The ONE statement of the test on the device: the reach,
// the clearance, the witness and the brake kernel all scan with it.
// fo_hr_scan_pose_rows takes the pose's values (px, py, c, s) themselves: the brake kernel's poses are interpolated, no sample of
// the arrays (fo_hidden_brake.hpp); the forms below hand it the values of sample i.
template <class Args, class V, class F>
__device__ __forceinline__ void fo_hr_scan_pose_rows(const Args &a, double px, double py, double c, double s, const V *__restrict__ map,
                                                     int none, int lox, int loy, int hix, int hiy, int row0, int row_step, F &&f) {
  const double cx = px + a.wb * c, cy = py + a.wb * s;
  const double bx = fabs(c) * a.hl + fabs(s) * a.hw, by = fabs(s) * a.hl + fabs(c) * a.hw;
  const double fx0 = (cx - bx - a.rx0) / a.cs - 0.5, fx1 = (cx + bx - a.rx0) / a.cs - 0.5;
  const double fy0 = (cy - by - a.ry0) / a.cs - 0.5, fy1 = (cy + by - a.ry0) / a.cs - 0.5;
  // NaN compares false: such a pose gets the empty range
  int gx0 = lox, gx1 = lox - 1, gy0 = loy, gy1 = loy - 1;
  if (fx0 <= (double)hix && fx1 >= (double)lox && fy0 <= (double)hiy && fy1 >= (double)loy) {
    gx0 = fx0 > (double)lox ? (int)floor(fx0) - 1 : lox;
    gx1 = fx1 < (double)hix ? (int)ceil(fx1) + 1 : hix;
    gy0 = fy0 > (double)loy ? (int)floor(fy0) - 1 : loy;
    gy1 = fy1 < (double)hiy ? (int)ceil(fy1) + 1 : hiy;
    gx0 = gx0 < lox ? lox : gx0; gx1 = gx1 > hix ? hix : gx1;
    gy0 = gy0 < loy ? loy : gy0; gy1 = gy1 > hiy ? hiy : gy1;
  }
  for (int gy = gy0 + row0; gy <= gy1; gy += row_step) {
    const double ey = (a.ry0 + ((double)gy + 0.5) * a.cs) - cy;
    const int wy = gy - a.iy0;
    const bool row_in = wy >= 0 && wy < a.ny, row_on = gy >= 0 && gy < a.rny;
    for (int gx = gx0; gx <= gx1; ++gx) {
      const double ex = (a.rx0 + ((double)gx + 0.5) * a.cs) - cx;
      const double u = ex * c + ey * s, w = ey * c - ex * s;
      if (!(fabs(u) <= a.hl && fabs(w) <= a.hw)) continue;
      const int wx = gx - a.ix0;
      int v = none;
      if (row_in && wx >= 0 && wx < a.nx) v = map[wy * a.nx + wx];
      else if (row_on && gx >= 0 && gx < a.rnx) v = a.raster[(size_t)gy * a.rnx + gx] ? 0 : none;
      f(v, gx, gy);
    }
  }
}

// the footprint of pose i of the trajectory arrays of `a`.  The heading is loaded first, in statements of its own: written so,
// fo_hr_traj_kernel keeps the load order and the waits it had before the pose form existed (compared in the gfx950 assembly);
// with the four loads as call arguments it waits for all of them before its first multiply.
template <class Args, class V, class F>
__device__ __forceinline__ void fo_hr_scan_footprint_rows(const Args &a, size_t i, const V *__restrict__ map, int none, int lox,
                                                          int loy, int hix, int hiy, int row0, int row_step, F &&f) {
  const double c = a.heading[2 * i], s = a.heading[2 * i + 1];
  fo_hr_scan_pose_rows(a, a.x[i], a.y[i], c, s, map, none, lox, loy, hix, hiy, row0, row_step, f);
}

// every row, the value alone: the scan of a lane that has a pose to itself
template <class Args, class V, class F>
__device__ __forceinline__ void fo_hr_scan_footprint(const Args &a, size_t i, const V *__restrict__ map, int none, int lox, int loy,
                                                     int hix, int hiy, F &&f) {
  fo_hr_scan_footprint_rows(a, i, map, none, lox, loy, hix, hiy, 0, 1, [&](int v, int, int) { f(v); });
}

__global__ __launch_bounds__(HR_THREADS) void fo_hr_traj_kernel(const HrTrajArgs a) {
  const uint8_t *__restrict__ A = a.arrival;   // read through the caches (staged in LDS it was 3.7 x slower)
  const int G = a.G, per_block = HR_THREADS / G;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m = (long long)blockIdx.x * per_block + sub;
  const bool live = m < a.M;
  int Lm = 0;
  if (live) {
    Lm = a.T;
    if (a.len) { const int l = a.len[m]; Lm = l < 0 ? 0 : (l < a.T ? l : a.T); }
  }
  const HrBox sb = fo_hr_scan_box(a);
  int first = 0x7fffffff, slack = 0x7fffffff;
  for (int k = kl; k < a.T; k += G) {
    int n = 0;
    if (live && k < Lm) {
      fo_hr_scan_footprint(a, (size_t)m * a.T + k, A, 255, sb.lox, sb.loy, sb.hix, sb.hiy, [&](int av) {
        if (av != 255) {
          const int d = av - k;
          slack = slack < d ? slack : d;
          n += av <= k;
        }
      });
      if (n > 0 && k < first) first = k;
    }
    if (live) a.cells[(size_t)m * a.T + k] = n;
  }
  for (int o = G >> 1; o > 0; o >>= 1) {            // lanes of a trajectory are G consecutive lanes of one wave
    const int f = __shfl_xor(first, o), sl = __shfl_xor(slack, o);
    first = first < f ? first : f;
    slack = slack < sl ? slack : sl;
  }
  if (live && kl == 0) {
    a.first[m] = first == 0x7fffffff ? -1 : first;
    a.slack[m] = slack;
  }
}

// first half of the distance transform, for the forecast and the clearance alike: the workspace of the row distances and the rows launch
int hr_launch_rows(fo_ctx *ctx, Scene *sc, const HrMapArgs &a, hipStream_t s) {
  if (int rc = fo_reserve(ctx, &sc->d_hr_g, &sc->cap_hr_g, (size_t)(a.ny + 2 * a.h) * a.nx)) return rc;
  HrMapArgs m = a;
  m.g = sc->d_hr_g;
  const size_t lds_rows = (size_t)((a.nx + 2 * a.h + 63) / 64) * sizeof(unsigned long long);
  hipLaunchKernelGGL(fo_hr_rows_kernel, dim3(a.ny + 2 * a.h), dim3(HR_THREADS), lds_rows, s, m);
  return FO_OK;
}

}  // namespace
