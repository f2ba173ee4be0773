// fo_hidden_reach_road.hpp -- the road metric of the hidden-traffic reach forecast (fo_scene_hidden_reach_road; DESIGN.md
// §5.10 "Road metric").  An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_reach.hpp (same
// translation unit, same flags); it uses that header's HrMapArgs, fo_hr_source and HR_* constants.
//
// d(g) = the cheapest 8-connected path from a source S(q) to g over passable cells (S or road), 12 per axis step and 17 per
// diagonal step, so that d / 13 never exceeds the Euclidean length of the lattice path.  Integers only.  Two kernels:
//   fo_hr_road_band_kernel     launch b = 1 .. ceil(L[J-1] / B) makes exact every cell with (b - 1) B < d <= b B, B = 12 * HALO:
//                              a workgroup per 32 x 32 tile stages the tile and a ring of HALO cells as uint16 in LDS (cells
//                              outside the window are 0 or 65535 straight from the raster; with b = 1 the window's cells come
//                              from S, later from the distance map), relaxes them to a fixed point -- at most HALO rounds, a
//                              workgroup-uniform exit -- and stores the tile.  A value above min(b B, L[J-1]) is never
//                              written, so every finite value of the map is a final distance at every moment: a neighbouring
//                              tile may store while this one stages, either value it can read is right.  No waiting between
//                              workgroups, no atomics.
//   fo_hr_road_arrival_kernel  a thread per window cell: A_geo = min { j : d <= L[j] } on road cells by binary search of L[] (LDS
//                              copy of the kernel argument), 255 otherwise; arrival = max(arrival, A_geo)
// Lanes run along x everywhere: coalesced loads, and the 16-bit LDS reads of a wave fall on consecutive addresses (two lanes
// share a dword, which broadcasts: no bank conflict).  Every output is written with plain vector stores.
#pragma once
#include "fo_hidden_reach.hpp"
#include "fo_scene_plan.hpp"   // HRR_HALO (ring staged around a tile = steps a band can hold), HRR_BAND = 12 HRR_HALO (B), reach_bands

namespace {

constexpr int HRR_TILE = 32;                         // tile edge
constexpr int HRR_REGION = HRR_TILE + 2 * HRR_HALO;  // staged edge: 64 = the lanes of a wave
constexpr int HRR_STRIDE = HRR_REGION + 2;           // + a border of "none" on every side: a neighbour read needs no bounds test
constexpr int HRR_OWN = HRR_REGION / (HR_THREADS / 64);   // staged rows a wave owns: 16
constexpr int HRR_NONE = 65535;
static_assert(HRR_REGION == 64 && HRR_OWN * (HR_THREADS / 64) == HRR_REGION, "a lane per staged column, whole rows per wave");
static_assert(13 * (FO_HIDDEN_REACH_MAX_HALO + 1) + 17 < HRR_NONE, "every distance within the longest reach fits a uint16");

struct HrRoadBandArgs {
  HrMapArgs m;                          // (g, arrival, h, J are not read here)
  uint16_t *dist;                       // [ny][nx]
  int prev, cap;                        // (b - 1) B and min(b B, L[J-1]) of this launch; prev == 0: the first launch
};

__global__ __launch_bounds__(HR_THREADS) void fo_hr_road_band_kernel(const HrRoadBandArgs a) {
  __shared__ uint16_t s_d[(HRR_REGION + 2) * HRR_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nx = a.m.nx, ny = a.m.ny;
  const int tx0 = blockIdx.x * HRR_TILE, ty0 = blockIdx.y * HRR_TILE;
  const bool first = a.prev == 0;
  for (int t = tid; t < HRR_STRIDE; t += HR_THREADS) {      // the border
    s_d[t] = HRR_NONE;
    s_d[(HRR_REGION + 1) * HRR_STRIDE + t] = HRR_NONE;
    s_d[t * HRR_STRIDE] = HRR_NONE;
    s_d[t * HRR_STRIDE + HRR_REGION + 1] = HRR_NONE;
  }
  // staged column `lane`, staged rows wave * HRR_OWN ..: window cell (wx, wy0 + i)
  const int wx = tx0 - HRR_HALO + lane, wy0 = ty0 - HRR_HALO + wave * HRR_OWN;
  uint16_t *own = s_d + (wave * HRR_OWN + 1) * HRR_STRIDE + lane + 1;
  unsigned passable = 0;               // bit i: the thread's cell i may take a distance
  bool active = false;                 // a final distance of the band before this one: only next to such a cell anything changes
#pragma unroll
  for (int i = 0; i < HRR_OWN; ++i) {
    const int wy = wy0 + i;
    int v = HRR_NONE;
    if (wx >= 0 && wx < nx && wy >= 0 && wy < ny) {
      const size_t c = (size_t)wy * nx + wx;
      const uint8_t cb = a.m.cls[c];
      const bool src = a.m.hidden ? a.m.hidden[c] != 0 : (!(cb & 2) && (cb & 5) != 0);
      if (src || (cb & 1)) passable |= 1u << i;
      v = first ? (src ? 0 : HRR_NONE) : (int)a.dist[c];
    } else {                            // outside the window passable = source: 0 or never
      const int qx = a.m.ix0 + wx, qy = a.m.iy0 + wy;
      if (qx >= 0 && qx < a.m.rnx && qy >= 0 && qy < a.m.rny && a.m.raster[(size_t)qy * a.m.rnx + qx]) v = 0;
    }
    own[i * HRR_STRIDE] = (uint16_t)v;
    active |= v <= a.prev && v + HRR_BAND > a.prev;
  }
  if (!__syncthreads_or(active)) {
    if (!first) return;                // nothing of the last band in reach: the map keeps what it holds
  } else {
    for (int round = 0; round < HRR_HALO; ++round) {
      // rows above / at / below the thread's cell, three columns each, slid down the thread's rows
      const uint16_t *p = own - HRR_STRIDE;
      int al = p[-1], am = p[0], ar = p[1];
      int cl = p[HRR_STRIDE - 1], cm = p[HRR_STRIDE], cr = p[HRR_STRIDE + 1];
      int nv[HRR_OWN];
      unsigned changed = 0;
#pragma unroll
      for (int i = 0; i < HRR_OWN; ++i) {
        p += HRR_STRIDE;
        const int bl = p[HRR_STRIDE - 1], bm = p[HRR_STRIDE], br = p[HRR_STRIDE + 1];
        int axis = am < bm ? am : bm, diag = al < ar ? al : ar;
        axis = axis < cl ? axis : cl;   diag = diag < bl ? diag : bl;
        axis = axis < cr ? axis : cr;   diag = diag < br ? diag : br;
        axis += 12;                     diag += 17;
        const int cand = axis < diag ? axis : diag;
        const bool take = ((passable >> i) & 1u) && cand < cm && cand <= a.cap;
        nv[i] = take ? cand : cm;
        changed |= (unsigned)take << i;
        al = cl; am = cm; ar = cr;
        cl = bl; cm = bm; cr = br;
      }
      __syncthreads();                  // every read of this round is done
#pragma unroll
      for (int i = 0; i < HRR_OWN; ++i)
        if ((changed >> i) & 1u) own[i * HRR_STRIDE] = (uint16_t)nv[i];
      if (!__syncthreads_or(changed != 0)) break;
    }
  }
  for (int t = tid; t < HRR_TILE * HRR_TILE; t += HR_THREADS) {
    const int x = tx0 + (t & (HRR_TILE - 1)), y = ty0 + t / HRR_TILE;
    if (x < nx && y < ny)
      a.dist[(size_t)y * nx + x] = s_d[(HRR_HALO + 1 + t / HRR_TILE) * HRR_STRIDE + HRR_HALO + 1 + (t & (HRR_TILE - 1))];
  }
}

struct HrRoadArrivalArgs {
  const uint8_t *cls;                   // [n]
  const uint16_t *dist;                 // [n]
  uint8_t *arrival;                     // [n]: the Euclidean map in, the later arrival of the two out
  int n, J;
};

__global__ __launch_bounds__(HR_THREADS) void fo_hr_road_arrival_kernel(const HrRoadArrivalArgs a, const HrR2 reach) {
  __shared__ int32_t s_l[HR_MAX_J];
  for (int t = threadIdx.x; t < a.J; t += HR_THREADS) s_l[t] = reach.v[t];
  __syncthreads();
  const int i = blockIdx.x * HR_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const int d = a.dist[i];
  int geo = 255;
  if ((a.cls[i] & 1) && d <= s_l[a.J - 1]) {      // first j with d <= L[j] (L is non-decreasing)
    int lo = 0, hi = a.J - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (d <= s_l[mid]) hi = mid; else lo = mid + 1;
    }
    geo = lo;
  }
  const int e = a.arrival[i];
  a.arrival[i] = (uint8_t)(geo > e ? geo : e);
}

// the road distance up to lmax: a launch per band of B, fixed by the reach alone, nothing is read back (one launch also when the
// reach is 0: the sources)
void hr_launch_bands(const HrMapArgs &a, uint16_t *d_dist, int lmax, hipStream_t s) {
  const int bands = reach_bands(lmax);
  const dim3 tiles((a.nx + HRR_TILE - 1) / HRR_TILE, (a.ny + HRR_TILE - 1) / HRR_TILE);
  for (int b = 1; b <= bands; ++b) {
    const HrRoadBandArgs ba{a, d_dist, (b - 1) * HRR_BAND, b * HRR_BAND < lmax ? b * HRR_BAND : lmax};
    hipLaunchKernelGGL(fo_hr_road_band_kernel, tiles, dim3(HR_THREADS), 0, s, ba);
  }
}

}  // namespace
