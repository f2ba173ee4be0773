// fo_hidden_reach_flow.hpp -- the road metric of the hidden-traffic reach forecast bound to the driving direction of the lanes
// (fo_scene_hidden_reach_flow, fo_scene_hidden_clearance_flow; DESIGN.md §5.10 "Lane flow").  An EXTENSION, not part of the
// reference.  Included by fo_scene.hip after fo_hidden_reach_road.hpp (same translation unit, same flags); it uses that header's
// HRR_* constants and HrMapArgs.
//
// Directions k = 0 .. 7 are the lattice steps E (1,0), NE (1,1), N (0,1), NW (-1,1), W (-1,0), SW (-1,-1), S (0,-1), SE (1,-1):
// step k points at k * 45 degrees.  out(q), a byte per cell of the world raster (the map's move table, built on the host once
// per map: the device computes no angle), has bit k set when a lane-abiding vehicle in q may take step k; 0xFF off the raster.
// A step q -> g = q + dir_k is allowed iff g is passable (the road metric's set, unchanged), bit k is set in out(q) AND in
// out(g): both ends decide.  d_flow(g) = the cheapest path from a source over allowed steps, 12 per axis step and 17 per
// diagonal one, 0 on sources, nothing beyond L[J-1], 65535 = none.  Everything else is the road metric's.  d_flow >= d_road, and
// a table of 0xFF gives d_flow == d_road.  Wrong-way drivers, U-turns and reversing vehicles are outside the model.
//
//   fo_hr_flow_band_kernel  the scheme of fo_hr_road_band_kernel (a workgroup per 32 x 32 tile, a ring of HRR_HALO cells, a
//                           border of "none", a lane per staged column and 16 rows per thread slid through registers, every
//                           read of a round before the barrier and every write after it, a workgroup-uniform exit, the early
//                           return of a tile without a final distance of the band before, no value above min(b B, L[J-1])
//                           ever written); a staged cell is ONE 32-bit LDS word, the distance in its low half and out above
//                           it, so the nine reads a cell makes deliver both, and the relaxation takes eight separately masked
//                           candidates in place of the grouped axis / diagonal minima.  The exactness argument of the bands is
//                           that of the road kernel: relaxation moves one step per round along a path, directed or not.
// Lanes run along x: coalesced loads, consecutive LDS words (no bank conflict).  No atomics, nothing waits for another
// workgroup, every output written with plain vector stores.
#pragma once
#include "fo_hidden_reach_road.hpp"

namespace {

constexpr unsigned HRF_ANY = 0xFFu;                   // every step allowed: off the raster
constexpr int HRF_FAR = 1 << 20;                      // what a step that is not allowed adds: above every cap

struct HrFlowBandArgs {
  HrMapArgs m;                          // (g, arrival, h, J are not read here)
  const uint8_t *moves;                 // [rny][rnx] out(q) of the world raster
  uint16_t *dist;                       // [ny][nx]
  int prev, cap;                        // (b - 1) B and min(b B, L[J-1]) of this launch; prev == 0: the first launch
};

// the distance over step k (weight w) out of the neighbour word nq into a cell whose move byte is `mine`; branch-free: a step that
// is not allowed costs HRF_FAR more
__device__ __forceinline__ int hrf_cand(unsigned nq, unsigned mine, int k, int w) {
  const unsigned barred = ((((nq >> 16) & mine) >> k) & 1u) ^ 1u;
  return (int)(nq & 0xFFFFu) + w + (int)(barred * (unsigned)HRF_FAR);
}

__global__ __launch_bounds__(HR_THREADS) void fo_hr_flow_band_kernel(const HrFlowBandArgs a) {
  __shared__ uint32_t s_w[(HRR_REGION + 2) * HRR_STRIDE];   // distance | out << 16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nx = a.m.nx, ny = a.m.ny;
  const int tx0 = blockIdx.x * HRR_TILE, ty0 = blockIdx.y * HRR_TILE;
  const bool first = a.prev == 0;
  for (int t = tid; t < HRR_STRIDE; t += HR_THREADS) {      // the border: no distance, and no step out of it either
    s_w[t] = HRR_NONE;
    s_w[(HRR_REGION + 1) * HRR_STRIDE + t] = HRR_NONE;
    s_w[t * HRR_STRIDE] = HRR_NONE;
    s_w[t * HRR_STRIDE + HRR_REGION + 1] = HRR_NONE;
  }
  // staged column `lane`, staged rows wave * HRR_OWN ..: window cell (wx, wy0 + i)
  const int wx = tx0 - HRR_HALO + lane, wy0 = ty0 - HRR_HALO + wave * HRR_OWN;
  uint32_t *own = s_w + (wave * HRR_OWN + 1) * HRR_STRIDE + lane + 1;
  const int qx = a.m.ix0 + wx;
  const bool qx_on = qx >= 0 && qx < a.m.rnx;
  unsigned passable = 0;               // bit i: the thread's cell i may take a distance
  bool active = false;                 // a final distance of the band before this one: only next to such a cell anything changes
#pragma unroll
  for (int i = 0; i < HRR_OWN; ++i) {
    const int wy = wy0 + i, qy = a.m.iy0 + wy;
    const bool on_raster = qx_on && qy >= 0 && qy < a.m.rny;
    const size_t rc = on_raster ? (size_t)qy * a.m.rnx + qx : 0;
    const unsigned out = on_raster ? a.moves[rc] : HRF_ANY;
    int v = HRR_NONE;
    if (wx >= 0 && wx < nx && wy >= 0 && wy < ny) {
      const size_t c = (size_t)wy * nx + wx;
      const uint8_t cb = a.m.cls[c];
      const bool src = a.m.hidden ? a.m.hidden[c] != 0 : (!(cb & 2) && (cb & 5) != 0);
      if (src || (cb & 1)) passable |= 1u << i;
      v = first ? (src ? 0 : HRR_NONE) : (int)a.dist[c];
    } else if (on_raster && a.m.raster[rc]) {   // outside the window passable = source: 0 or never
      v = 0;
    }
    own[i * HRR_STRIDE] = (uint32_t)v | out << 16;
    active |= v <= a.prev && v + HRR_BAND > a.prev;
  }
  if (!__syncthreads_or(active)) {
    if (!first) return;                // nothing of the last band in reach: the map keeps what it holds
  } else {
    for (int round = 0; round < HRR_HALO; ++round) {
      // rows below / at / above the thread's cell (y - 1, y, y + 1), three columns each, slid along the thread's rows
      const uint32_t *p = own - HRR_STRIDE;
      unsigned al = p[-1], am = p[0], ar = p[1];
      unsigned cl = p[HRR_STRIDE - 1], cm = p[HRR_STRIDE], cr = p[HRR_STRIDE + 1];
      unsigned nv[HRR_OWN];
      unsigned changed = 0;
#pragma unroll
      for (int i = 0; i < HRR_OWN; ++i) {
        p += HRR_STRIDE;
        const unsigned bl = p[HRR_STRIDE - 1], bm = p[HRR_STRIDE], br = p[HRR_STRIDE + 1];
        const unsigned mine = cm >> 16;
        // the step INTO this cell out of each neighbour: from the west it is E, from the south-west NE, ...
        int cand = hrf_cand(cl, mine, 0, 12);
        int c1 = hrf_cand(al, mine, 1, 17);
        int c2 = hrf_cand(am, mine, 2, 12);
        int c3 = hrf_cand(ar, mine, 3, 17);
        int c4 = hrf_cand(cr, mine, 4, 12);
        int c5 = hrf_cand(br, mine, 5, 17);
        int c6 = hrf_cand(bm, mine, 6, 12);
        int c7 = hrf_cand(bl, mine, 7, 17);
        cand = cand < c1 ? cand : c1;   c2 = c2 < c3 ? c2 : c3;
        c4 = c4 < c5 ? c4 : c5;         c6 = c6 < c7 ? c6 : c7;
        cand = cand < c2 ? cand : c2;   c4 = c4 < c6 ? c4 : c6;
        cand = cand < c4 ? cand : c4;
        const bool take = ((passable >> i) & 1u) && cand < (int)(cm & 0xFFFFu) && cand <= a.cap;
        nv[i] = take ? (cm & 0xFFFF0000u) | (unsigned)cand : cm;
        changed |= (unsigned)take << i;
        al = cl; am = cm; ar = cr;
        cl = bl; cm = bm; cr = br;
      }
      __syncthreads();                  // every read of this round is done
#pragma unroll
      for (int i = 0; i < HRR_OWN; ++i)
        if ((changed >> i) & 1u) own[i * HRR_STRIDE] = nv[i];
      if (!__syncthreads_or(changed != 0)) break;
    }
  }
  for (int t = tid; t < HRR_TILE * HRR_TILE; t += HR_THREADS) {
    const int x = tx0 + (t & (HRR_TILE - 1)), y = ty0 + t / HRR_TILE;
    if (x < nx && y < ny)
      a.dist[(size_t)y * nx + x] =
          (uint16_t)(s_w[(HRR_HALO + 1 + t / HRR_TILE) * HRR_STRIDE + HRR_HALO + 1 + (t & (HRR_TILE - 1))] & 0xFFFFu);
  }
}

// the lane-flow distance up to lmax: the launches of hr_launch_bands, each over the move table
void hr_launch_flow_bands(const HrMapArgs &a, const uint8_t *d_moves, uint16_t *d_dist, int lmax, hipStream_t s) {
  const int bands = reach_bands(lmax);
  const dim3 tiles((a.nx + HRR_TILE - 1) / HRR_TILE, (a.ny + HRR_TILE - 1) / HRR_TILE);
  for (int b = 1; b <= bands; ++b) {
    const HrFlowBandArgs ba{a, d_moves, d_dist, (b - 1) * HRR_BAND, b * HRR_BAND < lmax ? b * HRR_BAND : lmax};
    hipLaunchKernelGGL(fo_hr_flow_band_kernel, tiles, dim3(HR_THREADS), 0, s, ba);
  }
}

}  // namespace
