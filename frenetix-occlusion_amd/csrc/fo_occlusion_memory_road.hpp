// fo_occlusion_memory_road.hpp -- the road metric of the occlusion memory (fo_scene_set_occlusion_memory_road; DESIGN.md
// §5.9 "Road metric").  An EXTENSION, not part of the reference.  Included by fo_scene.hip (same translation unit, same
// flags); launched in place of fo_occlusion_memory_kernel on a step that is not a reset, between the settlement and the
// compaction.
//
// An occluded cell g stays occluded iff the disc test of the Euclidean memory holds (some g + d, dx^2 + dy^2 <= r2, was maybe
// occupied on the previous step) AND a hidden road user could have got there along passable cells: d(g) <= L = isqrt(169 r2),
// d = the cheapest 8-connected path from a cell of P_{k-1} over cells of (P_{k-1} or road), 12 per axis step and 17 per
// diagonal step (§5.10's weights).  A path of cost <= L has at most n = L / 12 steps, so the tile and a halo of n cells decide
// every cell of the tile.  Integers only.
//
// One workgroup (256) per 32 x 32 tile: the tile and its halo staged as uint16 in LDS (0 = source, OMR_OPEN = passable and not
// reached, OMR_WALL = impassable, a border of OMR_WALL so that a neighbour read needs no bounds test), relaxed in LDS -- a lane
// per staged column, a wave's rows slid through registers, all reads of a round before a barrier, all writes after it -- until
// a round changes nothing, at most n rounds, a workgroup-uniform exit.  A value above L is never written.  Lanes run along x:
// coalesced byte loads, and the 16-bit LDS reads of a wave fall on consecutive addresses (two lanes share a dword, which
// broadcasts: no bank conflict).  A workgroup without an occluded cell stages nothing.  Plain vector stores; the only atomics
// are the compaction's per-256-cell counts, lowered once per distinct block a wave's cleared cells fall in.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "fo_hip.h"
#include "fo_scene_plan.hpp"   // OMR_SMALL_N, omr_small

namespace {

constexpr int OMR_TILE = 32;                                   // tile edge
constexpr int OMR_CELLS = OMR_TILE * OMR_TILE / 256;           // tile cells per thread: rows ly + 8 i of column lx
constexpr int OMR_MAX_N = 34;                                  // isqrt(169 * 32^2) / 12
constexpr int OMR_MAX_REGION = OMR_TILE + 2 * OMR_MAX_N;       // staged edge at the cap: 100
// two shapes of the one kernel, chosen by n on the host: OWN staged rows per wave (4 OWN >= R; the rows past R are walls, so
// the unrolled relaxation needs no row test) and NCOL staged columns per lane (64 NCOL >= R)
constexpr int OMR_SMALL_OWN = 16, OMR_LARGE_OWN = 25;   // (OMR_SMALL_N, the largest n of the small shape: fo_scene_plan.hpp)
static_assert(4 * OMR_SMALL_OWN >= OMR_TILE + 2 * OMR_SMALL_N && 4 * OMR_LARGE_OWN >= OMR_MAX_REGION, "every staged row has a wave");
constexpr int OMR_OPEN = 65534, OMR_WALL = 65535;
static_assert(OMR_MAX_N == 416 / 12 && 416 * 416 <= 169 * FO_OCCLUSION_MEMORY_MAX_HALO * FO_OCCLUSION_MEMORY_MAX_HALO &&
                  417 * 417 > 169 * FO_OCCLUSION_MEMORY_MAX_HALO * FO_OCCLUSION_MEMORY_MAX_HALO,
              "n at the longest reach the arming call accepts");
static_assert(OMR_MAX_N >= FO_OCCLUSION_MEMORY_MAX_HALO, "the disc lies inside the staged region (n >= h for every r2)");
static_assert(416 + 17 < OMR_OPEN, "every candidate fits below the two marks");

struct OccMemRoadArgs {
  int r2 = 0, h = 0;          // the disc: D = {dx^2 + dy^2 <= r2}, h = isqrt(r2)
  int L = 0, n = 0;           // isqrt(169 r2) and L / 12 >= h
  int pix0 = 0, piy0 = 0, pnx = 0, pny = 0;
  const uint8_t *prev = nullptr;
  uint8_t *cur = nullptr;
};

// dynamic LDS of a launch: [4 OWN + 2][32 + 2 n + 2] uint16 (5.5 KB at n = 4, 20.8 KB at the cap)
inline size_t occ_mem_road_lds(int n) {
  const size_t own = omr_small(n) ? OMR_SMALL_OWN : OMR_LARGE_OWN;
  return (4 * own + 2) * (size_t)(OMR_TILE + 2 * n + 2) * sizeof(uint16_t);
}

template <int OWN, int NCOL>
__global__ __launch_bounds__(256) void fo_occlusion_memory_road_kernel(const uint8_t *__restrict__ raster, int rnx, int rny,
                                                                       int ix0, int iy0, int nx, int ny,
                                                                       uint8_t *__restrict__ cls, uint8_t *__restrict__ occ_flag,
                                                                       int32_t *__restrict__ blk, OccMemRoadArgs a) {
  extern __shared__ uint16_t s_d[];      // [4 OWN + 2][R + 2], R = 32 + 2 n
  __shared__ int half_w[2 * FO_OCCLUSION_MEMORY_MAX_HALO + 1];   // row dy of D: |dx| <= half_w[dy + h] (-1: empty row)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lx = tid & (OMR_TILE - 1), ly = tid >> 5;
  const int tx0 = blockIdx.x * OMR_TILE, ty0 = blockIdx.y * OMR_TILE;
  const int ix = tx0 + lx;
  uint8_t c[OMR_CELLS];
  bool any_occ = false;
#pragma unroll
  for (int i = 0; i < OMR_CELLS; ++i) {
    const int iy = ty0 + ly + 8 * i;
    c[i] = (ix < nx && iy < ny) ? cls[iy * nx + ix] : 0;
    any_occ |= (c[i] & 4) != 0;
  }
  unsigned hit = 0;                      // bit i: the thread's occluded cell i stays occluded
  if (__syncthreads_or(any_occ)) {
    const int n = a.n, R = OMR_TILE + 2 * n, S = R + 2;
    for (int t = tid; t < (4 * OWN + 2) * S; t += 256) s_d[t] = OMR_WALL;   // the border and the rows past R
    __syncthreads();
    // staged cell (sx, sy) = raster cell (qx0 + sx, qy0 + sy); a wave per row, lanes along x
    const int qx0 = ix0 + tx0 - n, qy0 = iy0 + ty0 - n;
    for (int sy = wave; sy < R; sy += 4) {
      const int qy = qy0 + sy, py = qy - a.piy0;
      for (int sx = lane; sx < R; sx += 64) {
        const int qx = qx0 + sx, px = qx - a.pix0;
        const bool on = qx >= 0 && qx < rnx && qy >= 0 && qy < rny;
        const bool road = on && raster[(size_t)qy * rnx + qx];
        int v;
        if (px >= 0 && px < a.pnx && py >= 0 && py < a.pny) v = a.prev[(size_t)py * a.pnx + px] ? 0 : road ? OMR_OPEN : OMR_WALL;
        else v = road ? 0 : OMR_WALL;                          // (unobserved road is a source)
        s_d[(sy + 1) * S + sx + 1] = (uint16_t)v;
      }
    }
    for (int t = tid; t <= 2 * a.h; t += 256) {
      const int rem = a.r2 - (t - a.h) * (t - a.h);
      int w = -1;
      if (rem >= 0) {                    // integer square root by bisection (rem <= 1024)
        int lo = 0, hi = FO_OCCLUSION_MEMORY_MAX_HALO;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (mid * mid <= rem) lo = mid; else hi = mid - 1;
        }
        w = lo;
      }
      half_w[t] = w;
    }
    __syncthreads();
    // relaxation: wave w owns the staged rows w OWN .. (w + 1) OWN - 1, a lane the columns lane (and lane + 64)
    const int r0 = wave * OWN;
    const int L = a.L;
    for (int round = 0; round < n; ++round) {
      int nv[NCOL][OWN];
      unsigned changed[NCOL];
#pragma unroll
      for (int k = 0; k < NCOL; ++k) {
        changed[k] = 0;
        const int sx = lane + 64 * k;
        if (sx < R) {                    // rows above / at / below the thread's cell, three columns each, slid down the rows
          const uint16_t *p = s_d + r0 * S + sx + 1;           // the row above the first own row, the thread's column
          int al = p[-1], am = p[0], ar = p[1];
          int cl = p[S - 1], cm = p[S], cr = p[S + 1];
#pragma unroll
          for (int i = 0; i < OWN; ++i) {
            p += S;
            const int bl = p[S - 1], bm = p[S], br = p[S + 1];
            int axis = am < bm ? am : bm, diag = al < ar ? al : ar;
            axis = axis < cl ? axis : cl;   diag = diag < bl ? diag : bl;
            axis = axis < cr ? axis : cr;   diag = diag < br ? diag : br;
            axis += 12;                     diag += 17;
            const int cand = axis < diag ? axis : diag;
            const bool take = cm != OMR_WALL && cand < cm && cand <= L;
            nv[k][i] = take ? cand : cm;
            changed[k] |= (unsigned)take << i;
            al = cl; am = cm; ar = cr;
            cl = bl; cm = bm; cr = br;
          }
        }
      }
      __syncthreads();                   // every read of this round is done
      bool any = false;
#pragma unroll
      for (int k = 0; k < NCOL; ++k) {
        if (changed[k]) {
          uint16_t *q = s_d + (r0 + 1) * S + lane + 64 * k + 1;
#pragma unroll
          for (int i = 0; i < OWN; ++i)
            if ((changed[k] >> i) & 1u) q[i * S] = (uint16_t)nv[k][i];
          any = true;
        }
      }
      if (!__syncthreads_or(any)) break;
    }
    // an occluded cell: within L along the road, and a source inside the disc
#pragma unroll
    for (int i = 0; i < OMR_CELLS; ++i) {
      if (!(c[i] & 4)) continue;
      const uint16_t *g = s_d + (n + 1 + ly + 8 * i) * S + n + 1 + lx;
      if (*g > L) continue;
      bool found = false;
      for (int dy = 0; dy <= 2 * a.h && !found; ++dy) {
        const int w = half_w[dy];
        const uint16_t *row = g + (dy - a.h) * S;
        for (int dx = -w; dx <= w; ++dx)
          if (row[dx] == 0) { found = true; break; }
      }
      hit |= (unsigned)found << i;
    }
  }
#pragma unroll
  for (int i = 0; i < OMR_CELLS; ++i) {
    const int iy = ty0 + ly + 8 * i;
    const bool in = ix < nx && iy < ny;
    const int idx = iy * nx + ix;
    const uint8_t H = (c[i] & 2) ? 0 : (c[i] & 4) ? (uint8_t)((hit >> i) & 1u) : (uint8_t)(c[i] & 1);
    if (in) a.cur[idx] = H;
    const bool clear = in && (c[i] & 4) && !H;
    if (clear) {
      cls[idx] = (uint8_t)(c[i] & ~4);
      occ_flag[idx] = 0;
    }
    // a wave is two 32-cell row segments here: one atomic per distinct 256-cell block its cleared cells fall in (at most four)
    unsigned long long m = __ballot(clear);
    while (m) {                          // (wave-uniform)
      const int b = __shfl(idx >> 8, __builtin_ctzll(m));
      const unsigned long long mb = __ballot(clear && (idx >> 8) == b);
      if (lane == 0) atomicSub(&blk[b], __popcll(mb));
      m &= ~mb;
    }
  }
}

}  // namespace
