// fo_occlusion_memory_flow.hpp -- the vehicle layer of the occlusion memory (fo_scene_set_occlusion_memory_vehicles; DESIGN.md
// §5.9 "Vehicle layer"): a second hidden set V next to H, for vehicles that obey the driving direction of the lanes.  An
// EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_reach_flow.hpp (same translation unit, same
// flags; it uses that header's hrf_cand, HRF_ANY and HRF_FAR); one launch directly after the main memory's launch and before the
// compaction, only when armed.
//
// PV_{k-1} = V of the previous step inside its window, the road bit elsewhere on the raster, 0 off it; PassV = PV_{k-1} or
// road.  A step q -> g = q + dir_j is allowed iff PassV(g), bit j is set in out(q) AND in out(g) (the move byte of the map's
// table, 0xFF off the raster: §5.10 "Lane flow", point 3).  d_flow(g) = the cheapest path from a cell of PV_{k-1} over allowed
// steps, 12 per axis step and 17 per diagonal one.  An occluded cell g keeps V(g) = 1 iff some g + d, dx^2 + dy^2 <= r2, lies
// in PV_{k-1} AND d_flow(g) <= L = isqrt(169 r2); a visible cell gives 0, a cell that is neither the road bit.  Integers only.
//
// The kernel runs AFTER the main memory has masked the class bytes, and V <= H cell by cell (every allowed step is a road
// step, r2 is not above the main call's, PV_{k-1} <= P_{k-1}), so it reads H of this step next to the masked byte: H = 0 gives
// V = 0 (visible cells, cells the main memory cleared, cells that are not road), a cell that is still occluded takes the two
// tests above, every other cell with H = 1 keeps 1.  A reset step copies H: V = H of a reset step.
//
// The scheme of fo_occlusion_memory_road_kernel: one workgroup (256) per 32 x 32 tile, the tile and a halo of n = L / 12 <= 34
// cells staged in LDS with a border of "none", a lane per staged column and a wave's rows slid through registers, all reads of
// a round before a barrier and all writes after it, a workgroup-uniform exit when a round changes nothing, at most n rounds, no
// value above L ever written; a workgroup without an occluded cell stages nothing.  What differs: a staged cell is the flow
// band kernel's 32-bit word, the distance in the low 16 bits and out << 16 (an impassable cell and the border carry no bit, so
// no step leads into or out of them and no passable flag is kept), eight separately masked candidates are taken branch-free,
// and a new distance goes back as a 16-bit store into the low half of its word.  Lanes run along x: coalesced byte loads,
// consecutive 32-bit LDS words along a wave (conflict-free).  The kernel writes V only: no class byte, no flag, no count, no
// atomics, plain vector stores.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "fo_hidden_reach_flow.hpp"      // hrf_cand, HRF_ANY, HRF_FAR
#include "fo_occlusion_memory_road.hpp"  // OMR_TILE, OMR_CELLS, OMR_MAX_N, OMR_MAX_REGION
#include "fo_scene_plan.hpp"             // OMF_SMALL_N, omf_small

namespace {

// two shapes of the one kernel, chosen by n on the host, as for the road kernel: OWN staged rows per wave (4 OWN >= R; the rows
// past R carry no bit) and NCOL staged columns per lane (64 NCOL >= R)
constexpr int OMF_SMALL_OWN = 16, OMF_LARGE_OWN = 25;
static_assert(4 * OMF_SMALL_OWN >= OMR_TILE + 2 * OMF_SMALL_N && 4 * OMF_LARGE_OWN >= OMR_MAX_REGION, "every staged row has a wave");
static_assert(64 >= OMR_TILE + 2 * OMF_SMALL_N && 128 >= OMR_MAX_REGION, "every staged column has a lane");
constexpr uint32_t OMF_NONE = 0xFFFFu;                // no distance, no step in or out: the border, an impassable cell
static_assert(416 + 17 < (int)OMF_NONE && (int)OMF_NONE + 17 < HRF_FAR, "every candidate fits below the mark, every barred one above it");

struct OccMemFlowArgs {
  int r2 = 0, h = 0;          // the disc: D = {dx^2 + dy^2 <= r2}, h = isqrt(r2)
  int L = 0, n = 0;           // isqrt(169 r2) and L / 12 >= h
  int reset = 1;
  int pix0 = 0, piy0 = 0, pnx = 0, pny = 0;
  const uint8_t *prev = nullptr;   // V of the previous step
  const uint8_t *hid = nullptr;    // H of THIS step, written by the main memory's launch
  uint8_t *cur = nullptr;          // V of this step
};

// dynamic LDS of a launch: [4 OWN + 2][32 + 2 n + 2] uint32 (11.1 KB at n = 4, 41.6 KB at the cap)
inline size_t occ_mem_flow_lds(int n) {
  const size_t own = omf_small(n) ? OMF_SMALL_OWN : OMF_LARGE_OWN;
  return (4 * own + 2) * (size_t)(OMR_TILE + 2 * n + 2) * sizeof(uint32_t);
}

template <int OWN, int NCOL>
__global__ __launch_bounds__(256) void fo_occlusion_memory_flow_kernel(const uint8_t *__restrict__ raster,
                                                                       const uint8_t *__restrict__ moves, int rnx, int rny,
                                                                       int ix0, int iy0, int nx, int ny,
                                                                       const uint8_t *__restrict__ cls, OccMemFlowArgs a) {
  extern __shared__ uint32_t s_vw[];     // [4 OWN + 2][R + 2], R = 32 + 2 n: distance | out << 16
  __shared__ int half_w[2 * FO_OCCLUSION_MEMORY_MAX_HALO + 1];   // row dy of D: |dx| <= half_w[dy + h] (-1: empty row)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lx = tid & (OMR_TILE - 1), ly = tid >> 5;
  const int tx0 = blockIdx.x * OMR_TILE, ty0 = blockIdx.y * OMR_TILE;
  const int ix = tx0 + lx;
  if (a.reset) {                         // (uniform over the grid) V = H of a reset step
#pragma unroll
    for (int i = 0; i < OMR_CELLS; ++i) {
      const int iy = ty0 + ly + 8 * i;
      if (ix < nx && iy < ny) a.cur[iy * nx + ix] = a.hid[iy * nx + ix];
    }
    return;
  }
  uint8_t hid[OMR_CELLS];
  unsigned occ = 0;                      // bit i: the thread's cell i is still occluded
#pragma unroll
  for (int i = 0; i < OMR_CELLS; ++i) {
    const int iy = ty0 + ly + 8 * i;
    const bool in = ix < nx && iy < ny;
    hid[i] = in ? a.hid[iy * nx + ix] : 0;
    occ |= (unsigned)(in && (cls[iy * nx + ix] & 4)) << i;
  }
  unsigned hit = 0;                      // bit i: the thread's occluded cell i stays in V
  if (__syncthreads_or(occ != 0)) {
    const int n = a.n, R = OMR_TILE + 2 * n, S = R + 2;
    for (int t = tid; t < (4 * OWN + 2) * S; t += 256) s_vw[t] = OMF_NONE;   // the border and the rows past R
    __syncthreads();
    // staged cell (sx, sy) = raster cell (qx0 + sx, qy0 + sy); a wave per row, lanes along x
    const int qx0 = ix0 + tx0 - n, qy0 = iy0 + ty0 - n;
    for (int sy = wave; sy < R; sy += 4) {
      const int qy = qy0 + sy, py = qy - a.piy0;
      for (int sx = lane; sx < R; sx += 64) {
        const int qx = qx0 + sx, px = qx - a.pix0;
        const bool on = qx >= 0 && qx < rnx && qy >= 0 && qy < rny;
        const size_t rc = on ? (size_t)qy * rnx + qx : 0;
        const bool road = on && raster[rc];
        const uint32_t out = on ? moves[rc] : HRF_ANY;
        bool src = road;                                       // (unobserved road is a source)
        if (px >= 0 && px < a.pnx && py >= 0 && py < a.pny) src = a.prev[(size_t)py * a.pnx + px] != 0;
        s_vw[(sy + 1) * S + sx + 1] = src ? out << 16 : road ? OMF_NONE | out << 16 : OMF_NONE;
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
      uint16_t nv[NCOL][OWN];
      unsigned changed[NCOL];
#pragma unroll
      for (int k = 0; k < NCOL; ++k) {
        changed[k] = 0;
        const int sx = lane + 64 * k;
        if (sx < R) {                    // rows below / at / above the thread's cell (y - 1, y, y + 1), three columns each, slid along the rows
          const uint32_t *p = s_vw + r0 * S + sx + 1;          // the row before the first own row, the thread's column
          uint32_t al = p[-1], am = p[0], ar = p[1];
          uint32_t cl = p[S - 1], cm = p[S], cr = p[S + 1];
#pragma unroll
          for (int i = 0; i < OWN; ++i) {
            p += S;
            const uint32_t bl = p[S - 1], bm = p[S], br = p[S + 1];
            const uint32_t mine = cm >> 16;
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
            const bool take = cand < (int)(cm & 0xFFFFu) && cand <= L;
            nv[k][i] = (uint16_t)cand;
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
          uint16_t *q = (uint16_t *)(s_vw + (r0 + 1) * S + lane + 64 * k + 1);   // the low half of the word: the distance
#pragma unroll
          for (int i = 0; i < OWN; ++i)
            if ((changed[k] >> i) & 1u) q[2 * i * S] = nv[k][i];
          any = true;
        }
      }
      if (!__syncthreads_or(any)) break;
    }
    // an occluded cell: within L over allowed steps, and a source inside the disc
#pragma unroll
    for (int i = 0; i < OMR_CELLS; ++i) {
      if (!((occ >> i) & 1u)) continue;
      const uint32_t *g = s_vw + (n + 1 + ly + 8 * i) * S + n + 1 + lx;
      if ((int)(*g & 0xFFFFu) > L) continue;
      bool found = false;
      for (int dy = 0; dy <= 2 * a.h && !found; ++dy) {
        const int w = half_w[dy];
        const uint32_t *row = g + (dy - a.h) * S;
        for (int dx = -w; dx <= w; ++dx)
          if ((row[dx] & 0xFFFFu) == 0) { found = true; break; }
      }
      hit |= (unsigned)found << i;
    }
  }
#pragma unroll
  for (int i = 0; i < OMR_CELLS; ++i) {
    const int iy = ty0 + ly + 8 * i;
    if (ix < nx && iy < ny)
      a.cur[iy * nx + ix] = (uint8_t)(hid[i] && (!((occ >> i) & 1u) || ((hit >> i) & 1u)));
  }
}

// the armed vehicle layer of this step (Scene::ov), directly behind launch_occlusion_memory: H of this step is the main call's
// d_cur, the class bytes are the masked ones
void launch_occlusion_memory_flow(const Scene *sc, const fo_step_t &p, hipStream_t s) {
  const fo_occlusion_memory_t &m = sc->ov;
  const StaticMap *map = sc->map;
  OccMemFlowArgs a;
  a.reset = m.reset ? 1 : 0; a.hid = sc->om.d_cur; a.cur = m.d_cur;
  if (!a.reset) {
    a.r2 = m.r2; a.h = reach_cells(m.r2); a.L = road_reach(m.r2); a.n = road_steps(a.L);
    a.pix0 = m.prev_ix0; a.piy0 = m.prev_iy0; a.pnx = m.prev_nx; a.pny = m.prev_ny; a.prev = m.d_prev;
  }
  const dim3 grid((p.win_nx + OMR_TILE - 1) / OMR_TILE, (p.win_ny + OMR_TILE - 1) / OMR_TILE);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), a.reset ? 0 : occ_mem_flow_lds(a.n), s, map->d_raster, map->d_lane_moves, map->rnx,
                       map->rny, p.win_ix0, p.win_iy0, p.win_nx, p.win_ny, p.d_cls, a);
  };
  if (omf_small(a.n)) go(fo_occlusion_memory_flow_kernel<OMF_SMALL_OWN, 1>); else go(fo_occlusion_memory_flow_kernel<OMF_LARGE_OWN, 2>);
}

}  // namespace
