// fo_occlusion_memory.hpp -- the occlusion memory of the step (an extension): fo_occlusion_memory_kernel (the Euclidean
// disc), and launch_occlusion_memory, which works out the reach and picks between it and the road metric's kernel
// (fo_occlusion_memory_road.hpp).  Part of the one translation unit fo_scene.hip.
#pragma once
#include "fo_occlusion_memory_road.hpp"
#include "fo_scene_plan.hpp"
#include "fo_scene_state.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ occlusion memory
// An extension, not part of the reference: a cell the settled classes call occluded stays occluded only
// if a hidden road user moving at the caller's v_max could have reached it since the previous step, i.e. if some cell
// g + d, d in D = {dx^2 + dy^2 <= r2}, was "maybe occupied" then (P_{k-1}: H of the previous step inside its window, the
// road bit outside it, 0 off the raster).  One thread per window cell on 64 x 4 tiles (a wave = 64 cells of one row); the
// tile's P_{k-1} with a halo of h = floor(sqrt(r2)) <= FO_OCCLUSION_MEMORY_MAX_HALO cells is staged in LDS, and only a
// block with an occluded cell stages it.  Runs after the settle kernel on the same stream and before the compaction:
// every class byte is owned by one thread here, so a plain byte store clears bit 4; the compaction's per-256-cell counts
// are lowered with at most two atomics per wave (a 64-cell row segment spans at most two 256-cell blocks).
constexpr int OM_TX = 64, OM_TY = 4, OM_H = FO_OCCLUSION_MEMORY_MAX_HALO;
struct OccMemArgs {
  int r2 = 0, h = 0, reset = 1;
  int pix0 = 0, piy0 = 0, pnx = 0, pny = 0;
  const uint8_t *prev = nullptr;
  uint8_t *cur = nullptr;
};
__global__ __launch_bounds__(256) void fo_occlusion_memory_kernel(const uint8_t *__restrict__ raster, int rnx, int rny, int ix0,
                                                                  int iy0, int nx, int ny, uint8_t *__restrict__ cls,
                                                                  uint8_t *__restrict__ occ_flag, int32_t *__restrict__ blk,
                                                                  OccMemArgs a) {
  __shared__ uint8_t tile[(OM_TX + 2 * OM_H) * (OM_TY + 2 * OM_H)];
  __shared__ int half_w[2 * OM_H + 1];   // row dy of D: |dx| <= half_w[dy + h] (-1: empty row)
  const int lane = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int ix = blockIdx.x * OM_TX + lane, iy = blockIdx.y * OM_TY + ty;
  const bool in = ix < nx && iy < ny;
  const int idx = iy * nx + ix;
  const uint8_t c = in ? cls[idx] : 0;
  const bool occ = in && (c & 4);
  int hit = 1;   // reset: P_{k-1} = road, and an occluded cell is a road cell with (0, 0) in D
  if (!a.reset && __syncthreads_or(occ)) {   // (a.reset is uniform over the grid)
    const int h = a.h, tw = OM_TX + 2 * h, th = OM_TY + 2 * h;
    const int qx0 = ix0 + blockIdx.x * OM_TX - h, qy0 = iy0 + blockIdx.y * OM_TY - h;   // raster cell of tile[0]
    for (int t = threadIdx.x; t < tw * th; t += 256) {
      const int qx = qx0 + t % tw, qy = qy0 + t / tw;
      const int px = qx - a.pix0, py = qy - a.piy0;
      uint8_t v = 0;
      if (px >= 0 && px < a.pnx && py >= 0 && py < a.pny) v = a.prev[(size_t)py * a.pnx + px];
      else if (qx >= 0 && qx < rnx && qy >= 0 && qy < rny) v = raster[(size_t)qy * rnx + qx] ? 1 : 0;
      tile[t] = v;
    }
    for (int t = threadIdx.x; t <= 2 * h; t += 256) {
      const int rem = a.r2 - (t - h) * (t - h);
      int w = -1;
      if (rem >= 0) {   // integer square root (the float guess corrected both ways)
        w = (int)sqrt((double)rem);
        while (w * w > rem) --w;
        while ((w + 1) * (w + 1) <= rem) ++w;
      }
      half_w[t] = w;
    }
    __syncthreads();
    if (occ) {
      hit = 0;
      for (int dy = 0; dy <= 2 * h && !hit; ++dy) {
        const int w = half_w[dy];
        const uint8_t *row = tile + (ty + dy) * tw + lane + h;
        for (int dx = -w; dx <= w; ++dx)
          if (row[dx]) { hit = 1; break; }
      }
    }
  }
  const uint8_t H = (c & 2) ? 0 : (c & 4) ? (uint8_t)hit : (uint8_t)(c & 1);
  if (in) a.cur[idx] = H;
  const bool clear = occ && !H;
  if (clear) {
    cls[idx] = (uint8_t)(c & ~4);
    occ_flag[idx] = 0;
  }
  const unsigned long long m = __ballot(clear);
  if (m) {   // (wave-uniform)
    const int b0 = __shfl(idx >> 8, __builtin_ctzll(m));
    const unsigned long long m0 = __ballot(clear && (idx >> 8) == b0), m1 = m & ~m0;
    const int b1 = __shfl(idx >> 8, m1 ? __builtin_ctzll(m1) : 0);
    if (lane == 0) {
      atomicSub(&blk[b0], __popcll(m0));
      if (m1) atomicSub(&blk[b1], __popcll(m1));
    }
  }
}

// the armed memory of this step (Scene::om), after the last writer of the classes and before the compaction reads the flags
// and counts: the disc kernel on a reset step (bit-identical in both metrics) or for the Euclidean metric, else the road
// kernel in the form its halo n asks for
void launch_occlusion_memory(const Scene *sc, const fo_step_t &p, hipStream_t s) {
  const fo_occlusion_memory_t &m = sc->om;
  const StaticMap *map = sc->map;
  if (sc->om_road && !m.reset) {
    OccMemRoadArgs a;
    a.r2 = m.r2; a.h = reach_cells(m.r2); a.L = road_reach(m.r2); a.n = road_steps(a.L);
    a.pix0 = m.prev_ix0; a.piy0 = m.prev_iy0; a.pnx = m.prev_nx; a.pny = m.prev_ny; a.prev = m.d_prev; a.cur = m.d_cur;
    const dim3 grid((p.win_nx + OMR_TILE - 1) / OMR_TILE, (p.win_ny + OMR_TILE - 1) / OMR_TILE);
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), occ_mem_road_lds(a.n), s, map->d_raster, map->rnx, map->rny, p.win_ix0, p.win_iy0,
                         p.win_nx, p.win_ny, p.d_cls, sc->d_flags, sc->d_blk, a);
    };
    if (omr_small(a.n)) go(fo_occlusion_memory_road_kernel<OMR_SMALL_OWN, 1>); else go(fo_occlusion_memory_road_kernel<OMR_LARGE_OWN, 2>);
    return;
  }
  OccMemArgs a;
  a.r2 = m.r2; a.reset = m.reset ? 1 : 0; a.cur = m.d_cur;
  if (!a.reset) {
    a.h = reach_cells(m.r2);
    a.pix0 = m.prev_ix0; a.piy0 = m.prev_iy0; a.pnx = m.prev_nx; a.pny = m.prev_ny; a.prev = m.d_prev;
  }
  hipLaunchKernelGGL(fo_occlusion_memory_kernel, dim3((p.win_nx + OM_TX - 1) / OM_TX, (p.win_ny + OM_TY - 1) / OM_TY), dim3(256), 0, s,
                     map->d_raster, map->rnx, map->rny, p.win_ix0, p.win_iy0, p.win_nx, p.win_ny, p.d_cls, sc->d_flags, sc->d_blk, a);
}

}  // namespace
