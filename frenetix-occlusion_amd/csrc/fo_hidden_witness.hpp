// fo_hidden_witness.hpp -- the route behind a candidate's hidden-traffic finding (fo_scene_hidden_witness; DESIGN.md §5.10
// "Witnesses").  An EXTENSION, not part of the reference.  Included by fo_scene.hip after fo_hidden_reach_flow.hpp (same
// translation unit, same flags: -ffp-contract=off, which the footprint test needs); it uses fo_hr_scan_footprint_rows.
//
// Inputs are the maps of one fo_scene_hidden_reach_road / _flow call (A = d_arrival, d = d_dist) and its d_first.  Per trajectory
// with k* = first >= 0: the conflict cell g* = the footprint cell of sample k* with A <= k* and the smallest (d, gy, gx); then
// the walk back from g* along d -- step k is taken backwards, c -> c - dir_k, when d(c - dir_k) + w_k == d(c) and the move bytes
// of both ends allow k; the direction of the step before is kept when it is among them, else the lowest k -- until d = 0.
//   fo_hr_witness_kernel   eight lanes per trajectory, lane k of a group owning lattice direction k; eight trajectories per wave,
//                          32 per workgroup.  Phase 1: the eight lanes split the rows of the footprint's box (stride 8) and
//                          reduce the key (d, gy, gx) with __shfl_xor over 1, 2, 4.  Phase 2: per round every lane loads d and
//                          out of its own predecessor cell, ONE __ballot tells every group its set K as 8 bits of the mask; no
//                          shuffle, no LDS.  The loop is wave-uniform: it ends after a round in which no group of the wave
//                          stepped, or at path_cap.
//                          Lane 0 of a group stores four direction bytes per dword, the rest of the row is padded with 255 by
//                          the eight lanes together.
// The maps are read through the caches (the access pattern of fo_hr_traj_kernel; a 301 x 301 d map is 181 KB anyway).  Every
// map index is made from a cell that was tested against the window and the raster first: no content of d, A or first can make a
// lane read outside them.  No atomics, no scratch, plain vector stores; every byte of every output is written.
#pragma once
#include "fo_hidden_reach_flow.hpp"

namespace {

static_assert(HW_LANES == 8 && HW_PER_BLOCK * HW_LANES == HR_THREADS, "a lane per lattice direction, 256 threads per workgroup");
constexpr int HW_NO_CELL = (int)0x80000000;         // INT32_MIN: cell / src of a trajectory without a witness
constexpr int HW_D_NONE = 65535;

struct HrWitnessArgs {
  int M, T;
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;                 // the window
  const uint8_t *arrival;               // [ny][nx]
  const uint16_t *dist;                 // [ny][nx]
  const uint8_t *moves;                 // [rny][rnx] out(q), null: every step allowed (the road metric)
  const int32_t *first;                 // [M]
  int path_cap;                         // multiple of 4
  int32_t *cell, *src;                  // [M][2]
  int32_t *steps, *wdist;               // [M]
  uint8_t *dirs;                        // [M][path_cap]
};

// d of world-raster cell (gx, gy): the map inside the window; outside it 0 on raster road, none elsewhere
__device__ __forceinline__ int hw_dist(const HrWitnessArgs &a, int gx, int gy) {
  const int wx = gx - a.ix0, wy = gy - a.iy0;
  if (wx >= 0 && wx < a.nx && wy >= 0 && wy < a.ny) return a.dist[(size_t)wy * a.nx + wx];
  if (gx >= 0 && gx < a.rnx && gy >= 0 && gy < a.rny) return a.raster[(size_t)gy * a.rnx + gx] ? 0 : HW_D_NONE;
  return HW_D_NONE;
}

// out of world-raster cell (gx, gy): the table's byte on the raster, every step off it (and without a table)
__device__ __forceinline__ unsigned hw_out(const HrWitnessArgs &a, int gx, int gy) {
  if (a.moves && gx >= 0 && gx < a.rnx && gy >= 0 && gy < a.rny) return a.moves[(size_t)gy * a.rnx + gx];
  return HRF_ANY;
}

__global__ __launch_bounds__(HR_THREADS) void fo_hr_witness_kernel(const HrWitnessArgs a) {
  const uint8_t *__restrict__ A = a.arrival;
  const int k = threadIdx.x & (HW_LANES - 1);                     // this lane's direction
  const int grp = (threadIdx.x & 63) / HW_LANES;                  // group of the wave: bits 8 grp .. 8 grp + 7 of a ballot
  const long long m = (long long)blockIdx.x * HW_PER_BLOCK + threadIdx.x / HW_LANES;
  const bool live = m < a.M;
  // step k points at k * 45 degrees: E, NE, N, NW, W, SW, S, SE
  const int dx = (k == 0 || k == 1 || k == 7) - (k == 3 || k == 4 || k == 5);
  const int dy = (k == 1 || k == 2 || k == 3) - (k == 5 || k == 6 || k == 7);
  const int w = (k & 1) ? 17 : 12;

  // ---- phase 1: the conflict cell
  int ks = -1;
  if (live) {
    ks = a.first[m];
    if (ks < 0 || ks >= a.T) ks = -1;                             // (a first that is no sample of this batch: no witness)
  }
  int bd = 0x7fffffff, by = 0x7fffffff, bx = 0x7fffffff;          // the smallest (d, gy, gx) of this lane's rows
  if (ks >= 0) {
    const HrBox sb = fo_hr_scan_box(a);
    fo_hr_scan_footprint_rows(a, (size_t)m * a.T + ks, A, 255, sb.lox, sb.loy, sb.hix, sb.hiy, k, HW_LANES, [&](int av, int gx, int gy) {
      if (av <= ks) {
        const int d = hw_dist(a, gx, gy);                         // rows and columns ascend: the first cell of a d stays
        if (d < bd) { bd = d; by = gy; bx = gx; }
      }
    });
  }
#pragma unroll
  for (int o = 1; o < HW_LANES; o <<= 1) {                        // lanes of a trajectory are 8 consecutive lanes of one wave
    const int od = __shfl_xor(bd, o), oy = __shfl_xor(by, o), ox = __shfl_xor(bx, o);
    const bool take = od < bd || (od == bd && (oy < by || (oy == by && ox < bx)));
    if (take) { bd = od; by = oy; bx = ox; }
  }
  const bool found = ks >= 0 && bd != 0x7fffffff;
  int cx = found ? bx : HW_NO_CELL, cy = found ? by : HW_NO_CELL;
  int dc = found ? bd : 0;
  // no witness: steps = -1; a first without a footprint cell that bears it out: not this definition's maps, steps = -2
  int steps = ks < 0 ? -1 : (found ? 0 : -2);
  if (live && k == 0) {
    a.cell[2 * m] = cx;
    a.cell[2 * m + 1] = cy;
    a.wdist[m] = found ? bd : -1;
  }

  // ---- phase 2: the walk
  bool walking = found && dc > 0;
  int prev = -1, i = 0;
  unsigned pack = 0xFFFFFFFFu;
  uint32_t *row = reinterpret_cast<uint32_t *>(a.dirs + (live ? (size_t)m * a.path_cap : 0));
  for (int round = 0; round < a.path_cap; ++round) {
    bool ok = false;
    if (walking) {
      const int px = cx - dx, py = cy - dy;
      const int dp = hw_dist(a, px, py);
      ok = dp != HW_D_NONE && dp + w == dc && ((hw_out(a, px, py) & hw_out(a, cx, cy)) >> k & 1u);
    }
    const unsigned long long all = __ballot(ok);                  // (wave-uniform loop: every lane reaches it)
    const unsigned K = (unsigned)(all >> (HW_LANES * grp)) & 0xFFu;
    if (walking) {
      if (K == 0) {                                               // no predecessor: the maps are not this definition's
        steps = -2;
        walking = false;
      } else {
        const int kt = (prev >= 0 && (K >> prev & 1u)) ? prev : __builtin_ctz(K);
        const int tx = (kt == 0 || kt == 1 || kt == 7) - (kt == 3 || kt == 4 || kt == 5);
        const int ty = (kt == 1 || kt == 2 || kt == 3) - (kt == 5 || kt == 6 || kt == 7);
        cx -= tx; cy -= ty;
        dc -= (kt & 1) ? 17 : 12;                                 // = d of the new cell, by the test above
        prev = kt;
        pack = (pack & ~(0xFFu << (8 * (i & 3)))) | ((unsigned)kt << (8 * (i & 3)));
        ++i;
        if ((i & 3) == 0) {
          if (k == 0) row[(i >> 2) - 1] = pack;
          pack = 0xFFFFFFFFu;
        }
        if (dc == 0) { steps = i; walking = false; }
      }
      if (!walking && (i & 3) != 0 && k == 0) row[i >> 2] = pack; // the last, partly filled dword
    }
    if (!all) break;                                              // nobody stepped: no group of this wave walks any more
  }
  if (walking) steps = -2;                                        // path_cap steps and not at a source (i == path_cap: nothing pending)
  if (live) {
    for (int j = ((i + 3) >> 2) + k; j < (a.path_cap >> 2); j += HW_LANES) row[j] = 0xFFFFFFFFu;
    if (k == 0) {
      a.src[2 * m] = cx;
      a.src[2 * m + 1] = cy;
      a.steps[m] = steps;
    }
  }
}

}  // namespace
