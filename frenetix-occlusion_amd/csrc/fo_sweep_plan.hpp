// fo_sweep_plan.hpp -- the launch plan of the sweep as a value: which kernel, agents per wave, horizon split, the phases of
// the tapered grid, chunk count and grid, from the batch shape and the FO_SWEEP_* knobs alone.  Host-only integer
// arithmetic, no HIP header: fo_sweep.hip includes it first (sweep_run, fo_sweep_reserve and fo_sweep_autotune plan through
// it, and the device headers take TILE / WAVES / TC / QWAVES from here), and a host compiler builds it alone
// (tests/test_sweep_plan_cpu.py).
#pragma once
#include <cstddef>

#ifndef FO_TC
#define FO_TC 8      // timesteps per chunk of the two-pass scheme (rows of the per-wave cp buffer)
#endif
#ifndef FO_QWAVES
#define FO_QWAVES 4  // waves per workgroup of the queue kernel (45 KB of LDS -> three workgroups per CU)
#endif

namespace {

constexpr int TILE = 64;   // trajectories per wave
constexpr int WAVES = 4;   // waves per workgroup
constexpr int TC = FO_TC;
constexpr int QWAVES = FO_QWAVES;
constexpr int AGENT_PAD_ROWS = 256;   // spare rows behind the agent table (unclamped row addresses of the queue kernel)

inline int round_up(int v, int q) { return (v + q - 1) / q * q; }
inline int tiles_of(int M) { return round_up(M > 0 ? M : 1, TILE) / TILE; }   // tiles of TILE trajectories (at least one)

// agents per wave in the first phase of the (tapered) grid: long workgroups keep the per-workgroup start-up (table fill,
// cross-wave fold) small, the taper takes care of the end of the launch.  Measured at steady clocks on 10 000 x 256 with
// float32 lists and the default taper: 2 -> 0.585 ms, 3 -> 0.556, 4 -> 0.546, 6 -> 0.552, 8 -> 0.550 (bench.py re-checks
// 1 / 2 / 4 / 8 per batch shape at set-up).
inline int pick_apw(int n_tiles, int A, int wpb) {
  int apw = 8;
  while (apw > 1 && (long)n_tiles * ((A + wpb * apw - 1) / (wpb * apw)) * wpb < 8192) apw >>= 1;
  return apw;
}

// the FO_SWEEP_* environment knobs that change the plan (tuning aids, tests, A/B runs); -1 / false = not set
struct SweepKnobs {
  bool force_generic = false;          // FO_SWEEP_GENERIC=1
  int apw = -1;                        // FO_SWEEP_APW (1..64, anything else is ignored)
  int split = -1;                      // FO_SWEEP_SPLIT: 1 = horizon-split form wherever it can run, 0 = never
  int split_apw = -1;                  // FO_SWEEP_SPLIT_APW (1..16): agents per workgroup of the horizon-split form
  bool has_taper = false;              // FO_SWEEP_TAPER="f0,f1,f2": fraction of the agents per phase ("0" = no taper)
  double taper[3] = {1.0, 0.0, 0.0};
};

struct SweepPlan {
  bool use_queue, split;   // queue kernel (else the generic one); horizon of every agent split over the waves of a workgroup
  int wpb, apw;            // waves per workgroup of the kernel that runs; agents per wave (of the first phase)
  int n_chunks;            // agent chunks per tile = rows of the partial buffer
  int ph_n[3], ph_a[4];    // tapered grid: ph_n[i] chunks of wpb x ph_a[i] agents, the rest of wpb x ph_a[3] (SweepArgs)
  int Mp, n_tiles, grid, block;
};

// M > 0 trajectories x T samples against A agents predicted over Ta samples.  Agents per wave by precedence: pick_apw <
// tuned_apw (fo_sweep_autotune's entry for this shape, 0 = none) < force_apw (fo_sweep_autotune while it measures, 0 = none)
// < FO_SWEEP_APW.
inline SweepPlan plan_sweep(int M, int T, int A, int Ta, int tuned_apw, int force_apw, const SweepKnobs &k) {
  SweepPlan p{};
  p.Mp = round_up(M, TILE);
  p.n_tiles = p.Mp / TILE;
  // (the queue kernel reads agent rows up to index T without clamping: horizons far beyond the predictions' take the generic kernel)
  // (the queue kernel addresses one agent's list rows by 32-bit byte offsets: (T-1) M pairs of float64 must stay under 4 GB)
  p.use_queue = !k.force_generic && (T <= Ta + AGENT_PAD_ROWS - 1 || A == 0) &&
                (size_t)(T > 1 ? T - 1 : 1) * (size_t)M * 16u < ((size_t)1 << 32);
  const int wpb = p.wpb = p.use_queue ? QWAVES : WAVES;
  int apw = pick_apw(p.n_tiles, A, wpb);
  if (tuned_apw > 0) apw = tuned_apw;
  if (force_apw > 0) apw = force_apw;
  if (k.apw >= 1 && k.apw <= 64) apw = k.apw;
  // Small batches: with one agent per wave the grid is n_tiles x A waves; below the 3 072 wave slots of the chip the
  // horizon of every agent is split over the four waves of a workgroup instead (one workgroup per tile and agent).
  p.split = p.use_queue && T <= QWAVES * TC && (k.split >= 0 ? k.split == 1 : (long)p.n_tiles * A < 3072);
  if (p.split) {
    // agents per workgroup of the horizon-split form, one after the other: 1.  (Measured on 2 000 x 32, 1 024 (tile, agent)
    // pairs on 768 resident workgroups: 2 / 3 / 4 agents per workgroup -- one round instead of two -- take 64 / 56 / 81 us
    // against 39: the launch lasts as long as its heaviest workgroup, the agents next to the candidates' path, and those
    // come in pairs.)
    apw = k.split_apw >= 1 && k.split_apw <= 16 ? k.split_apw : 1;
  }
  p.apw = apw;
  // Tapered grid (queue kernel, grids beyond one round of the chip): agents per wave halve from phase to phase down to
  // one -- see SweepArgs::ph_n.  f[]: fraction of the agents per phase.
  for (int i = 0; i < 4; ++i) p.ph_a[i] = apw;
  p.n_chunks = A > 0 ? (p.split ? (A + apw - 1) / apw : (A + wpb * apw - 1) / (wpb * apw)) : 0;
  p.ph_n[0] = p.n_chunks;   // one phase unless tapered below
  if (p.use_queue && !p.split && apw >= 2 && A > 0) {
    double f[3] = {0.85, 0.10, 0.0};
    if (apw >= 8) { f[0] = 0.55; f[1] = 0.25; f[2] = 0.12; }
    if (k.has_taper) {
      for (int i = 0; i < 3; ++i) f[i] = k.taper[i];
      if (f[0] <= 0.0) f[0] = 1.0;
    }
    if ((long)p.n_tiles * p.n_chunks >= 768 && f[0] < 1.0) {
      int left = A, ap = apw;
      p.n_chunks = 0;
      for (int ph = 0; ph < 3; ++ph) {
        p.ph_a[ph] = ap;
        p.ph_n[ph] = (int)(f[ph] * A) / (wpb * ap);
        if (p.ph_n[ph] * wpb * ap > left) p.ph_n[ph] = left / (wpb * ap);
        left -= p.ph_n[ph] * wpb * ap;
        p.n_chunks += p.ph_n[ph];
        ap = ap >= 2 ? ap / 2 : 1;
      }
      p.ph_a[3] = 1;
      p.n_chunks += (left + wpb - 1) / wpb;
    }
  }
  p.grid = (p.n_tiles + 7) / 8 * 8 * p.n_chunks;
  p.block = TILE * wpb;
  return p;
}

// What fo_sweep_reserve sets aside so that no batch of at most max_M trajectories and max_A agents makes sweep_run
// allocate (no knob set): the partial buffer in (tile, chunk) cells of NPS x TILE doubles -- a plan needs n_tiles x
// (n_chunks + 1) of them -- and the rows of the chunk table, of which it needs n_chunks + 1.  A full grid has <= ceil(A / 4)
// + 1 chunks (one agent per wave at worst, the tapered tail one more); a batch below 3 072 (tile, agent) pairs whose
// horizon fits takes the horizon-split form with one chunk per agent, but then tiles x A < 3 072 bounds the product
// (tiles x (A + 2) <= 3 072 + 2 tiles).  The longest horizon does not enter: a batch may always be shorter than it.
// tests/test_sweep_plan_cpu.py holds both functions against plan_sweep.
inline size_t max_chunk_cells(int max_M, int max_A) {
  const size_t tiles = (size_t)tiles_of(max_M);
  const size_t full = ((size_t)(max_A + WAVES - 1) / WAVES + 2) * tiles;
  const size_t split = (3072 + 2 * tiles) < tiles * ((size_t)max_A + 2) ? (3072 + 2 * tiles) : tiles * ((size_t)max_A + 2);
  return full > split ? full : split;
}
inline size_t max_chunk_rows(int max_A) { return (size_t)max_A + 3; }

}  // namespace
