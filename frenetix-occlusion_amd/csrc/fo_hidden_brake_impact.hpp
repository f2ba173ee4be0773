// fo_hidden_brake_impact.hpp -- the hidden-traffic impact verdict (fo_scene_hidden_brake_impact; DESIGN.md §5.10 "Impact verdict"):
// the worst harm that remains after braking, per candidate -- the speed the ego has left where a braking manoeuvre from one of its
// first B brake starts is hit by a class of hidden road user, priced by that class's harm row -- folded into the two reserved columns
// of the planning step's cost row and its safety flag.  An EXTENSION, not part of the reference.  Included by fo_scene.hip after
// fo_hidden_brake_verdict.hpp (same translation unit, same flags: -ffp-contract=off); it stages with hbu_stage, forms first[c] with
// hbu_first and walks with hbu_walk (fo_hidden_brake_users.hpp, where the bounds reasoning stands).  What the speeds mean per
// trajectory is fo_hidden_impact.hpp's.
//
// Inputs are those of fo_hr_brake_verdict_kernel without commit_min, and harm_limit, rows [C][4] and speed_of [C] (a device buffer:
// the host builds it once per set of users).  The definition stands in include/fo_hip.h.
//   fo_hr_brake_impact_kernel<NC, NK>  the verdict kernel -- its lanes, its grid and its LDS are brake_verdict_group / _per_block /
//                        _blocks / _lds_bytes -- that keeps, next to commit[c], the greatest speed at a hit and the lowest brake
//                        start that attains it per class: a lane visits its b in ascending order, so it updates on `>`; over the G
//                        lanes of a trajectory the larger speed wins by __shfl_xor, on equal speed the lower start.  Lane 0 of each
//                        trajectory evaluates the 2 C logistics, chooses the class, writes the outputs and folds the row.
// v[m][first[c]] is read from the staged V row: first[c] < Lm <= T.  rows and speed_of are read at c < C alone, finite at m < M.
// Every byte of every output is written; of cost and safe only what the definition names.
#pragma once
#include "fo_hidden_brake_verdict.hpp"
#include "fo_hidden_impact.hpp"

namespace {

struct HrBrakeImpactArgs {
  int M, T, G, P, C, B;                 // G lanes per trajectory (power of two, <= 64), P trajectories per workgroup, C classes, B starts
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  const int32_t *len;                   // [M] or null
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;                 // the window
  const int32_t *key0, *key1, *key2;    // [ny][nx] each; those beyond K are null and never read (named members: see HrBrakeUsersArgs)
  const int32_t *qmin0, *qmin1, *qmin2; // [M][T] each
  uint32_t map_of;                      // hbu_map_of
  const double *v, *arc;                // [M][T]
  double a_brake, dt;
  const double *speed_of, *rows;        // [C], [C][4]
  double harm_limit;
  const uint8_t *finite;                // [M] or null (every candidate counts as finite)
  double *cost;                         // [M][FO_NC] or null (both or neither)
  uint8_t *safe;                        // [M] or null
  double *harm;                         // [M][2]
  int32_t *user;                        // [M]
  double *speed;                        // [C][M]
  int32_t *at, *commit, *first;         // [C][M]
};
static_assert(sizeof(HrBrakeImpactArgs) + sizeof(HbThr) <= 4096, "the arguments, map_of and the table fit the kernel-argument segment");

// dynamic LDS: brake_verdict_lds_bytes(T, K, C, B).  The waves-per-SIMD hint: left to itself the allocator takes 99 - 100 registers at
// width 4 and 132 - 134 at width 8 -- one register granule above 5 and 4 waves per SIMD; asked for those it stays within 96 and 128
// without a private segment (DESIGN.md §5.10 "Impact verdict", the kernel table).
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) __attribute__((amdgpu_waves_per_eu(NC == 4 ? 5 : 4))) void fo_hr_brake_impact_kernel(const HrBrakeImpactArgs a, const HbThr thr) {
  extern __shared__ double hbi_rows[];  // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin per map, then thr
  const int G = a.G, T = a.T, B = a.B, nc = a.C, per_block = a.P;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = sub < per_block && m < a.M;
  int32_t *QM = (int32_t *)(hbi_rows + (size_t)per_block * 6 * T);   // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  hbu_stage<NK>(a, hbi_rows, QM, TH, m0, per_block, [&](int t) { return thr.v[t]; });
  __syncthreads();
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hbi_rows + (size_t)row_of * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  int fm[NC];                           // over ALL samples k < Lm, which the lanes of the trajectory split
  hbu_first<NC, NK>(QM + (size_t)row_of * T, (size_t)per_block * T, TH, T, Lm, kl, G, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  int32_t commit[NC], at[NC];           // at: 0x7fffffff = no hit start yet, so that the lower start wins among equal speeds
  double speed[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    commit[c] = 0x7fffffff;
    at[c] = 0x7fffffff;
    speed[c] = -INFINITY;
  }
  const int ends = B < Lm ? B : Lm;     // brake starts with a manoeuvre (Lm = 0 on lanes without a trajectory)
  for (int b = kl; b < ends; b += G) {
    int bf[NC];
    const double vb = V[b];
    const int st = hb_stop_sample(vb, a.a_brake, a.dt, b, Lm);
    hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a.a_brake, st, mk, sb, bf);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (hb_unclear(fm[c], b, bf[c], st)) {
        commit[c] = commit[c] < b ? commit[c] : b;
        // the candidate itself is met at fm[c] <= b, before braking from b changes anything; else the manoeuvre's speed at its hit
        const bool met = fm[c] >= 0 && fm[c] <= b;
        const double u = met ? V[fm[c] < 0 ? 0 : fm[c]] : hb_speed(vb, a.a_brake, a.dt, bf[c], b);
        if (u > speed[c]) {             // (ascending b: strictly above keeps the lowest start; a NaN never wins)
          speed[c] = u;
          at[c] = b;
        }
      }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hb_shfl_min(commit[c], 1, G);       // lanes of a trajectory are G consecutive lanes of one wave
    commit[c] = commit[c] == 0x7fffffff ? -1 : fo_hidden_verdict_commit(commit[c], B);
    for (int o = G >> 1; o >= 1; o >>= 1) {
      const double ws = __shfl_xor(speed[c], o);
      const int wa = __shfl_xor(at[c], o);
      if (ws > speed[c] || (ws == speed[c] && wa < at[c])) {
        speed[c] = ws;
        at[c] = wa;
      }
    }
    if (at[c] == 0x7fffffff) {          // no hit start
      at[c] = -1;
      speed[c] = 0.0;
    }
  }
  if (live && kl == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        const size_t i = (size_t)c * a.M + (size_t)m;
        a.commit[i] = commit[c];
        a.first[i] = fm[c];
        a.speed[i] = speed[c];
        a.at[i] = at[c];
      }
    const bool finite = a.finite ? a.finite[m] != 0 : true;
    const fo_hidden_impact_t r = fo_hidden_impact_classes<NC>(speed, at, nc, a.rows, a.speed_of, finite);
    a.harm[2 * (size_t)m] = r.obst_harm;
    a.harm[2 * (size_t)m + 1] = r.ego_harm;
    a.user[m] = r.user;
    if (a.cost) fo_hidden_impact_fold(r, a.harm_limit, a.cost + (size_t)m * FO_NC, a.safe + m);
  }
}

template <int NC>
void hbi_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeImpactArgs &a, const HbThr &thr) {
  hbu_launch_maps(K, fo_hr_brake_impact_kernel<NC, 1>, fo_hr_brake_impact_kernel<NC, 2>, fo_hr_brake_impact_kernel<NC, 3>,
                  grid, block, lds, s, a, thr);
}

}  // namespace
