// fo_hidden_brake_verdict.hpp -- the hidden-traffic fail-safe verdict (fo_scene_hidden_brake_verdict; DESIGN.md §5.10 "Fail-safe
// verdict"): is each candidate still fail-safe against every class of hidden road user from every brake start up to the replanning
// interval -- folded into the two reserved columns of the planning step's cost row and its safety flag.  An EXTENSION, not part of
// the reference.  Included by fo_scene.hip after fo_hidden_brake_users.hpp (same translation unit, same flags: -ffp-contract=off);
// it stages with hbu_stage, forms first[c] with hbu_first and walks with hbu_walk (fo_hidden_brake_users.hpp, where the bounds
// reasoning stands).  What the lanes' commits mean per trajectory is fo_hidden_verdict.hpp's.
//
// Inputs are those of fo_hr_brake_users_kernel, B (the brake starts walked), commit_min, finite [M] and the cost / safe pair.  The
// definition stands in include/fo_hip.h.
//   fo_hr_brake_verdict_kernel<NC, NK>  the users kernel over b < B alone and without brake_first / stop: a lane per (m, b),
//                        G = brake_verdict_group(B) lanes per trajectory (a power of two <= 64: one wave holds them), P =
//                        brake_verdict_per_block(T, K, B) trajectories per workgroup -- LDS caps P, so the lanes from P * G on
//                        stage rows and then have no trajectory.  LDS as in the users kernel: the six rows and the K qmin rows of
//                        each trajectory, then the table (brake_verdict_lds_bytes).  first[c] runs over ALL samples k < Lm (it is
//                        the users entry's), the lanes of a trajectory split them.  commit[c] is the minimum over the G lanes by
//                        __shfl_xor; lane 0 of each trajectory forms the class minimum, writes the outputs and folds the row.
// finite is read at m < M alone.  Every byte of every output is written; of cost and safe only what the definition names.
#pragma once
#include "fo_hidden_brake_users.hpp"
#include "fo_hidden_verdict.hpp"

namespace {

struct HrBrakeVerdictArgs {
  int M, T, G, P, C, B;                 // G lanes per trajectory (power of two, <= 64), P trajectories per workgroup, C classes, B starts
  int commit_min;
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
  const uint8_t *finite;                // [M] or null (every candidate counts as finite)
  double *cost;                         // [M][FO_NC] or null (both or neither)
  uint8_t *safe;                        // [M] or null
  int32_t *fail_safe, *user;            // [M]
  int32_t *commit, *first;              // [C][M]
};
static_assert(sizeof(HrBrakeVerdictArgs) + sizeof(HbThr) <= 4096, "the arguments, map_of and the table fit the kernel-argument segment");

// dynamic LDS: brake_verdict_lds_bytes(T, K, C, B)
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_verdict_kernel(const HrBrakeVerdictArgs a, const HbThr thr) {
  extern __shared__ double hbv_rows[];  // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin per map, then thr
  const int G = a.G, T = a.T, B = a.B, nc = a.C, per_block = a.P;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = sub < per_block && m < a.M;
  int32_t *QM = (int32_t *)(hbv_rows + (size_t)per_block * 6 * T);   // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  hbu_stage<NK>(a, hbv_rows, QM, TH, m0, per_block, [&](int t) { return thr.v[t]; });
  __syncthreads();
  const int row_of = live ? sub : 0;    // (lanes without a trajectory read nothing: Lm = 0; their pointers stay inside the rows)
  const double *X = hbv_rows + (size_t)row_of * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  int fm[NC];                           // over ALL samples k < Lm, which the lanes of the trajectory split
  hbu_first<NC, NK>(QM + (size_t)row_of * T, (size_t)per_block * T, TH, T, Lm, kl, G, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  int32_t commit[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) commit[c] = 0x7fffffff;
  const int ends = B < Lm ? B : Lm;     // brake starts with a manoeuvre (Lm = 0 on lanes without a trajectory)
  for (int b = kl; b < ends; b += G) {
    int bf[NC];
    const double vb = V[b];
    const int st = hb_stop_sample(vb, a.a_brake, a.dt, b, Lm);
    hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a.a_brake, st, mk, sb, bf);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (hb_unclear(fm[c], b, bf[c], st)) commit[c] = commit[c] < b ? commit[c] : b;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hb_shfl_min(commit[c], 1, G);       // lanes of a trajectory are G consecutive lanes of one wave
    commit[c] = commit[c] == 0x7fffffff ? -1 : fo_hidden_verdict_commit(commit[c], B);
  }
  if (live && kl == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) {
        a.commit[(size_t)c * a.M + (size_t)m] = commit[c];
        a.first[(size_t)c * a.M + (size_t)m] = fm[c];
      }
    const bool finite = a.finite ? a.finite[m] != 0 : true;
    const fo_hidden_verdict_t r = fo_hidden_verdict_classes<NC>(commit, nc, B, finite);
    a.fail_safe[m] = r.fail_safe;
    a.user[m] = r.user;
    if (a.cost) fo_hidden_verdict_fold(r, a.commit_min, a.cost + (size_t)m * FO_NC, a.safe + m);
  }
}

template <int NC>
void hbv_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeVerdictArgs &a, const HbThr &thr) {
  hbu_launch_maps(K, fo_hr_brake_verdict_kernel<NC, 1>, fo_hr_brake_verdict_kernel<NC, 2>, fo_hr_brake_verdict_kernel<NC, 3>,
                  grid, block, lds, s, a, thr);
}

}  // namespace
