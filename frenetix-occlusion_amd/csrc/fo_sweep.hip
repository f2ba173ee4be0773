// fo_sweep.hip -- the trajectory x agent criticality sweep for gfx950 (MI355X, CDNA4).
//
// One launch evaluates DCE -> TTC/TTCE/WTTC, CP and harm/risk for M candidate trajectories x A agent predictions
// x T timesteps; it replaces M calls of FOInterface.trajectory_safety_assessment
// (ref: interface.py:216-219 -> metrics/metric.py:35-100 -> metrics/{dce,ttc,ttce,wttc,cp,hr}.py).
//
// Mapping (wave64): lane = trajectory (64 consecutive trajectories per wave, trajectory-fastest SoA tile
// [T][6][Mp] so that every per-timestep load/store of a wave is one contiguous 512-byte segment); the agent
// prediction a wave works on is wave-uniform, so its samples come through the scalar cache (s_load) and live
// in SGPRs.  The four waves of a workgroup share one trajectory tile (L1/L2 reuse) and take different agents;
// workgroups that share a tile are placed on the same XCD (blockIdx % 8) so the tile stays in that XCD's L2.
// No MFMA: this is branchy fp64 geometry + transcendentals, not a contraction.
//
// Arithmetic is float64 throughout (the reference is numpy float64; np.round(d,3) at dce.py:79 turns 1e-7
// errors into 1e-3 jumps, see DESIGN.md "Why fp64").
#include <hip/hip_runtime.h>
#include <math.h>
#include <cstdlib>
#include <type_traits>
#include "fo_ctx.hpp"
#include "fo_agent_rows.hpp"
#include "fo_prep_traj.hpp"
#include "fo_sweep_plan.hpp"
#include "fo_verdict.hpp"
#include "fo_sweep_common.hpp"
#include "fo_sweep_generic.hpp"
#include "fo_sweep_queue.hpp"
#include "fo_sweep_be_reduce.hpp"

namespace {

// one instantiation of the queue kernel per output mode: cost vectors only / + pair scalars / + float64 or float32 lists
template <bool ALLM, bool SPLIT>
void launch_queue(int lst, bool pair, dim3 g, dim3 b, hipStream_t s, const SweepArgs &a) {
  if (lst == LST_F64) hipLaunchKernelGGL((fo_sweep_queue_kernel<true, LST_F64, ALLM, SPLIT>), g, b, 0, s, a);
  else if (lst == LST_F32) hipLaunchKernelGGL((fo_sweep_queue_kernel<true, LST_F32, ALLM, SPLIT>), g, b, 0, s, a);
  // (round 6: the headline format has every instantiation the other list formats have -- horizon-split for small batches,
  // metric subsets -- instead of dropping to the generic kernel at the reference's own batch sizes, metric.py:125-147)
  else if (lst == LST_F32X) hipLaunchKernelGGL((fo_sweep_queue_kernel<true, LST_F32X, ALLM, SPLIT>), g, b, 0, s, a);
  else if (pair) hipLaunchKernelGGL((fo_sweep_queue_kernel<true, LST_NONE, ALLM, SPLIT>), g, b, 0, s, a);
  else hipLaunchKernelGGL((fo_sweep_queue_kernel<false, LST_NONE, ALLM, SPLIT>), g, b, 0, s, a);
}

// the list format of a run as the LST_* mode of a sweep instantiation
int lst_mode_of(const fo_ctx *ctx, const double *d_lists) {
  return !d_lists ? LST_NONE : ctx->list_format == FO_LISTS_F32 ? LST_F32 : ctx->list_format == FO_LISTS_F32_EXACT ? LST_F32X : LST_F64;
}
// the batch shape an entry of fo_sweep_autotune's table was measured on
bool tuned_for(const fo_ctx::Tuned &tu, int n_tiles, int A, int T, int lst, bool pair) {
  return tu.n_tiles == n_tiles && tu.A == A && tu.T == T && tu.lst == lst && tu.pair == pair;
}
// agents per wave fo_sweep_autotune measured for this shape on this context (the latest entry), 0 = none
int tuned_apw(const fo_ctx *ctx, int n_tiles, int A, int T, int lst, bool pair) {
  int apw = 0;
  for (int i = 0; i < ctx->n_tuned; ++i)
    if (tuned_for(ctx->tuned[i], n_tiles, A, T, lst, pair)) apw = ctx->tuned[i].apw;
  return apw;
}

// The agent table (+ AGENT_PAD_ROWS spare rows: the sweep reads row t + 1 of an agent without clamping, up to the trajectory
// horizon), the per-agent constants and integers for A agents x Ta samples.  A constants buffer that grew is cleared
// (generation-tagged slots, fo_agent_rows.hpp): on *stream, or with a blocking hipMemset where the caller has none (null).
int reserve_agents(fo_ctx *ctx, int A, int Ta, const hipStream_t *stream) {
  const size_t n = (size_t)(A > 0 ? A : 1);
  int rc;
  if ((rc = fo_reserve(ctx, &ctx->d_agent_tab, &ctx->cap_agent_tab, (n * Ta + AGENT_PAD_ROWS) * NAF))) return rc;
  const size_t cap0 = ctx->cap_agent_const;
  if ((rc = fo_reserve(ctx, &ctx->d_agent_const, &ctx->cap_agent_const, n * NAC))) return rc;
  if (ctx->cap_agent_const != cap0) {
    const size_t bytes = ctx->cap_agent_const * sizeof(double);
    FO_HIP_TRY(ctx, stream ? hipMemsetAsync(ctx->d_agent_const, 0, bytes, *stream) : hipMemset(ctx->d_agent_const, 0, bytes));
  }
  return fo_reserve(ctx, &ctx->d_agent_int, &ctx->cap_agent_int, n * 2);
}

}  // namespace

extern "C" {

// called from fo_create (fo_api.hip)
int fo_sweep_init_(fo_ctx *ctx) {
  FO_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_erf_tab, sizeof(double2) * ERF_N));
  hipLaunchKernelGGL(fo_erf_table_kernel, dim3((ERF_N + 255) / 256), dim3(256), 0, 0, (double2 *)ctx->d_erf_tab);
  FO_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_exp_tab, sizeof(double) * EXP_N));
  hipLaunchKernelGGL(fo_exp_table_kernel, dim3(1), dim3(EXP_N), 0, 0, (double *)ctx->d_exp_tab);
  FO_HIP_TRY(ctx, hipGetLastError());
  {  // Gauss-Legendre rules of the correlation integral: Newton on the Legendre recurrence; stored as
     // t = (x + 1)/2 and w/(4 pi)  (Int_0^asr f = asr/2 Sum w f(asr t), times the 1/(2 pi) of the formula)
    static double gl[2 * GL_TOTAL];
    double *o = gl;
    for (int r = 0; r < GL_NR; ++r) {
      const int n = gl_nodes(r);
      for (int i = 0; i < n; ++i) {
        double x = -cos(M_PI * (i + 0.75) / (n + 0.5)), dp = 1.0;
        for (int it = 0; it < 100; ++it) {
          double p0 = 1.0, p1 = x;
          for (int k = 2; k <= n; ++k) { const double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k; p0 = p1; p1 = p2; }
          dp = n * (x * p1 - p0) / (x * x - 1.0);
          const double dx = p1 / dp;
          x -= dx;
          if (fabs(dx) < 1e-16) break;
        }
        *o++ = 0.5 * (x + 1.0);
        *o++ = 2.0 / ((1.0 - x * x) * dp * dp) / (4.0 * M_PI);
      }
    }
    FO_HIP_TRY(ctx, hipMalloc((void **)&ctx->d_gl_tab, sizeof gl));
    FO_HIP_TRY(ctx, hipMemcpy(ctx->d_gl_tab, gl, sizeof gl, hipMemcpyHostToDevice));
  }
  FO_HIP_TRY(ctx, hipDeviceSynchronize());
  return FO_OK;
}

int fo_sweep_configure(fo_ctx *ctx, const fo_vehicle_t *veh, const fo_harm_coeff_t *hc, const fo_thresholds_t *thr,
                       uint32_t metric_mask, double dt) {
  if (!ctx || !veh || !hc || !thr) return fo_fail(ctx, FO_E_ARG, "fo_sweep_configure: null argument");
  if (!(veh->length > 0) || !(veh->width > 0) || !(dt > 0)) return fo_fail(ctx, FO_E_ARG, "fo_sweep_configure: bad vehicle/dt");
  ctx->veh = *veh; ctx->hc = *hc; ctx->thr = *thr; ctx->dt = dt;
  ctx->mask = required_metrics(metric_mask);
  ctx->configured = true;
  return FO_OK;
}

int fo_sweep_reserve(fo_ctx *ctx, int max_M, int max_T, int max_A, int max_Ta) {
  if (!ctx || max_M < 0 || max_T < 1 || max_A < 0 || max_Ta < 0) return fo_fail(ctx, FO_E_ARG, "fo_sweep_reserve: bad sizes");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int Mp = tiles_of(max_M) * TILE;
  int rc;
  if ((rc = fo_reserve(ctx, &ctx->d_traj_tab, &ctx->cap_traj_tab, (size_t)(max_T + 1) * NEF * Mp))) return rc;   // (+ a spare row, see sweep_run)
  // partial rows and chunk table: the planner's worst case for every batch within these sizes (fo_sweep_plan.hpp)
  if ((rc = fo_reserve(ctx, &ctx->d_partial, &ctx->cap_partial, max_chunk_cells(max_M, max_A) * NPS * TILE))) return rc;
  if ((rc = fo_reserve(ctx, &ctx->d_chunk_tab, &ctx->cap_chunk_tab, 2 * max_chunk_rows(max_A)))) return rc;
  if ((rc = reserve_agents(ctx, max_A, max_Ta > 0 ? max_Ta : 1, nullptr))) return rc;
  return FO_OK;
}

int fo_sweep_set_list_format(fo_ctx *ctx, int format) {
  if (!ctx) return FO_E_ARG;
  if (format != FO_LISTS_F64 && format != FO_LISTS_F32 && format != FO_LISTS_F32_EXACT)
    return fo_fail(ctx, FO_E_ARG, "fo_sweep_set_list_format: unknown format %d", format);
  ctx->list_format = format;
  return FO_OK;
}

// Book-keeping of a new agent set without the launch that fills it: buffers, sizes, generation tag.  `out` says where
// the rows go -- fo_sweep_set_agents launches fo_prep_agents_kernel on it, the fused planning step (fo_step_run) hands it to
// the phantom prediction kernel, which writes the rows of its own slots.
int fo_sweep_agents_begin_(fo_ctx *ctx, int A, int Ta, void *stream, fo_agent_table_t *out) {
  if (!ctx || !out) return FO_E_ARG;
  if (!ctx->configured) return fo_fail(ctx, FO_E_STATE, "fo_sweep_set_agents: call fo_sweep_configure first");
  if (A < 0 || (A > 0 && Ta < 1)) return fo_fail(ctx, FO_E_ARG, "fo_sweep_set_agents: bad arguments (A=%d Ta=%d)", A, Ta);
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = reserve_agents(ctx, A, Ta, &s))) return rc;
  ctx->A = A;
  ctx->Ta = Ta;
  if (ctx->status_gen >= (1 << 30)) {  // generations never run out in practice; start over cleanly if they do
    FO_HIP_TRY(ctx, hipMemsetAsync(ctx->d_status, 0, fo_ctx::kStatusWords * sizeof(int), s));
    FO_HIP_TRY(ctx, hipMemsetAsync(ctx->d_agent_const, 0, ctx->cap_agent_const * sizeof(double), s));   // (the tagged slots as well)
    ctx->status_gen = 0;
  }
  out->tab = ctx->d_agent_tab; out->cst = ctx->d_agent_const; out->aint = ctx->d_agent_int; out->status = ctx->d_status;
  out->gen = ++ctx->status_gen;
  out->ego_mass = ctx->veh.mass; out->hlA = 0.5 * ctx->veh.length; out->hwA = 0.5 * ctx->veh.width; out->hc = ctx->hc;
  return FO_OK;
}

int fo_sweep_set_agents(fo_ctx *ctx, int A, int Ta, const double *d_pos, const double *d_yaw, const double *d_v,
                        const double *d_cov, const double *d_shape, const double *d_raw_dims, const int32_t *d_type,
                        const int32_t *d_len, void *stream) {
  if (!ctx) return FO_E_ARG;
  if (!ctx->configured) return fo_fail(ctx, FO_E_STATE, "fo_sweep_set_agents: call fo_sweep_configure first");
  if (A < 0 || (A > 0 && (Ta < 1 || !d_pos || !d_yaw || !d_v || !d_cov || !d_shape || !d_raw_dims || !d_type || !d_len)))
    return fo_fail(ctx, FO_E_ARG, "fo_sweep_set_agents: bad arguments (A=%d Ta=%d)", A, Ta);
  fo_agent_table_t at;
  int rc;
  if ((rc = fo_sweep_agents_begin_(ctx, A, Ta, stream, &at))) return rc;
  if (A > 0) {
    const int n = A * Ta;
    hipLaunchKernelGGL(fo_prep_agents_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, Ta, d_pos, d_yaw, d_v, d_cov,
                       d_shape, d_raw_dims, d_type, d_len, at.ego_mass, at.hlA, at.hwA, at.hc, at.tab, at.cst, at.aint, at.status, at.gen);
    FO_HIP_TRY(ctx, hipGetLastError());
  }
  return FO_OK;
}

}  // extern "C"

namespace {

// The plan's knobs from the environment; `any` = fo_env_any("FO_SWEEP_"), so that production makes no getenv at all
// (FO_SWEEP_ABLATE and the trace paths are no plan inputs: sweep_run reads them where it uses them)
SweepKnobs read_knobs(bool any) {
  SweepKnobs k;
  if (!any) return k;
  if (const char *e = getenv("FO_SWEEP_GENERIC")) k.force_generic = e[0] == '1';   // debug / A-B aid
  if (const char *e = getenv("FO_SWEEP_APW")) k.apw = atoi(e);                      // tuning aid
  if (const char *e = getenv("FO_SWEEP_SPLIT")) k.split = e[0] == '1';              // tests, A/B runs
  if (const char *e = getenv("FO_SWEEP_SPLIT_APW")) k.split_apw = atoi(e);          // tests, A/B runs
  if (const char *e = getenv("FO_SWEEP_TAPER")) {                                   // tuning aid
    k.has_taper = true;
    sscanf(e, "%lf,%lf,%lf", &k.taper[0], &k.taper[1], &k.taper[2]);
  }
  return k;
}

// what fo_prep_traj_block needs to write the tile table and the chunk table of plan p
fo_prep_args_t prep_args_of(const fo_ctx *ctx, const SweepPlan &p, int M, int T, const double *d_x, const double *d_y,
                            const double *d_theta, const double *d_v) {
  const int tz = T > FO_PREP_TZ ? FO_PREP_TZ : T;   // horizon slice per block
  fo_prep_args_t pa;
  pa.on = 1; pa.M = M; pa.T = T; pa.tz = tz; pa.n_tiles = p.n_tiles; pa.nz = (T + tz - 1) / tz;
  pa.x = d_x; pa.y = d_y; pa.th = d_theta; pa.v = d_v; pa.tab = ctx->d_traj_tab; pa.chunk_tab = ctx->d_chunk_tab;
  pa.n_chunks = p.n_chunks; pa.wpb = p.wpb; pa.n0 = p.ph_n[0]; pa.n1 = p.ph_n[1]; pa.n2 = p.ph_n[2];
  pa.a0 = p.ph_a[0]; pa.a1 = p.ph_a[1]; pa.a2 = p.ph_a[2]; pa.a3 = p.ph_a[3];
  return pa;
}

// the sweep kernels' argument block (the trace buffer of the tuning build is the caller's)
SweepArgs sweep_args_of(const fo_ctx *ctx, const SweepPlan &p, int M, int T, double *d_pair_f, int32_t *d_pair_i,
                        double *d_lists, uint32_t ablate) {
  SweepArgs a{};
  a.M = M; a.Mp = p.Mp; a.T = T; a.A = ctx->A; a.Ta = ctx->Ta; a.n_tiles = p.n_tiles; a.nt8 = (p.n_tiles + 7) / 8; a.apw = p.apw;
  a.chunk_tab = ctx->d_chunk_tab;
  a.erf_tab = (const double2 *)ctx->d_erf_tab;
  a.exp_tab = (const double *)ctx->d_exp_tab;
  a.gl = (const double *)ctx->d_gl_tab;
  a.status = ctx->d_status;
  a.gen = ctx->status_gen;
  a.aint = ctx->d_agent_int;
  a.traj = ctx->d_traj_tab; a.atab = ctx->d_agent_tab; a.acst = ctx->d_agent_const; a.partial = ctx->d_partial;
  a.pair_f = d_pair_f; a.pair_i = d_pair_i; a.lists = d_lists;
  a.be_mask = (ctx->mask & FO_M_BE) ? ctx->d_be_mask : nullptr;
  a.hlA = 0.5 * ctx->veh.length; a.hwA = 0.5 * ctx->veh.width; a.wb = ctx->veh.wb_rear_axle;
  a.len3 = ctx->veh.length / 2.0 * (2.0 / 3.0);  // r_x * (2/3)  (collision_probability.py:160-161)
  a.off_x = ctx->veh.length / 6.0; a.off_y = ctx->veh.width / 2.0;
  a.hc = ctx->hc; a.dt = ctx->dt; a.thr_dce = ctx->thr.dce; a.mask = ctx->mask;
  a.ablate = ablate;
  return a;
}

// the sweep kernel of plan p: the instantiation for this output mode and metric set
void launch_sweep(const SweepPlan &p, int lst, bool pair, hipStream_t s, const SweepArgs &a) {
  const dim3 g(p.grid), b(p.block);
  if (p.use_queue) {
    const uint32_t all5 = FO_M_DCE | FO_M_CP | FO_M_TTC | FO_M_TTCE | FO_M_HR;
    const bool allm = (a.mask & all5) == all5 && a.ablate == 0;
    if (allm && p.split) launch_queue<true, true>(lst, pair, g, b, s, a);
    else if (p.split) launch_queue<false, true>(lst, pair, g, b, s, a);
    else if (allm) launch_queue<true, false>(lst, pair, g, b, s, a);
    else launch_queue<false, false>(lst, pair, g, b, s, a);
  } else {
    if (lst == LST_F64) hipLaunchKernelGGL((fo_sweep_generic_kernel<true, LST_F64>), g, b, 0, s, a);
    else if (lst_is32(lst)) hipLaunchKernelGGL((fo_sweep_generic_kernel<true, LST_F32>), g, b, 0, s, a);   // (converts at the store: exact)
    else if (pair) hipLaunchKernelGGL((fo_sweep_generic_kernel<true, LST_NONE>), g, b, 0, s, a);
    else hipLaunchKernelGGL((fo_sweep_generic_kernel<false, LST_NONE>), g, b, 0, s, a);
  }
}

// fo_sweep_run.  plan_only: everything up to the first launch -- argument checks, the grid plan, the work buffers -- and
// *plan_only = what the tile-table launch would have been given (fo_step_run hands it to the scene stage's ray kernel, whose
// extra workgroups write the table); prepped: that has happened on this stream, skip the launch.
int sweep_run(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, const double *d_theta,
              const double *d_v, const double *d_a, double *d_cost, uint8_t *d_safe, double *d_pair_f,
              int32_t *d_pair_i, double *d_lists, void *stream, fo_prep_args_t *plan_only, bool prepped) {
  if (plan_only) *plan_only = fo_prep_args_t();
  if (!ctx) return FO_E_ARG;
  if (!ctx->configured) return fo_fail(ctx, FO_E_STATE, "fo_sweep_run: call fo_sweep_configure first");
  if (M < 0 || T < 1 || (M > 0 && (!d_x || !d_y || !d_theta || !d_v || !d_cost || !d_safe)))
    return fo_fail(ctx, FO_E_ARG, "fo_sweep_run: bad arguments (M=%d T=%d)", M, T);
  if ((d_pair_f == nullptr) != (d_pair_i == nullptr)) return fo_fail(ctx, FO_E_ARG, "fo_sweep_run: pair_f and pair_i go together");
  if (d_lists && !d_pair_f) return fo_fail(ctx, FO_E_ARG, "fo_sweep_run: lists output requires the pair outputs");
  const bool do_be = (ctx->mask & FO_M_BE) != 0;
  if (do_be && M > 0 && !d_a) return fo_fail(ctx, FO_E_ARG, "fo_sweep_run: metric 'be' needs the acceleration profile d_a");
  if (M == 0) return FO_OK;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int A = ctx->A, Ta = ctx->Ta;
  if (!plan_only && d_lists && A > 0 && T > 1 && !(ctx->mask & (FO_M_CP | FO_M_HR)))  // nothing will write them: all-ones = NaN
    FO_HIP_TRY(ctx, hipMemsetAsync(d_lists, 0xFF, (ctx->list_format != FO_LISTS_F64 ? sizeof(float) : sizeof(double)) *
                                                     FO_NL * (size_t)A * (T - 1) * M, s));
  const bool knobs = fo_env_any("FO_SWEEP_");   // (any tuning / test knob of this family in the environment at all?)
  const int lst = lst_mode_of(ctx, d_lists);
  const bool pair = d_pair_f != nullptr;
  // a setting fo_sweep_autotune measured for this shape on this context wins over the static choice
  const SweepPlan p = plan_sweep(M, T, A, Ta, tuned_apw(ctx, tiles_of(M), A, T, lst, pair), ctx->force_apw, read_knobs(knobs));
  const int Mp = p.Mp;
  int rc;
  // (T + 1 rows per tile's worth: the sweep prefetches row t + 1 without clamping, the last tile's last prefetch lands in the spare)
  if ((rc = fo_reserve(ctx, &ctx->d_traj_tab, &ctx->cap_traj_tab, (size_t)(T + 1) * NEF * Mp))) return rc;
  if ((rc = fo_reserve(ctx, &ctx->d_partial, &ctx->cap_partial, (size_t)(p.n_chunks + 1) * NPS * Mp))) return rc;
  if ((rc = fo_reserve(ctx, &ctx->d_chunk_tab, &ctx->cap_chunk_tab, (size_t)2 * (p.n_chunks + 1)))) return rc;
  if (do_be && A > 0) {
    if ((rc = fo_reserve(ctx, &ctx->d_be_dist, &ctx->cap_be_dist, (size_t)(T + 1) * Mp))) return rc;  // [T][Mp] + min(a) [Mp]
    if ((rc = fo_reserve(ctx, &ctx->d_be_btn, &ctx->cap_be_btn, (size_t)A * Mp))) return rc;
    if ((rc = fo_reserve(ctx, &ctx->d_be_mask, &ctx->cap_be_mask, (size_t)A * Mp))) return rc;
  }

  if (A > 0) {
    const fo_prep_args_t pa = prep_args_of(ctx, p, M, T, d_x, d_y, d_theta, d_v);
    if (plan_only) { *plan_only = pa; return FO_OK; }
    if (!prepped) {
      hipLaunchKernelGGL(fo_prep_traj_kernel, dim3(p.n_tiles, 2, pa.nz), dim3(256), (size_t)2 * pa.tz * (TILE + 1) * sizeof(double), s, pa);
      FO_HIP_TRY(ctx, hipGetLastError());
    }
    const char *ab = fo_getenv(knobs, "FO_SWEEP_ABLATE");
    SweepArgs a = sweep_args_of(ctx, p, M, T, d_pair_f, d_pair_i, d_lists, ab ? (uint32_t)atoi(ab) : 0u);
    ctx->last_grid = p.grid; ctx->last_block = p.block; ctx->last_apw = p.apw;
    const bool timed = ctx->timing && ctx->n_timed < fo_ctx::kMaxTimed && (ctx->n_launch++ % ctx->timing_stride) == 0;
    if (timed) FO_HIP_TRY(ctx, hipEventRecord(ctx->ev_start[ctx->n_timed], s));
#if FO_TRACE
    static long long *d_trace = nullptr;
    const char *trace_path = fo_getenv(knobs, "FO_SWEEP_TRACE");
    if (trace_path && !d_trace) (void)hipMalloc((void **)&d_trace, sizeof(long long) * 4 * 65536);
    a.trace = trace_path ? d_trace : nullptr;
#endif
    launch_sweep(p, lst, pair, s, a);
    FO_HIP_TRY(ctx, hipGetLastError());
    if (timed) FO_HIP_TRY(ctx, hipEventRecord(ctx->ev_stop[ctx->n_timed++], s));
#if FO_TRACE
    if (a.trace && fo_getenv(knobs, "FO_SWEEP_TRACE_DUMP")) {   // (set for the one launch that is to be dumped)
      (void)hipStreamSynchronize(s);
      // (FO_SWEEP_TRACE_PHASES: the per-workgroup phase stamps as well, rows [32768, 32768 + grid) -- tools/split_trace.py)
      const size_t rows = fo_getenv(knobs, "FO_SWEEP_TRACE_PHASES") && p.grid <= 32768 ? (size_t)32768 + p.grid : (size_t)p.grid;
      long long *h = (long long *)malloc(sizeof(long long) * 4 * rows);
      (void)hipMemcpy(h, d_trace, sizeof(long long) * 4 * rows, hipMemcpyDeviceToHost);
      if (FILE *f = fopen(trace_path, "wb")) { fwrite(h, sizeof(long long), 4 * rows, f); fclose(f); }
      free(h);
    }
#endif
  }
  if (plan_only) return FO_OK;   // (no agents: nothing to prepare)
  const double *be_btn = nullptr;
  if (do_be && A > 0 && T >= 1) {
    double *dist = ctx->d_be_dist, *mina = ctx->d_be_dist + (size_t)T * Mp;
    hipLaunchKernelGGL(fo_be_prep_kernel, dim3((Mp + 255) / 256), dim3(256), 0, s, M, Mp, T, d_x, d_y, d_a, dist, mina);
    hipLaunchKernelGGL(fo_be_kernel, dim3(p.n_tiles, (A + 3) / 4), dim3(256), 0, s, M, Mp, T, A, Ta, ctx->d_traj_tab, dist,
                       mina, ctx->d_agent_tab, ctx->d_agent_const, ctx->d_agent_int, ctx->d_be_mask, 0.5 * ctx->veh.length,
                       0.5 * ctx->veh.width, ctx->veh.wb_rear_axle, ctx->veh.a_max, ctx->dt, ctx->d_be_btn, d_pair_f);
    FO_HIP_TRY(ctx, hipGetLastError());
    be_btn = ctx->d_be_btn;
  }
  hipLaunchKernelGGL(fo_reduce_kernel, dim3((M + 63) / 64), dim3(64 * RED_WAVES), 0, s, M, Mp, A, p.n_chunks, ctx->d_partial,
                     ctx->thr, ctx->mask, be_btn, d_cost, d_safe, ctx->d_status, ctx->status_gen);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

}  // namespace

extern "C" {

int fo_sweep_run(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, const double *d_theta,
                 const double *d_v, const double *d_a, double *d_cost, uint8_t *d_safe, double *d_pair_f,
                 int32_t *d_pair_i, double *d_lists, void *stream) {
  return sweep_run(ctx, M, T, d_x, d_y, d_theta, d_v, d_a, d_cost, d_safe, d_pair_f, d_pair_i, d_lists, stream, nullptr, false);
}

// the two halves of fo_sweep_run for the fused planning step (fo_step_run, fo_api.hip): plan -> *prep; [the scene stage writes
// the tile table] -> run without the table launch
int fo_sweep_plan_(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, const double *d_theta,
                   const double *d_v, const double *d_a, double *d_cost, uint8_t *d_safe, double *d_pair_f,
                   int32_t *d_pair_i, double *d_lists, void *stream, fo_prep_args_t *prep) {
  if (!prep) return FO_E_ARG;
  return sweep_run(ctx, M, T, d_x, d_y, d_theta, d_v, d_a, d_cost, d_safe, d_pair_f, d_pair_i, d_lists, stream, prep, false);
}
int fo_sweep_run_prepped_(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, const double *d_theta,
                          const double *d_v, const double *d_a, double *d_cost, uint8_t *d_safe, double *d_pair_f,
                          int32_t *d_pair_i, double *d_lists, void *stream) {
  return sweep_run(ctx, M, T, d_x, d_y, d_theta, d_v, d_a, d_cost, d_safe, d_pair_f, d_pair_i, d_lists, stream, nullptr, true);
}

// Per-shape choice of the sweep kernel's agents-per-wave, measured on the caller's own batch (include/fo_hip.h).
int fo_sweep_autotune(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, const double *d_theta, const double *d_v,
                      const double *d_a, double *d_cost, uint8_t *d_safe, double *d_pair_f, int32_t *d_pair_i, double *d_lists,
                      int reps, int *best_apw, double *ms4, void *stream) {
  if (!ctx) return FO_E_ARG;
  if (reps < 1) return fo_fail(ctx, FO_E_ARG, "fo_sweep_autotune: reps must be positive");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int A = ctx->A;
  const int n_tiles = tiles_of(M);   // the key of the tuned table, as sweep_run looks it up
  const int lst = lst_mode_of(ctx, d_lists);
  static const int cand[4] = {1, 2, 4, 8};
  hipEvent_t e0, e1;
  FO_HIP_TRY(ctx, hipEventCreate(&e0));
  FO_HIP_TRY(ctx, hipEventCreate(&e1));
  int rc = FO_OK, best = 0;
  double best_ms = INFINITY;
  const bool was_timing = ctx->timing;
  ctx->timing = false;
  for (int c = 0; c < 4 && rc == FO_OK; ++c) {
    ctx->force_apw = cand[c];
    for (int i = 0; i < (reps + 3) / 4 && rc == FO_OK; ++i)
      rc = fo_sweep_run(ctx, M, T, d_x, d_y, d_theta, d_v, d_a, d_cost, d_safe, d_pair_f, d_pair_i, d_lists, stream);
    if (rc == FO_OK && hipEventRecord(e0, s) != hipSuccess) rc = FO_E_HIP;
    for (int i = 0; i < reps && rc == FO_OK; ++i)
      rc = fo_sweep_run(ctx, M, T, d_x, d_y, d_theta, d_v, d_a, d_cost, d_safe, d_pair_f, d_pair_i, d_lists, stream);
    float ms = 0.f;
    if (rc == FO_OK && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                        hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) rc = FO_E_HIP;
    if (rc == FO_OK) {
      if (ms4) ms4[c] = (double)ms / reps;
      if ((double)ms / reps < best_ms) { best_ms = (double)ms / reps; best = cand[c]; }
    }
  }
  ctx->force_apw = 0;
  ctx->timing = was_timing;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != FO_OK) return rc == FO_E_HIP ? fo_fail(ctx, FO_E_HIP, "fo_sweep_autotune: HIP event failure") : rc;
  // remember (replace an entry of the same shape; the table is small and round-robin)
  int slot = -1;
  for (int i = 0; i < ctx->n_tuned; ++i)
    if (tuned_for(ctx->tuned[i], n_tiles, A, T, lst, d_pair_f != nullptr)) slot = i;
  if (slot < 0) {
    if (ctx->n_tuned < fo_ctx::kMaxTuned) slot = ctx->n_tuned++;
    else slot = ctx->next_tuned++ % fo_ctx::kMaxTuned;
  }
  ctx->tuned[slot] = fo_ctx::Tuned{n_tiles, A, T, lst, d_pair_f != nullptr, best};
  if (best_apw) *best_apw = best;
  // leave the outputs of a run with the chosen setting behind
  return fo_sweep_run(ctx, M, T, d_x, d_y, d_theta, d_v, d_a, d_cost, d_safe, d_pair_f, d_pair_i, d_lists, stream);
}

int fo_sweep_timing(fo_ctx *ctx, int enable) {
  if (!ctx) return FO_E_ARG;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (enable && !ctx->ev_start) {
    ctx->ev_start = new hipEvent_t[fo_ctx::kMaxTimed];
    ctx->ev_stop = new hipEvent_t[fo_ctx::kMaxTimed];
    for (int i = 0; i < fo_ctx::kMaxTimed; ++i) {
      FO_HIP_TRY(ctx, hipEventCreate(&ctx->ev_start[i]));
      FO_HIP_TRY(ctx, hipEventCreate(&ctx->ev_stop[i]));
    }
  }
  ctx->timing = enable != 0;
  ctx->timing_stride = enable > 1 ? enable : 1;  // enable = k > 1: every k-th launch carries the event pair
  ctx->n_launch = 0;
  ctx->n_timed = 0;
  return FO_OK;
}

int fo_sweep_timing_read(fo_ctx *ctx, double *total_ms, int *launches) {
  if (!ctx || !total_ms || !launches) return FO_E_ARG;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  double sum = 0.0;
  for (int i = 0; i < ctx->n_timed; ++i) {
    float ms = 0.f;
    FO_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop[i]));
    FO_HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start[i], ctx->ev_stop[i]));
    sum += ms;
  }
  *total_ms = sum;
  *launches = ctx->n_timed;
  ctx->n_timed = 0;
  return FO_OK;
}

int fo_sweep_timing_read_each(fo_ctx *ctx, double *each_ms, int cap, int *launches) {
  if (!ctx || !each_ms || !launches || cap < 0) return FO_E_ARG;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < ctx->n_timed && i < cap; ++i) {
    float ms = 0.f;
    FO_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop[i]));
    FO_HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start[i], ctx->ev_stop[i]));
    each_ms[i] = ms;
  }
  *launches = ctx->n_timed;
  ctx->n_timed = 0;
  return FO_OK;
}

int fo_sweep_last_launch(const fo_ctx *ctx, int *grid, int *block, int *agents_per_wave) {
  if (!ctx) return FO_E_ARG;
  if (grid) *grid = ctx->last_grid;
  if (block) *block = ctx->last_block;
  if (agents_per_wave) *agents_per_wave = ctx->last_apw;
  return FO_OK;
}

}  // extern "C"
