// fo_scene_hidden.hpp -- the host side of the hidden-traffic extensions: the fourteen fo_scene_hidden_* entry
// points, what they ask of their arguments and how they fill their kernels' arguments.  A part of fo_scene.hip's translation unit,
// included behind the kernel parts (fo_hidden_*.hpp), whose argument structures and launch helpers it uses; it holds no device code.
//
// Every question stands once: hr_check_* is what the forecast and the clearance ask, hb_check_* what the brake entries ask on top,
// hbu_* what the four entries of the users family (brake_users, ladder_users, verdict, ladder_verdict) share -- their parameter
// structures carry the same member names up to d_arc, so these are templates over the structure.  All of them take (ctx, ..., fn),
// fn the entry's name as the refusal spells it, and return FO_OK or the refusal's code.  An entry is the list of its questions in
// the order its comment in fo_hip.h gives; every refusal precedes the first device call.
#pragma once

// ---- what the reach forecast and the clearance ask alike
static int hr_check_scene(fo_ctx *ctx, const void *p, const char *fn) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "%s: call fo_scene_set_map first", fn);
  if (!p) return fo_fail(ctx, FO_E_ARG, "%s: no parameters", fn);
  const StaticMap *m = ((Scene *)ctx->scene)->map;
  if (m->P < 1 || !m->d_raster) return fo_fail(ctx, FO_E_STATE, "%s: call fo_scene_set_map first", fn);
  return FO_OK;
}

static int hr_check_extent(fo_ctx *ctx, int nx, int ny, const char *fn) {
  if (nx < 1 || ny < 1 || nx > 32768 || ny > 32768) return fo_fail(ctx, FO_E_ARG, "%s: window %d x %d outside [1, 32768]^2", fn, nx, ny);
  return FO_OK;
}

static int hr_check_window(fo_ctx *ctx, const uint8_t *d_cls, int nx, int ny, const char *fn) {
  if (!d_cls) return fo_fail(ctx, FO_E_ARG, "%s: no cell classes (d_cls of the visibility stage)", fn);
  return hr_check_extent(ctx, nx, ny, fn);
}

// the reach table of a forecast: there at all, then (after the checks a caller puts between) its values
static int hr_check_table(fo_ctx *ctx, int J, const int32_t *h_r2, const char *fn) {
  if (J < 1 || J > HR_MAX_J)
    return fo_fail(ctx, FO_E_ARG, "%s: J = %d outside [1, %d] (arrival steps are bytes, 255 = never)", fn, J, HR_MAX_J);
  if (!h_r2) return fo_fail(ctx, FO_E_ARG, "%s: no reach table h_r2 [J]", fn);
  return FO_OK;
}

// r2: the largest squared reach of the call, `what` its name and `speed` the speed that sets it, as the refusal names them
static int hr_check_halo(fo_ctx *ctx, int r2, const char *what, const char *speed, const char *fn) {
  constexpr int cap = FO_HIDDEN_REACH_MAX_HALO;
  if (r2 >= (cap + 1) * (cap + 1))
    return fo_fail(ctx, FO_E_ARG, "%s: %s = %d is a reach of more than FO_HIDDEN_REACH_MAX_HALO = %d cells "
                   "(shorten the horizon or lower %s; the reach is never cut short)", fn, what, r2, cap, speed);
  return FO_OK;
}

static int hr_check_table_values(fo_ctx *ctx, int J, const int32_t *h_r2, const char *fn) {
  if (h_r2[0] < 0) return fo_fail(ctx, FO_E_ARG, "%s: h_r2[0] = %d is negative", fn, h_r2[0]);
  for (int j = 1; j < J; ++j)
    if (h_r2[j] < h_r2[j - 1])
      return fo_fail(ctx, FO_E_ARG, "%s: h_r2 decreases at entry %d (%d after %d)", fn, j, h_r2[j], h_r2[j - 1]);
  return hr_check_halo(ctx, h_r2[J - 1], "h_r2[J-1]", "v_max", fn);
}

static int hr_check_poses(fo_ctx *ctx, const double *d_x, const double *d_y, const double *d_heading, const char *fn) {
  if (!d_x || !d_y || !d_heading)
    return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
  return FO_OK;
}

static int hr_check_footprint(fo_ctx *ctx, double hl, double hw, double wb, const char *fn) {
  const double ext = HR_MAX_EXTENT * ((Scene *)ctx->scene)->map->cs;   // (NaN fails every comparison)
  if (!(hl >= 0.0 && hl <= ext) || !(hw >= 0.0 && hw <= ext) || !(fabs(wb) <= ext))
    return fo_fail(ctx, FO_E_ARG, "%s: half extents outside [0, %g m] or |wb| above it (hl = %g, hw = %g, wb = %g; "
                   "FO_HIDDEN_REACH_MAX_HALF_EXTENT = %d cells)", fn, ext, hl, hw, wb, HR_MAX_EXTENT);
  return FO_OK;
}

// the lane flow reads the map's move table
static int hr_check_moves(fo_ctx *ctx, const char *fn) {
  if (!((Scene *)ctx->scene)->map->d_lane_moves)
    return fo_fail(ctx, FO_E_STATE, "%s: the map has no move table (call fo_scene_set_lane_moves first)", fn);
  return FO_OK;
}

// ---- what the entries over a forecast's arrival map ask of it (the forecast itself, witness, brake, brake_ladder): the table, the
// maps -- `maps`: they are there, `no_maps`: the entry's own words where they are not --, the window (`cls`: with the cell classes),
// the table's values, M; then, with M > 0 and around what an entry asks between, the samples and the forecast's own buffers
static int hr_check_forecast(fo_ctx *ctx, const fo_hidden_reach_t &b, bool maps, const char *no_maps, bool cls, const char *fn) {
  int rc;
  if ((rc = hr_check_table(ctx, b.J, b.h_r2, fn))) return rc;
  if (!maps) return fo_fail(ctx, FO_E_ARG, no_maps, fn);
  if ((rc = cls ? hr_check_window(ctx, b.d_cls, b.win_nx, b.win_ny, fn) : hr_check_extent(ctx, b.win_nx, b.win_ny, fn))) return rc;
  if ((rc = hr_check_table_values(ctx, b.J, b.h_r2, fn))) return rc;
  if (b.M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, b.M);
  return FO_OK;
}

static int hr_check_forecast_samples(fo_ctx *ctx, const fo_hidden_reach_t &b, const char *fn) {
  if (b.T < 1 || b.T > b.J)
    return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, J = %d] (every sample needs its reach)", fn, b.T, b.J);
  return FO_OK;
}

static int hr_check_forecast_poses(fo_ctx *ctx, const fo_hidden_reach_t &b, const char *fn) {
  if (!b.d_x || !b.d_y || !b.d_heading || !b.d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T], d_heading [M][T][2] and d_first [M] of the forecast are required with M > 0", fn);
  return FO_OK;
}

// ---- what the brake entries ask on top
static int hb_check_dt(fo_ctx *ctx, double dt, const char *fn) {
  if (!(dt > 0.0) || !std::isfinite(dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, dt);
  return FO_OK;
}

static int hb_check_brake(fo_ctx *ctx, double a_brake, double dt, const char *fn) {
  if (!(a_brake >= 0.0) || !std::isfinite(a_brake))      // (NaN fails every comparison)
    return fo_fail(ctx, FO_E_ARG, "%s: a_brake = %g, a finite deceleration >= 0 is needed", fn, a_brake);
  return hb_check_dt(ctx, dt, fn);
}

static int hb_check_level_values(fo_ctx *ctx, int n, const double *h_levels, const char *fn) {
  for (int l = 0; l < n; ++l)
    if (!(h_levels[l] >= 0.0) || !std::isfinite(h_levels[l]))      // (NaN fails every comparison)
      return fo_fail(ctx, FO_E_ARG, "%s: h_levels[%d] = %g, a finite deceleration >= 0 is needed", fn, l, h_levels[l]);
  return FO_OK;
}

// the ladder of the users family, L levels; ascending: the verdict's answer is a maximum over brake starts
static int hb_check_levels(fo_ctx *ctx, int L, const double *h_levels, bool ascending, const char *fn) {
  if (L < 1 || L > FO_HIDDEN_BRAKE_MAX_LEVELS)
    return fo_fail(ctx, FO_E_ARG, "%s: L = %d outside [1, FO_HIDDEN_BRAKE_MAX_LEVELS = %d]", fn, L, FO_HIDDEN_BRAKE_MAX_LEVELS);
  if (!h_levels) return fo_fail(ctx, FO_E_ARG, "%s: no decelerations h_levels [L]", fn);
  if (int rc = hb_check_level_values(ctx, L, h_levels, fn)) return rc;
  for (int l = 1; ascending && l < L; ++l)
    if (!(h_levels[l] > h_levels[l - 1]))
      return fo_fail(ctx, FO_E_ARG, "%s: h_levels[%d] = %g after %g: the levels must be strictly ascending (the answer is the gentlest "
                     "sufficient one)", fn, l, h_levels[l], h_levels[l - 1]);
  return FO_OK;
}

static int hb_check_samples(fo_ctx *ctx, int T, const char *fn) {
  if (T < 1 || T > HR_MAX_J) return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, %d]", fn, T, HR_MAX_J);
  return FO_OK;
}

static int hb_check_starts(fo_ctx *ctx, int B, int T, const char *fn) {
  if (B < 1 || B > T) return fo_fail(ctx, FO_E_ARG, "%s: B = %d outside [1, T = %d]", fn, B, T);
  return FO_OK;
}

static int hb_check_speeds(fo_ctx *ctx, const double *d_v, const double *d_arc, const char *fn) {
  if (!d_v || !d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
  return FO_OK;
}

// the classes and their threshold table, which travels as a kernel argument: there at all (before M is looked at) ...
static int hb_check_classes(fo_ctx *ctx, int C, const int32_t *h_thr, int nx, int ny, const char *fn) {
  if (C < 1 || C > FO_HIDDEN_BRAKE_MAX_CLASSES)
    return fo_fail(ctx, FO_E_ARG, "%s: C = %d outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = %d]", fn, C, FO_HIDDEN_BRAKE_MAX_CLASSES);
  if (!h_thr) return fo_fail(ctx, FO_E_ARG, "%s: no threshold table h_thr [C][T]", fn);
  return hr_check_extent(ctx, nx, ny, fn);
}

// ... its size, with M > 0 ...
static int hb_check_table_size(fo_ctx *ctx, int C, int T, const char *fn) {
  if (C * T > FO_HIDDEN_BRAKE_MAX_TABLE)
    return fo_fail(ctx, FO_E_ARG, "%s: C * T = %d * %d = %d entries, the table is a kernel argument of at most "
                   "FO_HIDDEN_BRAKE_MAX_TABLE = %d", fn, C, T, C * T, FO_HIDDEN_BRAKE_MAX_TABLE);
  return FO_OK;
}

// ... together with a ladder's levels ...
static int hb_check_arg_bytes(fo_ctx *ctx, int C, int T, int L, const char *fn) {
  if (4 * C * T + 8 * L > FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES)
    return fo_fail(ctx, FO_E_ARG, "%s: %d thresholds (C * T = %d * %d) and %d levels take 4 * %d + 8 * %d = %d bytes, they travel as a "
                   "kernel argument of at most FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES = %d", fn, C * T, C, T, L, C * T, L,
                   4 * C * T + 8 * L, FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES);
  return FO_OK;
}

// ... and its rows: row c against the cap of the map it names, r2_cap[map_of[c]] -- or, map_of null, every row against the one cap
static int hb_check_rows(fo_ctx *ctx, int C, int T, const int32_t *h_thr, const int32_t *r2_cap, const int32_t *map_of, const char *fn) {
  for (int c = 0; c < C; ++c) {
    const int32_t *row = h_thr + (size_t)c * T;
    const int k = map_of ? map_of[c] : 0;
    const int64_t cap = (int64_t)169 * r2_cap[k];
    if (row[0] < 0) return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][0] = %d is negative", fn, c, row[0]);
    for (int j = 1; j < T; ++j)
      if (row[j] < row[j - 1])
        return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d] decreases at entry %d (%d after %d)", fn, c, j, row[j], row[j - 1]);
    if (row[T - 1] > cap && !map_of)
      return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][T-1] = %d lies beyond 169 r2_cap = %lld (the key map ends at the cap)", fn, c,
                     row[T - 1], (long long)cap);
    if (row[T - 1] > cap)
      return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][T-1] = %d lies beyond 169 r2_cap[%d] = %lld (the key map of class %d ends at its cap)",
                     fn, c, row[T - 1], k, (long long)cap, c);
  }
  return FO_OK;
}

// d_cost_or_null and d_safe_or_null of a verdict
static int hb_check_cost_pair(fo_ctx *ctx, const double *d_cost, const uint8_t *d_safe, const char *fn) {
  if (!d_cost != !d_safe)
    return fo_fail(ctx, FO_E_ARG, "%s: d_cost_or_null [M][FO_NC] and d_safe_or_null [M] go together (%s is missing)", fn,
                   d_safe ? "d_cost_or_null" : "d_safe_or_null");
  return FO_OK;
}

// ---- the users family; P: its parameter structure.  Before M is looked at: the maps, the classes, the window, every map's cap,
// every class's map, M (entries of r2_cap beyond K and of map_of beyond C are not looked at)
template <class P>
static int hbu_check_head(fo_ctx *ctx, const P &p, const char *fn) {
  int rc;
  if (p.K < 1 || p.K > FO_HIDDEN_BRAKE_MAX_MAPS)
    return fo_fail(ctx, FO_E_ARG, "%s: K = %d outside [1, FO_HIDDEN_BRAKE_MAX_MAPS = %d]", fn, p.K, FO_HIDDEN_BRAKE_MAX_MAPS);
  if ((rc = hb_check_classes(ctx, p.C, p.h_thr, p.win_nx, p.win_ny, fn))) return rc;
  for (int k = 0; k < p.K; ++k) {
    if (p.r2_cap[k] < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap[%d] = %d is negative", fn, k, p.r2_cap[k]);
    static const char *const names[FO_HIDDEN_BRAKE_MAX_MAPS] = {"r2_cap[0]", "r2_cap[1]", "r2_cap[2]"};
    if ((rc = hr_check_halo(ctx, p.r2_cap[k], names[k], "v_cap", fn))) return rc;
  }
  for (int c = 0; c < p.C; ++c)
    if (p.map_of[c] < 0 || p.map_of[c] >= p.K)
      return fo_fail(ctx, FO_E_ARG, "%s: map_of[%d] = %d outside [0, K = %d)", fn, c, p.map_of[c], p.K);
  if (p.M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p.M);
  return FO_OK;
}

// with M > 0, behind the sizes: the table's rows, the poses, the K clearances' maps, the speeds
template <class P>
static int hbu_check_inputs(fo_ctx *ctx, const P &p, const char *fn) {
  int rc;
  if ((rc = hb_check_rows(ctx, p.C, p.T, p.h_thr, p.r2_cap, p.map_of, fn))) return rc;
  if ((rc = hr_check_poses(ctx, p.d_x, p.d_y, p.d_heading, fn))) return rc;
  for (int k = 0; k < p.K; ++k)
    if (!p.d_key[k] || !p.d_qmin[k])
      return fo_fail(ctx, FO_E_ARG, "%s: d_key[%d] [win_ny][win_nx] and d_qmin[%d] [M][T] of clearance %d are required with M > 0", fn,
                     k, k, k);
  return hb_check_speeds(ctx, p.d_v, p.d_arc, fn);
}

// what its kernels take of the maps: named members (see HrBrakeUsersArgs), those beyond K null; map_of two bits a class (hbu_map_of)
struct HbuMaps {
  const int32_t *key[FO_HIDDEN_BRAKE_MAX_MAPS], *qmin[FO_HIDDEN_BRAKE_MAX_MAPS];
  uint32_t map_of;
};

template <class P>
static HbuMaps hbu_maps(const P &p) {
  HbuMaps m{};
  for (int k = 0; k < p.K; ++k) { m.key[k] = p.d_key[k]; m.qmin[k] = p.d_qmin[k]; }
  for (int c = 0; c < p.C; ++c) m.map_of |= (uint32_t)p.map_of[c] << (2 * c);
  return m;
}

// ---- the tables that travel as kernel arguments: n = C * T thresholds, and a ladder's L levels in front of them
static HbThr hb_thr(const int32_t *h_thr, int n) {
  HbThr thr;
  for (int t = 0; t < FO_HIDDEN_BRAKE_MAX_TABLE; ++t) thr.v[t] = t < n ? h_thr[t] : 0;
  return thr;
}

static HbluPack hblu_pack(const double *h_levels, int L, const int32_t *h_thr, int n) {
  HbluPack pk;
  memset(pk.w, 0, sizeof pk.w);
  memcpy(pk.w, h_levels, (size_t)L * sizeof(double));        // (little endian: low word first)
  memcpy(pk.w + 2 * L, h_thr, (size_t)n * sizeof(int32_t));
  return pk;
}

// the road metric's distance map: the caller's buffer, or -- the caller does not want the distances -- a workspace of the context
static int hr_dist_buffer(fo_ctx *ctx, Scene *sc, bool road, size_t cells, uint16_t **d_dist) {
  if (!road || *d_dist) return FO_OK;
  if (int rc = fo_reserve(ctx, &sc->d_hr_dist, &sc->cap_hr_dist, cells)) return rc;
  *d_dist = sc->d_hr_dist;
  return FO_OK;
}

// the metrics of the forecast: `road` adds the distance bands and the arrival merge between the map and the trajectories, `flow`
// (with road) takes the bands over the map's move table in place of the undirected ones
static int hidden_reach_call(fo_ctx *ctx, const fo_hidden_reach_t *p, bool road, bool flow, uint16_t *d_dist, const char *fn, void *stream) {
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if ((rc = hr_check_forecast(ctx, *p, p->d_arrival, "%s: no buffer for the arrival map (d_arrival is required)", true, fn))) return rc;
  const int h = reach_cells(p->h_r2[p->J - 1]);
  if (p->M > 0) {
    if ((rc = hr_check_forecast_samples(ctx, *p, fn))) return rc;
    if ((rc = hr_check_poses(ctx, p->d_x, p->d_y, p->d_heading, fn))) return rc;
    if (!p->d_cells || !p->d_first || !p->d_slack)
      return fo_fail(ctx, FO_E_ARG, "%s: d_cells [M][T], d_first [M] and d_slack [M] are required with M > 0", fn);
    if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  }
  if (flow && (rc = hr_check_moves(ctx, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int nx = p->win_nx, ny = p->win_ny;
  if ((rc = hr_dist_buffer(ctx, sc, road, (size_t)ny * nx, &d_dist))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HrMapArgs a{sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, nx, ny, p->d_cls, p->d_hidden_or_null,
              h, p->J, nullptr, p->d_arrival};
  if ((rc = hr_launch_rows(ctx, sc, a, s))) return rc;
  a.g = sc->d_hr_g;
  HrR2 r2;
  for (int j = 0; j < HR_MAX_J; ++j) r2.v[j] = p->h_r2[j < p->J ? j : p->J - 1];
  hipLaunchKernelGGL(fo_hr_cols_kernel<HrR2>, dim3((nx + HR_TX - 1) / HR_TX, (ny + HR_TY - 1) / HR_TY), dim3(HR_THREADS),
                     (size_t)(HR_TY + 2 * h) * HR_TX, s, a, r2);
  if (road) {
    HrR2 reach;                         // L[j] = isqrt(169 R2[j]): the reach in distance units (12 / 17 per step, 13 per cell)
    for (int j = 0; j < HR_MAX_J; ++j) reach.v[j] = road_reach(r2.v[j]);
    if (flow) hr_launch_flow_bands(a, sc->map->d_lane_moves, d_dist, reach.v[p->J - 1], s);
    else hr_launch_bands(a, d_dist, reach.v[p->J - 1], s);
    const HrRoadArrivalArgs aa{p->d_cls, d_dist, p->d_arrival, nx * ny, p->J};
    hipLaunchKernelGGL(fo_hr_road_arrival_kernel, dim3((nx * ny + HR_THREADS - 1) / HR_THREADS), dim3(HR_THREADS), 0, s, aa, reach);
  }
  if (p->M > 0) {
    int G = 1;
    while (G < p->T && G < 64) G <<= 1;
    HrTrajArgs t{p->M, p->T, G, p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0,
                 sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, nx, ny, p->d_arrival,
                 p->d_cells, p->d_first, p->d_slack};
    const int per_block = HR_THREADS / G;
    const dim3 grid((unsigned)(((size_t)p->M + per_block - 1) / per_block));
    hipLaunchKernelGGL(fo_hr_traj_kernel, grid, dim3(HR_THREADS), 0, s, t);
  }
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the clearance: the distance transform and the distance bands of the reach, run to a cap in place of a table's end; `flow`: the
// road metric alone, its bands over the map's move table
static int hidden_clearance_call(fo_ctx *ctx, const fo_hidden_clearance_t *p, bool flow, const char *fn, void *stream) {
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if (flow && p->metric != FO_HIDDEN_CLEARANCE_ROAD)
    return fo_fail(ctx, FO_E_ARG, "%s: metric = %d (the lane flow is a road metric: 1 road)", fn, p->metric);
  if (p->metric != FO_HIDDEN_CLEARANCE_EUCLID && p->metric != FO_HIDDEN_CLEARANCE_ROAD)
    return fo_fail(ctx, FO_E_ARG, "%s: metric = %d (0 euclid, 1 road)", fn, p->metric);
  if (!p->d_key) return fo_fail(ctx, FO_E_ARG, "%s: no buffer for the key map (d_key is required)", fn);
  if ((rc = hr_check_window(ctx, p->d_cls, p->win_nx, p->win_ny, fn))) return rc;
  if (p->r2_cap < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap = %d is negative", fn, p->r2_cap);
  if ((rc = hr_check_halo(ctx, p->r2_cap, "r2_cap", "v_cap", fn))) return rc;
  const int h = reach_cells(p->r2_cap);
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (p->M > 0) {
    if (p->T < 1) return fo_fail(ctx, FO_E_ARG, "%s: T = %d (at least one sample with M > 0)", fn, p->T);
    if ((rc = hr_check_poses(ctx, p->d_x, p->d_y, p->d_heading, fn))) return rc;
    if (!p->d_qmin) return fo_fail(ctx, FO_E_ARG, "%s: d_qmin [M][T] is required with M > 0", fn);
    if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  }
  if (flow && (rc = hr_check_moves(ctx, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int nx = p->win_nx, ny = p->win_ny;
  const bool road = p->metric == FO_HIDDEN_CLEARANCE_ROAD;
  uint16_t *d_dist = p->d_dist_or_null;
  if ((rc = hr_dist_buffer(ctx, sc, road, (size_t)ny * nx, &d_dist))) return rc;
  hipStream_t s = (hipStream_t)stream;
  HrMapArgs a{sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, nx, ny, p->d_cls, p->d_hidden_or_null,
              h, 0, nullptr, nullptr};
  if ((rc = hr_launch_rows(ctx, sc, a, s))) return rc;
  a.g = sc->d_hr_g;
  hipLaunchKernelGGL(fo_hr_cols_kernel<HrKeyOut>, dim3((nx + HR_TX - 1) / HR_TX, (ny + HR_TY - 1) / HR_TY), dim3(HR_THREADS),
                     (size_t)(HR_TY + 2 * h) * HR_TX, s, a, HrKeyOut{p->r2_cap, p->d_key});
  if (road) {
    if (flow) hr_launch_flow_bands(a, sc->map->d_lane_moves, d_dist, road_reach(p->r2_cap), s);
    else hr_launch_bands(a, d_dist, road_reach(p->r2_cap), s);  // to Lcap = isqrt(169 r2_cap)
    const HcMergeArgs ma{d_dist, p->d_key, nx * ny};
    hipLaunchKernelGGL(fo_hc_road_merge_kernel, dim3((nx * ny + HR_THREADS - 1) / HR_THREADS), dim3(HR_THREADS), 0, s, ma);
  }
  if (p->M > 0) {
    HcTrajArgs t{p->M, p->T, p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0,
                 sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, nx, ny, p->d_key, p->d_qmin};
    const size_t poses = (size_t)p->M * p->T;
    hipLaunchKernelGGL(fo_hc_traj_kernel, dim3((unsigned)((poses + HR_THREADS - 1) / HR_THREADS)), dim3(HR_THREADS), 0, s, t);
  }
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the impact verdict of every trajectory over its first B brake starts against every class of road user on the key map it names --
// the worst harm that remains after braking, folded into the reserved cost columns and the safety flag: one launch; map_of and the
// table travel as kernel arguments, the harm rows and speeds in the caller's device buffer.  The ONE host part of both entries:
// head-on (fo_hidden_brake_impact.hpp) and, LANES, by approach angle (fo_hidden_brake_impact_lanes.hpp), which asks for its mask,
// its two numbers, its two outputs and the map's move table on top
template <bool LANES, class P>
static int hidden_brake_impact_call(fo_ctx *ctx, const P *p, const char *fn, void *stream) {
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if ((rc = hbu_check_head(ctx, *p, fn))) return rc;
  if ((rc = hb_check_brake(ctx, p->a_brake, p->dt, fn))) return rc;
  if (!(p->harm_limit >= 0.0))                                   // (NaN fails the comparison; +inf passes)
    return fo_fail(ctx, FO_E_ARG, "%s: harm_limit = %g, a harm >= 0 (or +inf) is needed", fn, p->harm_limit);
  if constexpr (LANES) {
    if (p->dir_mask >> p->C != 0u)
      return fo_fail(ctx, FO_E_ARG, "%s: dir_mask = 0x%x has bits at or above C = %d", fn, p->dir_mask, p->C);
    if (!(fabs(p->cos_h) <= 1.0) || !(fabs(p->sin_h) <= 1.0))    // (NaN fails the comparison)
      return fo_fail(ctx, FO_E_ARG, "%s: cos_h = %g, sin_h = %g, the cosine and sine of 22.5 deg + heading_slack in [-1, 1] are needed",
                     fn, p->cos_h, p->sin_h);
    if (p->dir_mask != 0u && (rc = hr_check_moves(ctx, fn))) return rc;
  }
  if (p->M == 0) return FO_OK;
  const int T = p->T, B = p->B, K = p->K, C = p->C;
  if ((rc = hb_check_samples(ctx, T, fn))) return rc;
  if ((rc = hb_check_starts(ctx, B, T, fn))) return rc;
  if ((rc = hb_check_table_size(ctx, C, T, fn))) return rc;
  if ((rc = hbu_check_inputs(ctx, *p, fn))) return rc;
  if (!p->d_speed_of || !p->d_harm_rows)
    return fo_fail(ctx, FO_E_ARG, "%s: d_speed_of [C] and d_harm_rows [C][4] are required with M > 0", fn);
  if constexpr (LANES) {
    if (!p->d_harm || !p->d_user || !p->d_closing || !p->d_cosine || !p->d_at || !p->d_commit || !p->d_first)
      return fo_fail(ctx, FO_E_ARG, "%s: d_harm [M][2], d_user [M], d_closing, d_cosine, d_at, d_commit and d_first [C][M] are required with M > 0", fn);
  } else {
    if (!p->d_harm || !p->d_user || !p->d_speed || !p->d_at || !p->d_commit || !p->d_first)
      return fo_fail(ctx, FO_E_ARG, "%s: d_harm [M][2], d_user [M], d_speed, d_at, d_commit and d_first [C][M] are required with M > 0", fn);
  }
  if ((rc = hb_check_cost_pair(ctx, p->d_cost_or_null, p->d_safe_or_null, fn))) return rc;
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HbuMaps mp = hbu_maps(*p);
  const HbThr thr = hb_thr(p->h_thr, C * T);
  const dim3 grid((unsigned)brake_verdict_blocks(p->M, T, K, B)), block(HB_THREADS);
  const size_t lds = brake_verdict_lds_bytes(T, K, C, B);
  hipStream_t s = (hipStream_t)stream;
  if constexpr (LANES) {
    const uint32_t dir = p->cos_h > -1.0 ? p->dir_mask : 0u;     // h >= pi: every class is head-on, the table is not read
    const HrBrakeImpactLanesArgs a{p->M, T, brake_verdict_group(B), brake_verdict_per_block(T, K, B), C, B, p->d_x, p->d_y, p->d_heading,
                                   p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster,
                                   sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, mp.key[0], mp.key[1],
                                   mp.key[2], mp.qmin[0], mp.qmin[1], mp.qmin[2], mp.map_of, p->d_v, p->d_arc, p->a_brake, p->dt,
                                   p->d_speed_of, p->d_harm_rows, p->harm_limit, sc->map->d_lane_moves, dir, p->cos_h, p->sin_h,
                                   p->d_finite_or_null, p->d_cost_or_null, p->d_safe_or_null, p->d_harm, p->d_user, p->d_closing,
                                   p->d_cosine, p->d_at, p->d_commit, p->d_first};
    if (brake_users_width(C) == 4) hbil_launch<4>(K, grid, block, lds, s, a, thr);
    else hbil_launch<8>(K, grid, block, lds, s, a, thr);
  } else {
    const HrBrakeImpactArgs a{p->M, T, brake_verdict_group(B), brake_verdict_per_block(T, K, B), C, B, p->d_x, p->d_y, p->d_heading,
                              p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster,
                              sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, mp.key[0], mp.key[1], mp.key[2],
                              mp.qmin[0], mp.qmin[1], mp.qmin[2], mp.map_of, p->d_v, p->d_arc, p->a_brake, p->dt, p->d_speed_of,
                              p->d_harm_rows, p->harm_limit, p->d_finite_or_null, p->d_cost_or_null, p->d_safe_or_null, p->d_harm,
                              p->d_user, p->d_speed, p->d_at, p->d_commit, p->d_first};
    if (brake_users_width(C) == 4) hbi_launch<4>(K, grid, block, lds, s, a, thr);
    else hbi_launch<8>(K, grid, block, lds, s, a, thr);
  }
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// The host part of the ladder verdict (fo_hidden_brake_ladder_verdict.hpp) and, HARM, of the harm ladder
// (fo_hidden_brake_harm_ladder.hpp), which asks for the impact entry's speeds, rows and limit behind the ladder verdict's list and for
// the curve's two outputs where that entry asks for its own: one launch; the levels, map_of and the table travel as kernel arguments.
// Both structures name their shared members alike.  HARM_LANES: the harm ladder by approach angle
// (fo_hidden_brake_harm_ladder_lanes.hpp), which asks for everything HARM asks for and, behind harm_limit, for the impact-lanes
// entry's mask, its two numbers and the map's move table
enum { HBLV_VERDICT = 0, HBLV_HARM = 1, HBLV_HARM_LANES = 2 };
template <int FORM, class P>
static int hidden_brake_ladder_verdict_call(fo_ctx *ctx, const P *p, const char *fn, void *stream) {
  constexpr bool HARM = FORM != HBLV_VERDICT, LANES = FORM == HBLV_HARM_LANES;
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if ((rc = hbu_check_head(ctx, *p, fn))) return rc;
  if ((rc = hb_check_levels(ctx, p->L, p->h_levels, true, fn))) return rc;
  if ((rc = hb_check_dt(ctx, p->dt, fn))) return rc;
  if (!(p->a_limit >= 0.0))                                      // (NaN fails the comparison; +inf passes)
    return fo_fail(ctx, FO_E_ARG, "%s: a_limit = %g, a deceleration >= 0 (or +inf) is needed", fn, p->a_limit);
  if (p->M == 0) return FO_OK;
  const int T = p->T, B = p->B, K = p->K, C = p->C, L = p->L;
  if ((rc = hb_check_samples(ctx, T, fn))) return rc;
  if ((rc = hb_check_starts(ctx, B, T, fn))) return rc;
  if ((rc = hb_check_table_size(ctx, C, T, fn))) return rc;
  if ((rc = hb_check_arg_bytes(ctx, C, T, L, fn))) return rc;
  if ((rc = hbu_check_inputs(ctx, *p, fn))) return rc;
  if constexpr (HARM) {
    if (!p->d_need || !p->d_at || !p->d_blocking || !p->d_user || !p->d_decel || !p->d_need_of || !p->d_first || !p->d_harm_at || !p->d_user_at)
      return fo_fail(ctx, FO_E_ARG, "%s: d_need, d_at, d_blocking, d_user, d_decel [M], d_need_of and d_first [C][M], d_harm_at and d_user_at "
                     "[M][L] are required with M > 0", fn);
  } else {
    if (!p->d_need || !p->d_at || !p->d_blocking || !p->d_user || !p->d_decel || !p->d_need_of || !p->d_first)
      return fo_fail(ctx, FO_E_ARG, "%s: d_need, d_at, d_blocking, d_user, d_decel [M], d_need_of and d_first [C][M] are required with M > 0", fn);
  }
  if ((rc = hb_check_cost_pair(ctx, p->d_cost_or_null, p->d_safe_or_null, fn))) return rc;
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  if constexpr (HARM) {
    if (!p->d_speed_of) return fo_fail(ctx, FO_E_ARG, "%s: d_speed_of [C] is required with M > 0", fn);
    if (!p->d_harm_rows) return fo_fail(ctx, FO_E_ARG, "%s: d_harm_rows [C][4] is required with M > 0", fn);
    if (!(p->harm_limit >= 0.0))                                 // (NaN fails the comparison; +inf passes)
      return fo_fail(ctx, FO_E_ARG, "%s: harm_limit = %g, a harm >= 0 (or +inf) is needed", fn, p->harm_limit);
  }
  if constexpr (LANES) {
    if (p->dir_mask >> p->C != 0u)
      return fo_fail(ctx, FO_E_ARG, "%s: dir_mask = 0x%x has bits at or above C = %d", fn, p->dir_mask, p->C);
    if (!(fabs(p->cos_h) <= 1.0) || !(fabs(p->sin_h) <= 1.0))    // (NaN fails the comparison)
      return fo_fail(ctx, FO_E_ARG, "%s: cos_h = %g, sin_h = %g, the cosine and sine of 22.5 deg + heading_slack in [-1, 1] are needed",
                     fn, p->cos_h, p->sin_h);
    if (p->dir_mask != 0u && (rc = hr_check_moves(ctx, fn))) return rc;
  }
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HbuMaps mp = hbu_maps(*p);
  const HbluPack pk = hblu_pack(p->h_levels, L, p->h_thr, C * T);
  const dim3 grid((unsigned)brake_ladder_verdict_blocks(p->M, T, K, L, B)), block(HB_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if constexpr (LANES) {
    const uint32_t dir = p->cos_h > -1.0 ? p->dir_mask : 0u;     // h >= pi: every class is head-on, the table is not read
    const HrBrakeHarmLadderLanesArgs a{p->M, T, B, L, C, brake_ladder_users_width(L), brake_ladder_verdict_group(L, B),
                                       brake_ladder_verdict_per_block(T, K, L, B), p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl,
                                       p->hw, p->wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny,
                                       p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, mp.key[0], mp.key[1], mp.key[2], mp.qmin[0],
                                       mp.qmin[1], mp.qmin[2], mp.map_of, p->d_v, p->d_arc, p->dt, p->a_limit, p->d_speed_of,
                                       p->d_harm_rows, p->harm_limit, sc->map->d_lane_moves, dir, p->cos_h, p->sin_h, p->d_finite_or_null,
                                       p->d_cost_or_null, p->d_safe_or_null, p->d_need, p->d_at, p->d_blocking, p->d_user, p->d_decel,
                                       p->d_need_of, p->d_first, p->d_harm_at, p->d_user_at};
    const size_t lds = brake_harm_ladder_lanes_lds_bytes(T, K, C, L, B);
    if (brake_users_width(C) == 4) hbll_launch<4>(K, grid, block, lds, s, a, pk);
    else hbll_launch<8>(K, grid, block, lds, s, a, pk);
  } else if constexpr (HARM) {
    const HrBrakeHarmLadderArgs a{p->M, T, B, L, C, brake_ladder_users_width(L), brake_ladder_verdict_group(L, B),
                                  brake_ladder_verdict_per_block(T, K, L, B), p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw,
                                  p->wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0,
                                  p->win_iy0, p->win_nx, p->win_ny, mp.key[0], mp.key[1], mp.key[2], mp.qmin[0], mp.qmin[1], mp.qmin[2],
                                  mp.map_of, p->d_v, p->d_arc, p->dt, p->a_limit, p->d_speed_of, p->d_harm_rows, p->harm_limit,
                                  p->d_finite_or_null, p->d_cost_or_null, p->d_safe_or_null, p->d_need, p->d_at, p->d_blocking, p->d_user,
                                  p->d_decel, p->d_need_of, p->d_first, p->d_harm_at, p->d_user_at};
    const size_t lds = brake_harm_ladder_lds_bytes(T, K, C, L, B);
    if (brake_users_width(C) == 4) hbhl_launch<4>(K, grid, block, lds, s, a, pk);
    else hbhl_launch<8>(K, grid, block, lds, s, a, pk);
  } else {
    const HrBrakeLadderVerdictArgs a{p->M, T, B, L, C, brake_ladder_users_width(L), brake_ladder_verdict_group(L, B),
                                     brake_ladder_verdict_per_block(T, K, L, B), p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw,
                                     p->wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0,
                                     p->win_iy0, p->win_nx, p->win_ny, mp.key[0], mp.key[1], mp.key[2], mp.qmin[0], mp.qmin[1], mp.qmin[2],
                                     mp.map_of, p->d_v, p->d_arc, p->dt, p->a_limit, p->d_finite_or_null, p->d_cost_or_null, p->d_safe_or_null,
                                     p->d_need, p->d_at, p->d_blocking, p->d_user, p->d_decel, p->d_need_of, p->d_first};
    const size_t lds = brake_ladder_verdict_lds_bytes(T, K, C, L, B);
    if (brake_users_width(C) == 4) hblv_launch<4>(K, grid, block, lds, s, a, pk);
    else hblv_launch<8>(K, grid, block, lds, s, a, pk);
  }
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

extern "C" {

int fo_scene_hidden_reach(fo_ctx *ctx, const fo_hidden_reach_t *p, void *stream) {
  return hidden_reach_call(ctx, p, false, false, nullptr, "fo_scene_hidden_reach", stream);
}

int fo_scene_hidden_reach_road(fo_ctx *ctx, const fo_hidden_reach_road_t *p, void *stream) {
  return hidden_reach_call(ctx, p ? &p->base : nullptr, true, false, p ? p->d_dist_or_null : nullptr, "fo_scene_hidden_reach_road", stream);
}

int fo_scene_hidden_reach_flow(fo_ctx *ctx, const fo_hidden_reach_road_t *p, void *stream) {
  return hidden_reach_call(ctx, p ? &p->base : nullptr, true, true, p ? p->d_dist_or_null : nullptr, "fo_scene_hidden_reach_flow", stream);
}

// the witness of every trajectory's finding: one launch over the maps of a road / flow forecast (fo_hidden_witness.hpp)
int fo_scene_hidden_witness(fo_ctx *ctx, const fo_hidden_witness_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_witness";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  const fo_hidden_reach_t &b = p->base;
  if (p->flow != 0 && p->flow != 1) return fo_fail(ctx, FO_E_ARG, "%s: flow = %d (0 road, 1 lanes)", fn, p->flow);
  if ((rc = hr_check_forecast(ctx, b, b.d_arrival && p->d_dist,
                              "%s: the maps of the forecast are required (base.d_arrival and d_dist [win_ny][win_nx])", false, fn)))
    return rc;
  const int min_cap = witness_min_cap(b.h_r2[b.J - 1]);
  if (p->path_cap < 0 || p->path_cap % 4 != 0 || p->path_cap < min_cap)
    return fo_fail(ctx, FO_E_ARG, "%s: path_cap = %d, a multiple of 4 that is >= isqrt(169 h_r2[J-1]) / 12 = %d is needed "
                   "(FO_HIDDEN_WITNESS_MAX_STEPS = %d always serves)", fn, p->path_cap, min_cap, FO_HIDDEN_WITNESS_MAX_STEPS);
  if (b.M > 0) {
    if ((rc = hr_check_forecast_samples(ctx, b, fn))) return rc;
    if ((rc = hr_check_forecast_poses(ctx, b, fn))) return rc;
    if (!p->d_cell || !p->d_src || !p->d_steps || !p->d_wdist || (!p->d_dirs && p->path_cap > 0))
      return fo_fail(ctx, FO_E_ARG, "%s: d_cell, d_src [M][2], d_steps, d_wdist [M] and d_dirs [M][path_cap] are required with M > 0", fn);
    if (((uintptr_t)p->d_dirs & 3) != 0)
      return fo_fail(ctx, FO_E_ARG, "%s: d_dirs must be aligned to 4 bytes (its rows are stored as dwords)", fn);
    if ((rc = hr_check_footprint(ctx, b.hl, b.hw, b.wb, fn))) return rc;
  }
  if (p->flow && (rc = hr_check_moves(ctx, fn))) return rc;
  if (b.M == 0) return FO_OK;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HrWitnessArgs a{b.M, b.T, b.d_x, b.d_y, b.d_heading, b.hl, b.hw, b.wb, sc->map->x0, sc->map->y0, sc->map->cs,
                        sc->map->d_raster, sc->map->rnx, sc->map->rny, b.win_ix0, b.win_iy0, b.win_nx, b.win_ny, b.d_arrival,
                        p->d_dist, p->flow ? sc->map->d_lane_moves : nullptr, b.d_first, p->path_cap, p->d_cell, p->d_src,
                        p->d_steps, p->d_wdist, p->d_dirs};
  hipLaunchKernelGGL(fo_hr_witness_kernel, dim3((unsigned)witness_blocks(b.M)), dim3(HR_THREADS), 0, (hipStream_t)stream, a);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the brake clearance of every (trajectory, brake start): one launch over the arrival map of any forecast (fo_hidden_brake.hpp)
int fo_scene_hidden_brake(fo_ctx *ctx, const fo_hidden_brake_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_brake";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  const fo_hidden_reach_t &b = p->base;
  if ((rc = hr_check_forecast(ctx, b, b.d_arrival, "%s: the map of the forecast is required (base.d_arrival [win_ny][win_nx])", false, fn)))
    return rc;
  if ((rc = hb_check_brake(ctx, p->a_brake, p->dt, fn))) return rc;
  if (b.M > 0) {
    if ((rc = hr_check_forecast_samples(ctx, b, fn))) return rc;
    if ((rc = hr_check_forecast_poses(ctx, b, fn))) return rc;
    if ((rc = hb_check_speeds(ctx, p->d_v, p->d_arc, fn))) return rc;
    if (!p->d_brake_first || !p->d_stop || !p->d_commit)
      return fo_fail(ctx, FO_E_ARG, "%s: d_brake_first, d_stop [M][T] and d_commit [M] are required with M > 0", fn);
    if ((rc = hr_check_footprint(ctx, b.hl, b.hw, b.wb, fn))) return rc;
  }
  if (b.M == 0) return FO_OK;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HrBrakeArgs a{b.M, b.T, brake_group(b.T), b.d_x, b.d_y, b.d_heading, b.d_len_or_null, b.hl, b.hw, b.wb, sc->map->x0,
                      sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, b.win_ix0, b.win_iy0, b.win_nx,
                      b.win_ny, b.d_arrival, b.d_first, p->d_v, p->d_arc, p->a_brake, p->dt, p->d_brake_first, p->d_stop, p->d_commit};
  hipLaunchKernelGGL(fo_hr_brake_kernel, dim3((unsigned)brake_blocks(b.M, b.T)), dim3(HB_THREADS), brake_lds_bytes(b.T),
                     (hipStream_t)stream, a);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

int fo_scene_hidden_clearance(fo_ctx *ctx, const fo_hidden_clearance_t *p, void *stream) {
  return hidden_clearance_call(ctx, p, false, "fo_scene_hidden_clearance", stream);
}

int fo_scene_hidden_clearance_flow(fo_ctx *ctx, const fo_hidden_clearance_t *p, void *stream) {
  return hidden_clearance_call(ctx, p, true, "fo_scene_hidden_clearance_flow", stream);
}

// the brake clearance of every (class, trajectory, brake start): one launch over the key map of a clearance call
// (fo_hidden_brake_classes.hpp); the threshold table travels as a kernel argument
int fo_scene_hidden_brake_classes(fo_ctx *ctx, const fo_hidden_brake_classes_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_brake_classes";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if ((rc = hb_check_classes(ctx, p->C, p->h_thr, p->win_nx, p->win_ny, fn))) return rc;
  if (p->r2_cap < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap = %d is negative", fn, p->r2_cap);
  if ((rc = hr_check_halo(ctx, p->r2_cap, "r2_cap", "v_cap", fn))) return rc;
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if ((rc = hb_check_brake(ctx, p->a_brake, p->dt, fn))) return rc;
  if (p->M == 0) return FO_OK;
  const int T = p->T, C = p->C;
  if ((rc = hb_check_samples(ctx, T, fn))) return rc;
  if ((rc = hb_check_table_size(ctx, C, T, fn))) return rc;
  if ((rc = hb_check_rows(ctx, C, T, p->h_thr, &p->r2_cap, nullptr, fn))) return rc;
  if ((rc = hr_check_poses(ctx, p->d_x, p->d_y, p->d_heading, fn))) return rc;
  if (!p->d_key || !p->d_qmin)
    return fo_fail(ctx, FO_E_ARG, "%s: d_key [win_ny][win_nx] and d_qmin [M][T] of the clearance are required with M > 0", fn);
  if ((rc = hb_check_speeds(ctx, p->d_v, p->d_arc, fn))) return rc;
  if (!p->d_brake_first || !p->d_stop || !p->d_commit || !p->d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_brake_first [C][M][T], d_stop [M][T], d_commit and d_first [C][M] are required with M > 0", fn);
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HrBrakeClassesArgs a{p->M, T, brake_group(T), C, p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb,
                             sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0,
                             p->win_iy0, p->win_nx, p->win_ny, p->d_key, p->d_qmin, p->d_v, p->d_arc, p->a_brake, p->dt,
                             p->d_brake_first, p->d_stop, p->d_commit, p->d_first};
  const HbThr thr = hb_thr(p->h_thr, C * T);
  const dim3 grid((unsigned)brake_classes_blocks(p->M, T)), block(HB_THREADS);
  const size_t lds = brake_classes_lds_bytes(T, C);
  hipStream_t s = (hipStream_t)stream;
  switch (brake_classes_width(C)) {
    case 1: hipLaunchKernelGGL(fo_hr_brake_classes_kernel<1>, grid, block, lds, s, a, thr); break;
    case 2: hipLaunchKernelGGL(fo_hr_brake_classes_kernel<2>, grid, block, lds, s, a, thr); break;
    case 4: hipLaunchKernelGGL(fo_hr_brake_classes_kernel<4>, grid, block, lds, s, a, thr); break;
    default: hipLaunchKernelGGL(fo_hr_brake_classes_kernel<8>, grid, block, lds, s, a, thr); break;
  }
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the brake clearance of every (class, trajectory, brake start) over the key maps of up to three clearance calls, each class on the
// map it names: one launch, one walk of every manoeuvre (fo_hidden_brake_users.hpp); map_of and the table travel as kernel arguments
int fo_scene_hidden_brake_users(fo_ctx *ctx, const fo_hidden_brake_users_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_brake_users";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if ((rc = hbu_check_head(ctx, *p, fn))) return rc;
  if ((rc = hb_check_brake(ctx, p->a_brake, p->dt, fn))) return rc;
  if (p->M == 0) return FO_OK;
  const int T = p->T, K = p->K, C = p->C;
  if ((rc = hb_check_samples(ctx, T, fn))) return rc;
  if ((rc = hb_check_table_size(ctx, C, T, fn))) return rc;
  if ((rc = hbu_check_inputs(ctx, *p, fn))) return rc;
  if (!p->d_brake_first || !p->d_stop || !p->d_commit || !p->d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_brake_first [C][M][T], d_stop [M][T], d_commit and d_first [C][M] are required with M > 0", fn);
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HbuMaps mp = hbu_maps(*p);
  const HrBrakeUsersArgs a{p->M, T, brake_group(T), C, p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb,
                           sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0,
                           p->win_iy0, p->win_nx, p->win_ny, mp.key[0], mp.key[1], mp.key[2], mp.qmin[0], mp.qmin[1], mp.qmin[2],
                           mp.map_of, p->d_v, p->d_arc, p->a_brake, p->dt, p->d_brake_first, p->d_stop, p->d_commit, p->d_first};
  const HbThr thr = hb_thr(p->h_thr, C * T);
  const dim3 grid((unsigned)brake_users_blocks(p->M, T)), block(HB_THREADS);
  const size_t lds = brake_users_lds_bytes(T, K, C);
  hipStream_t s = (hipStream_t)stream;
  if (brake_users_width(C) == 4) hbu_launch<4>(K, grid, block, lds, s, a, thr);
  else hbu_launch<8>(K, grid, block, lds, s, a, thr);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the brake clearance of every (trajectory, brake start < B) at every level of a ladder of decelerations, and the first clear level:
// one launch over the arrival map of any forecast (fo_hidden_brake_ladder.hpp); the levels travel as a kernel argument
int fo_scene_hidden_brake_ladder(fo_ctx *ctx, const fo_hidden_brake_ladder_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_brake_ladder";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  const fo_hidden_reach_t &b = p->base;
  if ((rc = hr_check_forecast(ctx, b, b.d_arrival, "%s: the map of the forecast is required (base.d_arrival [win_ny][win_nx])", false, fn)))
    return rc;
  if (p->K < 1 || p->K > FO_HIDDEN_BRAKE_MAX_LEVELS)
    return fo_fail(ctx, FO_E_ARG, "%s: K = %d outside [1, FO_HIDDEN_BRAKE_MAX_LEVELS = %d]", fn, p->K, FO_HIDDEN_BRAKE_MAX_LEVELS);
  if (!p->h_levels) return fo_fail(ctx, FO_E_ARG, "%s: no decelerations h_levels [K]", fn);
  if ((rc = hb_check_level_values(ctx, p->K, p->h_levels, fn))) return rc;
  if ((rc = hb_check_dt(ctx, p->dt, fn))) return rc;
  if (b.M > 0) {
    if ((rc = hr_check_forecast_samples(ctx, b, fn))) return rc;
    if ((rc = hb_check_starts(ctx, p->B, b.T, fn))) return rc;
    if ((rc = hr_check_forecast_poses(ctx, b, fn))) return rc;
    if ((rc = hb_check_speeds(ctx, p->d_v, p->d_arc, fn))) return rc;
    if (!p->d_brake_first || !p->d_stop || !p->d_required || !p->d_last_unclear || !p->d_commit)
      return fo_fail(ctx, FO_E_ARG, "%s: d_brake_first, d_stop [M][B][K], d_required, d_last_unclear [M][B] and d_commit [M][K] are required "
                     "with M > 0", fn);
    if ((rc = hr_check_footprint(ctx, b.hl, b.hw, b.wb, fn))) return rc;
  }
  if (b.M == 0) return FO_OK;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HrBrakeLadderArgs a{b.M, b.T, p->B, p->K, brake_ladder_width(p->K), brake_ladder_group(b.T, p->K, p->B), b.d_x, b.d_y, b.d_heading,
                            b.d_len_or_null, b.hl, b.hw, b.wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx,
                            sc->map->rny, b.win_ix0, b.win_iy0, b.win_nx, b.win_ny, b.d_arrival, b.d_first, p->d_v, p->d_arc, p->dt,
                            p->d_brake_first, p->d_stop, p->d_required, p->d_last_unclear, p->d_commit};
  HbLevels lv;
  for (int k = 0; k < FO_HIDDEN_BRAKE_MAX_LEVELS; ++k) lv.v[k] = k < p->K ? p->h_levels[k] : 0.0;
  hipLaunchKernelGGL(fo_hr_brake_ladder_kernel, dim3((unsigned)brake_ladder_blocks(b.M, b.T, p->K, p->B)), dim3(HB_THREADS),
                     brake_ladder_lds_bytes(b.T, p->K, p->B), (hipStream_t)stream, a, lv);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the brake ladder of every (trajectory, brake start < B) against every class of road user on the key map it names, and the first
// level clear of all of them: one launch (fo_hidden_brake_ladder_users.hpp); the levels, map_of and the table travel as kernel arguments
int fo_scene_hidden_brake_ladder_users(fo_ctx *ctx, const fo_hidden_brake_ladder_users_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_brake_ladder_users";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if ((rc = hbu_check_head(ctx, *p, fn))) return rc;
  if ((rc = hb_check_levels(ctx, p->L, p->h_levels, false, fn))) return rc;
  if ((rc = hb_check_dt(ctx, p->dt, fn))) return rc;
  if (p->M == 0) return FO_OK;
  const int T = p->T, B = p->B, K = p->K, C = p->C, L = p->L;
  if ((rc = hb_check_samples(ctx, T, fn))) return rc;
  if ((rc = hb_check_starts(ctx, B, T, fn))) return rc;
  if ((rc = hb_check_table_size(ctx, C, T, fn))) return rc;
  if ((rc = hb_check_arg_bytes(ctx, C, T, L, fn))) return rc;
  if ((rc = hbu_check_inputs(ctx, *p, fn))) return rc;
  if (!p->d_required || !p->d_last_unclear || !p->d_commit || !p->d_first || !p->d_required_all || !p->d_last_unclear_all || !p->d_blocking)
    return fo_fail(ctx, FO_E_ARG, "%s: d_required, d_last_unclear [C][M][B], d_commit [C][M][L], d_first [C][M], d_required_all, "
                   "d_last_unclear_all and d_blocking [M][B] are required with M > 0", fn);
  if (!p->d_brake_first_or_null != !p->d_stop_or_null)
    return fo_fail(ctx, FO_E_ARG, "%s: the detail d_brake_first_or_null [C][M][B][L] and d_stop_or_null [M][B][L] is given whole or not "
                   "at all (%s is missing)", fn, p->d_stop_or_null ? "d_brake_first_or_null" : "d_stop_or_null");
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HbuMaps mp = hbu_maps(*p);
  const HrBrakeLadderUsersArgs a{p->M, T, B, L, C, brake_ladder_users_width(L), brake_ladder_users_group(T, K, L, B), p->d_x, p->d_y,
                                 p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0, sc->map->cs,
                                 sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, mp.key[0],
                                 mp.key[1], mp.key[2], mp.qmin[0], mp.qmin[1], mp.qmin[2], mp.map_of, p->d_v, p->d_arc, p->dt,
                                 p->d_required, p->d_last_unclear, p->d_commit, p->d_first, p->d_required_all, p->d_last_unclear_all,
                                 p->d_blocking, p->d_brake_first_or_null, p->d_stop_or_null};
  const HbluPack pk = hblu_pack(p->h_levels, L, p->h_thr, C * T);
  const dim3 grid((unsigned)brake_ladder_users_blocks(p->M, T, K, L, B)), block(HB_THREADS);
  const size_t lds = brake_ladder_users_lds_bytes(T, K, C, L, B);
  hipStream_t s = (hipStream_t)stream;
  if (brake_users_width(C) == 4) hblu_launch<4>(K, grid, block, lds, s, a, pk);
  else hblu_launch<8>(K, grid, block, lds, s, a, pk);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// (cos, sin) of the headings, the travelled arc and the finite flag of every candidate, on the device: one launch
// (fo_hidden_poses.hpp); needs no scene
int fo_scene_hidden_poses(fo_ctx *ctx, const fo_hidden_poses_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_poses";
  if (!ctx) return fo_fail(ctx, FO_E_STATE, "%s: no context", fn);
  if (!p) return fo_fail(ctx, FO_E_ARG, "%s: no parameters", fn);
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (p->M == 0) return FO_OK;
  if (int rc = hb_check_samples(ctx, p->T, fn)) return rc;
  if (!p->d_x || !p->d_y || !p->d_theta || !p->d_v) return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y, d_theta and d_v [M][T] are required with M > 0", fn);
  if (!p->d_heading || !p->d_arc || !p->d_finite)
    return fo_fail(ctx, FO_E_ARG, "%s: d_heading [M][T][2], d_arc [M][T] and d_finite [M] are required with M > 0", fn);
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HiddenPosesArgs a{p->M, p->T, p->d_x, p->d_y, p->d_theta, p->d_v, p->d_len_or_null, p->d_heading, p->d_arc, p->d_finite};
  hipLaunchKernelGGL(fo_hidden_poses_kernel, dim3((unsigned)poses_blocks(p->M)), dim3(POSES_THREADS), 0, (hipStream_t)stream, a);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the fail-safe verdict of every trajectory over its first B brake starts against every class of road user on the key map it names,
// folded into the reserved cost columns and the safety flag: one launch (fo_hidden_brake_verdict.hpp); map_of and the table travel as
// kernel arguments
int fo_scene_hidden_brake_verdict(fo_ctx *ctx, const fo_hidden_brake_verdict_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_brake_verdict";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if ((rc = hbu_check_head(ctx, *p, fn))) return rc;
  if ((rc = hb_check_brake(ctx, p->a_brake, p->dt, fn))) return rc;
  if (p->M == 0) return FO_OK;
  const int T = p->T, B = p->B, K = p->K, C = p->C;
  if ((rc = hb_check_samples(ctx, T, fn))) return rc;
  if ((rc = hb_check_starts(ctx, B, T, fn))) return rc;
  if (p->commit_min < 0 || p->commit_min > B)
    return fo_fail(ctx, FO_E_ARG, "%s: commit_min = %d outside [0, B = %d]", fn, p->commit_min, B);
  if ((rc = hb_check_table_size(ctx, C, T, fn))) return rc;
  if ((rc = hbu_check_inputs(ctx, *p, fn))) return rc;
  if (!p->d_fail_safe || !p->d_user || !p->d_commit || !p->d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_fail_safe, d_user [M], d_commit and d_first [C][M] are required with M > 0", fn);
  if ((rc = hb_check_cost_pair(ctx, p->d_cost_or_null, p->d_safe_or_null, fn))) return rc;
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HbuMaps mp = hbu_maps(*p);
  const HrBrakeVerdictArgs a{p->M, T, brake_verdict_group(B), brake_verdict_per_block(T, K, B), C, B, p->commit_min, p->d_x, p->d_y,
                             p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0, sc->map->cs,
                             sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, mp.key[0],
                             mp.key[1], mp.key[2], mp.qmin[0], mp.qmin[1], mp.qmin[2], mp.map_of, p->d_v, p->d_arc, p->a_brake, p->dt,
                             p->d_finite_or_null, p->d_cost_or_null, p->d_safe_or_null, p->d_fail_safe, p->d_user, p->d_commit,
                             p->d_first};
  const HbThr thr = hb_thr(p->h_thr, C * T);
  const dim3 grid((unsigned)brake_verdict_blocks(p->M, T, K, B)), block(HB_THREADS);
  const size_t lds = brake_verdict_lds_bytes(T, K, C, B);
  hipStream_t s = (hipStream_t)stream;
  if (brake_users_width(C) == 4) hbv_launch<4>(K, grid, block, lds, s, a, thr);
  else hbv_launch<8>(K, grid, block, lds, s, a, thr);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the impact verdict, head-on and by approach angle: hidden_brake_impact_call above
int fo_scene_hidden_brake_impact(fo_ctx *ctx, const fo_hidden_brake_impact_t *p, void *stream) {
  return hidden_brake_impact_call<false>(ctx, p, "fo_scene_hidden_brake_impact", stream);
}

int fo_scene_hidden_brake_impact_lanes(fo_ctx *ctx, const fo_hidden_brake_impact_lanes_t *p, void *stream) {
  return hidden_brake_impact_call<true>(ctx, p, "fo_scene_hidden_brake_impact_lanes", stream);
}

// the harm row of a class of hidden road user (fo_hidden_impact.hpp), for the caller that builds d_harm_rows
int fo_hidden_impact_row(int type, double size, double ego_mass, const fo_harm_coeff_t *hc, double *row) {
  if (!hc || !row || !(size > 0.0) || !(size < INFINITY) || !(ego_mass > 0.0) || !(ego_mass < INFINITY)) return FO_E_ARG;
  double r[4];
  if (!fo_hidden_impact_row_of(type, size, ego_mass, *hc, r)) return FO_E_ARG;
  for (int i = 0; i < 4; ++i) row[i] = r[i];
  return FO_OK;
}

// the ladder verdict and the harm ladder: hidden_brake_ladder_verdict_call above
int fo_scene_hidden_brake_ladder_verdict(fo_ctx *ctx, const fo_hidden_brake_ladder_verdict_t *p, void *stream) {
  return hidden_brake_ladder_verdict_call<HBLV_VERDICT>(ctx, p, "fo_scene_hidden_brake_ladder_verdict", stream);
}

int fo_scene_hidden_brake_harm_ladder(fo_ctx *ctx, const fo_hidden_brake_harm_ladder_t *p, void *stream) {
  return hidden_brake_ladder_verdict_call<HBLV_HARM>(ctx, p, "fo_scene_hidden_brake_harm_ladder", stream);
}

int fo_scene_hidden_brake_harm_ladder_lanes(fo_ctx *ctx, const fo_hidden_brake_harm_ladder_lanes_t *p, void *stream) {
  return hidden_brake_ladder_verdict_call<HBLV_HARM_LANES>(ctx, p, "fo_scene_hidden_brake_harm_ladder_lanes", stream);
}

}  // extern "C"
