/* fo_hip.h -- C ABI of the MI355X (gfx950) implementation of the Frenetix-Occlusion per-timestep hot path.
 *
 * Shared library: frenetix-occlusion_amd/lib/libfo_hip.so  (built by __graft_entry__.build()).
 * All pointers named d_* are DEVICE pointers (HBM), caller-owned, and must stay valid until the work queued on
 * `stream` (a hipStream_t passed as void*; NULL = the default stream) has completed.  No torch types, no C++
 * types, no exceptions cross this boundary: every entry point returns 0 or a negative FO_E_* code and
 * fo_last_error(ctx) gives the message.  One context per ego vehicle per GPU; a context is not re-entrant
 * (same ownership model as one FOInterface instance, /root/reference/frenetix_occlusion/interface.py:85-90).
 *
 * Citations "ref:" are relative to /root/reference/frenetix_occlusion/.
 *
 * Array layouts (float64 unless noted):
 *   trajectories  x,y,theta,v,a : [M][T]   row = one candidate trajectory (trajectory.cartesian.*, ref: interface.py:216)
 *   agent predictions           : pos [A][Ta][2], yaw [A][Ta], v [A][Ta], cov [A][Ta][4] (xx,xy,yx,yy),
 *                                 shape [A][2] = prediction['shape'] (inflated length,width; ref: agent.py:404-409,523-524),
 *                                 raw_dims [A][2] = agent.shape (ref: agent.py:216), type int32 [A] (FO_TYPE_*),
 *                                 len int32 [A] = number of valid samples of that prediction (1..Ta; 0 = inactive slot)
 *   outputs, trajectory index fastest (lane = trajectory):
 *     cost   [M][FO_NC]                 per-trajectory cost vector (the unit all-gathered across GPUs)
 *     safe   uint8 [M]                  safety_assessment of metric.py:50-100
 *     pair_f [FO_NPF][A][M]             per (trajectory, agent) scalars
 *     pair_i int32 [FO_NPI][A][M]
 *     lists  FO_NL A (T-1) M doubles    per-timestep lists of hr.py:87-98 (NaN past the reference's list length), n = A (T-1) M
 *                                       entries each, in three blocks: collision probability [A][T-1][M] at offset 0;
 *                                       (ego harm, obstacle harm) pairs [A][T-1][M][2] at offset n; (ego risk, obstacle risk)
 *                                       pairs [A][T-1][M][2] at offset 3 n -- a GPU lane writes one sample with three
 *                                       stores of 8 + 16 + 16 bytes, each contiguous across the trajectories of a wave
 */
#ifndef FO_HIP_H
#define FO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FO_ABI_VERSION 12

enum { FO_OK = 0, FO_E_ARG = -1, FO_E_UNSUPPORTED_COV = -2, FO_E_HIP = -3, FO_E_NOMEM = -4, FO_E_STATE = -5 };

/* commonroad ObstacleType strings -> codes (ref: metrics/utils/harm_model.py:15-32) */
enum {
  FO_TYPE_CAR = 0, FO_TYPE_TRUCK = 1, FO_TYPE_BUS = 2, FO_TYPE_BICYCLE = 3, FO_TYPE_PEDESTRIAN = 4,
  FO_TYPE_PRIORITY_VEHICLE = 5, FO_TYPE_PARKED_VEHICLE = 6, FO_TYPE_TRAIN = 7, FO_TYPE_MOTORCYCLE = 8,
  FO_TYPE_TAXI = 9, FO_TYPE_UNKNOWN = 10, FO_TYPE_STRUCTURE = 11
};

/* activated_metrics bits (ref: metrics/metric.py:109-117; dependency closure :125-147 is applied inside) */
enum { FO_M_DCE = 1, FO_M_CP = 2, FO_M_TTC = 4, FO_M_TTCE = 8, FO_M_WTTC = 16, FO_M_BE = 32, FO_M_HR = 64 };

/* vehicle_params attributes the path reads (ref: convert_dynamic_obstacle.py:60,78; collision_probability.py:35;
 * harm_model.py:96-97; be.py:56) */
typedef struct { double length, width, wb_rear_axle, mass, a_max; } fo_vehicle_t;

/* coefficients read from config/harm_params.json (ref: harm_params.json:26-29,40-45,98-101) */
typedef struct {
  double lr4s_const, lr4s_speed, lr4s_side, lr4s_rear;
  double lr1s_const, lr1s_speed;
  double ped_const, ped_speed;
} fo_harm_coeff_t;

/* metrics.metric_thresholds of the YAML (ref: config/config.yaml:14-22); NaN = null = check disabled */
typedef struct { double harm, risk, be, cp, ttc, dce; } fo_thresholds_t;

enum { FO_PF_DCE = 0, FO_PF_TTC, FO_PF_TTCE, FO_PF_MAX_EGO_RISK, FO_PF_MAX_OBST_RISK, FO_PF_HARM_WITH_CP,
       FO_PF_MAX_EGO_HARM, FO_PF_MAX_OBST_HARM, FO_PF_MAX_CP, FO_PF_BE_DECEL, FO_PF_BE_BTN, FO_PF_SPARE, FO_NPF = 12 };
enum { FO_PI_TIME_DCE = 0, FO_PI_RISK_INDEX, FO_PI_CP_ARGMAX, FO_PI_HR_VALID, FO_NPI = 4 };
enum { FO_L_CP = 0, FO_L_EGO_HARM, FO_L_OBST_HARM, FO_L_EGO_RISK, FO_L_OBST_RISK, FO_NL = 5 };
enum { FO_C_WTTC = 0, FO_C_MIN_DCE, FO_C_MAX_EGO_RISK, FO_C_MAX_OBST_RISK, FO_C_MAX_EGO_HARM, FO_C_MAX_OBST_HARM,
       FO_C_MAX_CP, FO_C_HARM_WITH_CP, FO_C_MIN_TTCE, FO_C_ARGMIN_DCE, FO_C_ARGMIN_TTC, FO_C_ARGMAX_RISK,
       FO_C_SAFE, FO_C_MAX_BTN, FO_C_RES0, FO_C_RES1, FO_NC = 16 };

typedef struct fo_ctx fo_ctx;

/* ---- context -------------------------------------------------------------------------------------------- */
int fo_create(fo_ctx **out, int device);            /* replaces: FOInterface.__init__ native state (interface.py:69-131) */
void fo_destroy(fo_ctx *ctx);
const char *fo_last_error(const fo_ctx *ctx);       /* replaces: Python exceptions (SURVEY 8b "error conventions") */
int fo_abi_version(void);
/* SHA-256 (hex) of the sources and flags this library was built from (__graft_entry__.source_id()): build(), smoke()
 * and bench.py compare it with the tree they run in, so a stale prebuilt library cannot pass for the current one */
const char *fo_build_id(void);

/* ---- metric sweep: replaces M calls of FOInterface.trajectory_safety_assessment (interface.py:216-219 ->
 *      metrics/metric.py:35-100 -> dce.py, ttc.py, ttce.py, wttc.py, cp.py, hr.py) ------------------------ */
int fo_sweep_configure(fo_ctx *ctx, const fo_vehicle_t *veh, const fo_harm_coeff_t *hc, const fo_thresholds_t *thr,
                       uint32_t metric_mask, double dt);        /* Metric.__init__ (metric.py:22-33), HR._load_param */

/* pre-size the context's HBM workspace so that fo_sweep_run never allocates (needed before hipGraph capture) -- for EVERY
 * batch of at most max_M trajectories, max_A agent slots and horizons up to max_T (a smaller batch may take the kernel's
 * horizon-split form, which keeps more partial rows per trajectory: the reservation covers that case as well) */
int fo_sweep_reserve(fo_ctx *ctx, int max_M, int max_T, int max_A, int max_Ta);

/* Element type of the per-timestep lists (d_lists of fo_sweep_run).  FO_LISTS_F64 (default): float64, the reference's
 * own numpy dtype (hr.py:87-98) -- what the parity tests hold to 1e-9.  FO_LISTS_F32: the same three blocks with float32
 * elements (cp float [n], harm float2 [n], risk float2 [n]; n = A (T-1) M), the storage SURVEY 8d prices at 648 B per
 * pair.  Collision probabilities and risks are the float64 results rounded at the store; harm entries away from the 5 m
 * gate are evaluated in float32 (hardware exp / rcp, |error| < 4e-7 -- north_star's tolerance is 1e-5).  cost, safe,
 * pair_f and pair_i are float64 / exact and bit-identical in both formats. */
/* FO_LISTS_F32_EXACT: float32 elements in the same layout as FO_LISTS_F32, every entry the float64 result rounded at the
 * store (the arithmetic of FO_LISTS_F64, the bytes of FO_LISTS_F32; bench.py times it beside FO_LISTS_F32 so that the
 * price of the float32 harm entries is a number). */
enum { FO_LISTS_F64 = 0, FO_LISTS_F32 = 1, FO_LISTS_F32_EXACT = 2 };
int fo_sweep_set_list_format(fo_ctx *ctx, int format);

/* replaces: agent_manager.predictions (agent.py:179-183) as read by every metric.
 * d_len [A]: valid samples of every prediction, clamped to [0, Ta] (a negative length is an unused slot, like 0).  ONE
 * value, FO_LEN_REFUSED (INT32_MIN: what fo_scene_spawn_rule_agents leaves in the first rule slot of a refused rule list),
 * counts as 0 live samples too AND marks the whole set as one that cannot be judged: see "A refused rule list" at
 * fo_sweep_check. */
#define FO_LEN_REFUSED (-2147483647 - 1)
int fo_sweep_set_agents(fo_ctx *ctx, int A, int Ta, const double *d_pos, const double *d_yaw, const double *d_v,
                        const double *d_cov, const double *d_shape, const double *d_raw_dims, const int32_t *d_type,
                        const int32_t *d_len, void *stream);

/* d_pair_f / d_pair_i / d_lists may be NULL (reduced output mode); d_cost and d_safe are required.
 * d_a (acceleration profile) may be NULL unless FO_M_BE is active (ref: metrics/be.py:66-68 reads cartesian.a).
 * FO_M_BE implies FO_M_TTC and FO_M_DCE (be.py:39,49 read results['ttc']); its per-pair outputs are
 * pair_f[FO_PF_BE_DECEL], pair_f[FO_PF_BE_BTN] (0 for pairs that do not collide, be.py:45-46) and the per-trajectory
 * maximum goes to cost[FO_C_MAX_BTN]; thresholds.be is applied like metric.py:54-61. */
int fo_sweep_run(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, const double *d_theta,
                 const double *d_v, const double *d_a, double *d_cost, uint8_t *d_safe, double *d_pair_f,
                 int32_t *d_pair_i, double *d_lists, void *stream);

/* The sweep kernel gives every wave `agents per wave` agents of a tile; the best value (1, 2, 4 or 8) depends on the batch
 * shape (how many workgroups the grid has against the chip's 768 slots).  fo_sweep_run picks one by a static rule;
 * fo_sweep_autotune MEASURES the four settings on the caller's own batch -- `reps` launches each, HIP events on `stream` --
 * and remembers the fastest for every later fo_sweep_run / fo_step_run on this context with the same shape (number of
 * 64-trajectory tiles, agent slots, horizon, output mode, list format).  Arguments as for fo_sweep_run (agents set
 * before); the outputs hold a complete result afterwards.  best_apw / ms4 [4] (ms per launch for 1, 2, 4, 8) may be
 * NULL.  Synchronises the stream; call it once when a planning loop starts.  (No counterpart in the reference.) */
int fo_sweep_autotune(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, const double *d_theta,
                      const double *d_v, const double *d_a, double *d_cost, uint8_t *d_safe, double *d_pair_f,
                      int32_t *d_pair_i, double *d_lists, int reps, int *best_apw, double *ms4, void *stream);

/* Blocks until `stream` has drained, then returns FO_E_UNSUPPORTED_COV if the last fo_sweep_set_agents met a matrix
 * that is no usable covariance -- asymmetric, not positive, or |correlation| > 0.99 (those agents' collision
 * probabilities are NaN and no trajectory reads as safe) -- else FO_OK.  Diagonal covariances take the closed form,
 * symmetric ones with correlation are integrated numerically (the reference hands any matrix to scipy's mvnun,
 * collision_probability.py:117).  Not capturable in a hipGraph.
 *
 * A refused rule list.  When the spawn rule families ran out of table space at a step (fo_scene_spawn_rules:
 * *d_n_out = -1), the agent set of that step is short of road users the reference would have put there, and a sweep over
 * it delivers NO usable verdict -- on the device, without any host read, whether or not anybody calls this function.
 * For every trajectory m: safe[m] = 0, cost[m][FO_C_SAFE] = 0, every other float column of cost[m] is NaN, FO_C_RES0 and
 * FO_C_RES1 keep their 0.  That holds in every output mode, for every metric mask (unlike the covariance poison it is not
 * gated on CP / HR), for FO_SPAWN_RULES and FO_SPAWN_BOTH, in both forms of fo_step_run, and for the stage calls
 * fo_scene_spawn_rule_agents -> fo_sweep_set_agents -> fo_sweep_run.  The pair and list buffers of such a step are
 * UNSPECIFIED: do not read them.  fo_sweep_check then returns FO_E_STATE with a message that names the rule tables (an
 * unusable covariance in the same set is reported first).  The mark carries the generation of its agent set: the next
 * fo_sweep_set_agents / fo_step_run on the context starts clean.  A fo_scene_hidden_brake_verdict stage queued behind such a
 * step writes FO_C_RES0 and FO_C_RES1 of the poisoned rows too (its fail_safe and user), and leaves their NaNs, safe = 0 and
 * FO_C_SAFE = 0 as they are: it only ever takes safety away. */
int fo_sweep_check(fo_ctx *ctx, void *stream);

/* HIP-event timing of the sweep kernel alone (events recorded on the launch stream around that one kernel):
 * enable, run K times (at most 1024 timed launches), then read the summed duration and the number of timed launches.
 * enable = k > 1 puts the event pair around every k-th launch only (the two event records cost a few microseconds of
 * stream time each).  fo_sweep_timing_read synchronises. */
int fo_sweep_timing(fo_ctx *ctx, int enable);
int fo_sweep_timing_read(fo_ctx *ctx, double *total_ms, int *launches);
/* the same read-out launch by launch: each_ms[i] = duration of the i-th timed launch, i < min(*launches, cap) */
int fo_sweep_timing_read_each(fo_ctx *ctx, double *each_ms, int cap, int *launches);

/* launch geometry of the last sweep launch (for profiling scripts) */
int fo_sweep_last_launch(const fo_ctx *ctx, int *grid, int *block, int *agents_per_wave);

/* ---- scene: visibility / occlusion / phantom spawn ------------------------------------------------------------
 * The reference computes these with GEOS polygon algebra; this library uses a polar ray fan + a cell grid (the
 * discretisation is specified in DESIGN.md).  Occluder ids: 0..E-1 = map boundary edge, E + o = obstacle o, -1 = none
 * within range.  Cell class bits: 1 road, 2 visible, 4 occluded.  Cells are indexed iy * win_nx + ix inside the
 * window whose lower-left raster cell is (win_ix0, win_iy0). */

/* One-off (replaces SensorModel.__init__ / _convert_lanelet_network, sensor_model.py:17-39,195-199): HOST arrays.
 * polygons: P lanelet polygons, vertices poly_xy[poly_off[p] .. poly_off[p+1]); edges [E][4] = occluding boundary
 * segments (ax, ay, bx, by); cs = cell size; margin = raster margin around the polygons' bounding box.
 * lane_yaw (optional, [rny][rnx], NaN off-lane) must match the raster geometry, which the caller may fix with
 * raster_origin[2] / raster_dims[2] (else it is derived from the bounding box and reported by fo_scene_map_info). */
int fo_scene_set_map(fo_ctx *ctx, int P, const int32_t *h_poly_off, const double *h_poly_xy, int E,
                     const double *h_edges, double cs, double margin, const double *h_lane_yaw_or_null,
                     const double *h_raster_origin_or_null, const int32_t *h_raster_dims_or_null);
/* Instead of fo_scene_set_map: let `ctx` read the static map (boundary pieces and their chunk boxes, road and
 * lane-heading rasters, chain labels, route table) that `owner` -- another context on the same device -- has uploaded,
 * by reference.  Several egos planning on one scenario on one GPU (BASELINE configs[4]: "shared occlusion map in HBM")
 * then hold the map once; every per-step buffer stays per context.  Reference counted: destroying the owner does not
 * pull the map away, and a later fo_scene_set_map gives the calling context a map of its own again.  (No counterpart in
 * the reference, which builds one shapely road polygon per SensorModel, sensor_model.py:195-199.)
 * The route table and the edge-line labels are part of the map: upload them through the owner BEFORE sharing.  While a
 * map has more than one reader, fo_scene_set_routes / fo_scene_set_edge_lines on any of them return FO_E_STATE (they
 * would free tables other contexts' kernels are reading); fo_scene_set_map detaches the caller first and is always
 * allowed.  The reference count is atomic: sharing and destroying from different host threads is safe. */
int fo_scene_share_map(fo_ctx *ctx, fo_ctx *owner);
/* One-off, after fo_scene_set_map (replaces FORoutePlanner, route_planner.py:15-90, evaluated for every lanelet up
 * front): HOST arrays.  Lanelet index p (order of the polygons given to fo_scene_set_map) has up to R candidate routes;
 * route r occupies vertices [first[p*R+r], first[p*R+r] + count[p*R+r]) of xy [NV][2] / s [NV] (arc length from the
 * route's first vertex); count 0 = no such route.  lanelet_raster int32 [rny][rnx]: lanelet index per raster cell, -1
 * off-lane. */
int fo_scene_set_routes(fo_ctx *ctx, int P, int R, const int32_t *h_first, const int32_t *h_count, int NV,
                        const double *h_xy, const double *h_s, const int32_t *h_lanelet_raster);
/* One-off, optional, after fo_scene_set_map: HOST int32 [E], label in [0, E) of the straight-line chain each boundary
 * piece belongs to (pieces that continue one another in a straight line; lanelet bounds are sampled polylines).  Two
 * rays that stop on the same chain see one occluder, which keeps the exact settlement of fo_scene_visibility to the
 * cells at real corners and depth discontinuities.  Without it every piece is its own chain. */
int fo_scene_set_edge_lines(fo_ctx *ctx, int E, const int32_t *h_line);
int fo_scene_map_info(fo_ctx *ctx, double *x0, double *y0, double *cs, int *nx, int *ny, int *n_edges);
/* Where an obstacle's shadow ends.  The reference builds an obstacle's occlusion polygon from the two silhouette corners
 * and the points `length` = 100 m beyond them along the sight lines (helper_functions.py:139-176: get_polygon_from_obstacle_
 * occlusion, _identify_projection_points): behind the chord between those two end points the obstacle hides nothing.  Seen
 * from close by (a 9 m truck within ~1.5 m) that chord falls inside the sensor range.  Default 100.0 = the reference's;
 * <= 0 or infinity = shadows without end.  Applied where cells are settled exactly (exact_cells of fo_scene_visibility:
 * every cell behind an obstacle is); the first-hit ranges / hit ids / the visible polygon's ring are unaffected.  The
 * reference's boundary shadows end at 101 x the vertex distance (:91-92), which the ray fan does not represent: inside
 * 1.5 r = 75 m that takes a boundary vertex within 0.74 m of the ego. */
int fo_scene_set_shadow_length(fo_ctx *ctx, double length);
int fo_scene_copy_raster(fo_ctx *ctx, uint8_t *h_out);

/* Ray fan about the ego heading, written on the device (replaces the angle bookkeeping of
 * _calc_visible_area_from_lanelet_geometry / _calc_relevant_sector, sensor_model.py:115-124,201-209).
 * d_dirs [n_rays][2]: full circle (fov_deg >= 359.9) angle_i = yaw + 2 pi i / n, else n rays from yaw - fov/2 to
 * yaw + fov/2 inclusive.  d_rmax [n_rays] (may be NULL): range of the sensor footprint along each ray; with
 * polygon_footprint != 0 the reference's inscribed polygon (Point.buffer(r) = regular 64-gon with a vertex at world
 * angle 0 [ext shapely default], or ego + 100 arc points), else r.  d_half [100][2] (may be NULL): unit directions of
 * the 100-point half fan about the heading whose radius-1.5 r polygon bounds the occluded area (sensor_model.py:85-93);
 * fo_scene_visibility takes it as d_half (NULL there = the true half disc). */
int fo_scene_fan(fo_ctx *ctx, int n_rays, double ego_yaw, double fov_deg, double r, int polygon_footprint,
                 double *d_dirs, double *d_rmax, double *d_half, void *stream);

/* Per step (replaces SensorModel.calc_visible_and_occluded_area, sensor_model.py:41-101).  d_dirs [n_rays][2] unit
 * ray directions in counter-clockwise order (full_circle: ray n_rays == ray 0); d_rmax [n_rays] (or NULL = r) range of
 * the sensor footprint along each ray -- the reference's footprint is a polygon (Point.buffer(r): regular 64-gon,
 * or the 100-point fan of _calc_relevant_sector, sensor_model.py:118-124,201-209); d_edge_skip [E] (or NULL = none)
 * marks boundary pieces that cast no shadow this step: rings of the road union enclosed by the footprint are interior
 * rings of road ∩ footprint and the reference walks exterior rings only (sensor_model.py:126-131).  Obstacles at this step:
 * d_ocorn [O][4][2] corner points (fo_obstacle.py:79-93), d_ocen [O][2], d_oflags [O] (bit0 present, bit1 occludes --
 * clear for bicycles, sensor_model.py:177).  Outputs: d_range/d_hit_id [n_rays], d_ring [n_rays][2] (vertices of the
 * visible polygon = what evaluate_scenario returns), d_obst_vis [O] (visible_objects_timestep), d_cls [ny][nx],
 * d_occ_idx (ascending, capacity nx*ny) + d_n_occ [1].  d_cls: 4-byte aligned, capacity rounded up to whole 32-bit words
 * (class bits are cleared with word atomics).
 * Cell classes: a road cell within r is visible iff its centre lies on the ego side of the chord between the hit points
 * of the two rays enclosing it.  exact_cells != 0: where those two rays stop at different occluders (or at an
 * obstacle) and the centre is not nearer than the shorter of the two by more than a cell, the fan cannot decide and
 * the cell is settled by the reference's own set algebra at the centre -- visible iff inside the footprint and no
 * occluding piece crosses the open segment ego -> centre (= the centre is in none of the shadow quads of
 * helper_functions.py:79-96 / occlusion polygons of :133-141); and no visible cell's centre lies within 5 mm of a
 * present non-bicycle obstacle (the buffered obstacle the reference subtracts, sensor_model.py:183). */
int fo_scene_visibility(fo_ctx *ctx, double ego_x, double ego_y, double head_x, double head_y, double r, int full_circle,
                        int exact_cells, int n_rays, const double *d_dirs, const double *d_rmax, const double *d_half,
                        const uint8_t *d_edge_skip, int O, const double *d_ocorn, const double *d_ocen,
                        const uint8_t *d_oflags, int win_ix0, int win_iy0, int win_nx, int win_ny, double *d_range,
                        int32_t *d_hit_id, double *d_ring, uint8_t *d_obst_vis, uint8_t *d_cls, int32_t *d_occ_idx,
                        int32_t *d_n_occ, void *stream);

/* EXTENSION, not part of the reference: occlusion memory.  Arms `ctx` for its NEXT visibility stage only
 * (fo_scene_visibility, or the visibility part of fo_step_run; NULL or no call = off: no launch, no buffer touched).  That
 * stage then keeps a settled occluded cell g occluded only if a hidden road user could have reached it since the previous
 * step: H(g) = 0 if visible; if occluded, 1 iff P(g + d) = 1 for some d with dx^2 + dy^2 <= r2; else the road bit.
 * P = H of the previous step inside its window (prev_*), the road raster outside it, 0 off the raster; reset != 0 makes
 * P = the road raster everywhere (the classes are then those of an unarmed stage).  Where H = 0 bit 4 of the class and the
 * cell's entry in the occluded list go away; H [win_ny][win_nx] (uint8 0 / 1) is written to d_cur, which the caller passes
 * as d_prev one step later (ping-pong: d_prev != d_cur).  One launch between the settlement and the compaction.
 * FO_E_ARG: r2 outside [0, FO_OCCLUSION_MEMORY_MAX_HALO^2], no d_cur, or (reset == 0) no d_prev / a d_prev smaller than
 * prev_nx * prev_ny bytes; the visibility stage returns FO_E_ARG when cur_bytes < win_nx * win_ny. */
#define FO_OCCLUSION_MEMORY_MAX_HALO 32
typedef struct {
  int32_t r2;                                   /* reach in cells, squared and floored: D = {(dx, dy) : dx^2 + dy^2 <= r2} */
  int32_t reset;                                /* != 0: P = road raster (first step, time going backwards, ...) */
  int32_t prev_ix0, prev_iy0, prev_nx, prev_ny; /* window of d_prev (unread when reset) */
  const uint8_t *d_prev;                        /* [prev_ny][prev_nx] H of the previous step (unread when reset) */
  uint8_t *d_cur;                               /* H of this step, [win_ny][win_nx] */
  int64_t prev_bytes, cur_bytes;                /* capacities of d_prev / d_cur */
} fo_occlusion_memory_t;
int fo_scene_set_occlusion_memory(fo_ctx *ctx, const fo_occlusion_memory_t *om);

/* EXTENSION: the occlusion memory under the road metric (DESIGN.md §5.9 "Road metric").  The same structure, checks and
 * refusals as fo_scene_set_occlusion_memory, and it too arms the NEXT visibility stage only; NULL disarms; of the two arming
 * calls the later one decides.  Integers only.  With P the P of the call above:
 *  Pass(q) = P(q) or road(q), road = the world raster's road bit, 0 off the raster.
 *  d(g) = min over 8-connected cell paths q0 .. qn = g with P(q0) = 1 and Pass(qi) for every i >= 1 (g included) of 12 per
 *   axis step and 17 per diagonal step (a diagonal step asks for its two end cells only); d = 0 where P = 1.
 *  L = isqrt(169 r2) (<= 416); a path of cost <= L has at most n = L / 12 <= 34 steps, so only cells within n cells of g matter.
 *  An occluded cell g keeps H(g) = 1 iff P(g + d) = 1 for some dx^2 + dy^2 <= r2 (the disc test above) AND d(g) <= L; visible
 *   cells give 0, cells that are neither the road bit, as above.  Cell by cell H_road <= H_euclid, with equality where every cell
 *   within n of g is passable.
 * reset != 0: the stage is bit-identical to one armed by fo_scene_set_occlusion_memory with reset != 0 (and launches that
 * call's kernel).  Otherwise one launch of fo_occlusion_memory_road_kernel in place of the disc kernel. */
int fo_scene_set_occlusion_memory_road(fo_ctx *ctx, const fo_occlusion_memory_t *om);

/* EXTENSION: the vehicle layer of the occlusion memory (DESIGN.md §5.9 "Vehicle layer"): a second hidden set V kept next to H,
 * for vehicles that obey the driving direction of the lanes.  It masks nothing: class bytes, occluded list and H of the stage
 * are those of the stage without it.  The same structure; d_prev / d_cur are V of the previous / of this step, the window
 * fields as above.  Valid only AFTER one of the two calls above has armed the main memory of the same stage; a later one of
 * those calls drops it; it too arms the NEXT visibility stage only, NULL disarms, a failed stage disarms.  Integers only.
 *  PV = V of the previous step inside its window, the road raster outside it, 0 off the raster; PassV(q) = PV(q) or road(q).
 *  A step q -> g = q + dir_j (j * 45 degrees) is allowed iff PassV(g), bit j of out(q) AND bit j of out(g); out = the map's move
 *   byte (fo_scene_set_lane_moves), 0xFF off the raster.  d_flow(g) = the cheapest path from a cell of PV over allowed steps, 12
 *   per axis step, 17 per diagonal one, 0 on PV.
 *  An occluded cell keeps V(g) = 1 iff PV(g + d) = 1 for some dx^2 + dy^2 <= r2 AND d_flow(g) <= isqrt(169 r2); visible cells
 *   give 0, cells that are neither the road bit.  reset != 0: V = H of a reset step.  Cell by cell V <= H (the stage reads H of
 *   this step and writes V = 0 wherever H = 0).
 * One launch of fo_occlusion_memory_flow_kernel behind the main memory's.
 * FO_E_STATE: no map, no armed main memory, no move table.  FO_E_ARG: no context, r2 outside [0, FO_OCCLUSION_MEMORY_MAX_HALO^2]
 * or above the main memory's r2, reset different from the main memory's, buffers as above (d_cur must not be the main d_cur);
 * the visibility stage returns FO_E_ARG when cur_bytes < win_nx * win_ny. */
int fo_scene_set_occlusion_memory_vehicles(fo_ctx *ctx, const fo_occlusion_memory_t *vm);

/* EXTENSION, not part of the reference: how much of the currently occluded area each candidate trajectory
 * will come to see.  d_x / d_y [M][T] as for fo_sweep_run; pose (m, k) = sample k * t_stride, K = ceil(T / t_stride).
 * From every pose a full fan of n_rays (<= 768: the 720-ray fan of the visibility stage fits) rays of length r along d_dirs [n_rays][2] (world-aligned, counter-
 * clockwise, e.g. fo_scene_fan with yaw 0) is cast against the static map and the obstacles where they stand now
 * (d_ocorn / d_oflags as for fo_scene_visibility).  d_revealed [M][K] = number of cells of the current occluded set
 * (d_occ_idx / d_n_occ and the window of the fo_scene_visibility call that produced them) whose centre lies within r
 * of the pose and on its side of the chord between the hit points of the two rays enclosing it; d_area [M][K] = area
 * of the polygon of hit points. */
int fo_scene_future_visibility(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, int t_stride, int n_rays,
                               const double *d_dirs, double r, int O, const double *d_ocorn, const uint8_t *d_oflags,
                               const int32_t *d_occ_idx, const int32_t *d_n_occ, int win_ix0, int win_iy0, int win_nx,
                               int32_t *d_revealed, double *d_area, void *stream);

/* EXTENSION, not part of the reference: the extended form of fo_scene_future_visibility (same meaning where the names are
 * the same; with n_slices = 1, fov_deg >= 359.9, d_heading = NULL and no first-seen outputs it computes the same bits).
 * Occluder slices: d_ocorn [n_slices][O][4][2], d_oflags [n_slices][O]; pose k reads slice min(k, n_slices - 1), so
 * obstacles move, appear (bit 0 set) or leave (cleared) along the trajectory.  Field of view: fov_deg >= 359.9 is a full
 * circle; below, d_dirs is the open fan about heading 0 (fo_scene_fan with yaw 0 and this fov_deg: rays from -fov/2 to
 * +fov/2 inclusive) -- the polygon is pose + hit points (open shoelace sum) and a cell outside the sector is not revealed.
 * d_heading [M][K][2] (unit (cos, sin) per pose, or NULL = world-aligned; required below 359.9): ray i of pose (m, k) is
 * (c ux - s uy, s ux + c uy) in float64 without contraction.  First-seen outputs (either may be NULL):
 * d_revealed_new [M][K] = cells of the occluded set inside pose k's fan and inside no earlier pose's fan of trajectory m,
 * d_revealed_any [M] = its row sum; exact integers (a workgroup per trajectory walks its poses in order with a seen set
 * in LDS), which needs win_nx * win_ny <= FO_FUTURE_VISIBILITY_MAX_CELLS.  FO_E_ARG: n_slices < 1, n_rays outside
 * [4, 768], a sector without d_heading, a window above the capacity with first-seen outputs, a missing buffer. */
#define FO_FUTURE_VISIBILITY_MAX_CELLS 114688
typedef struct {
  int32_t M, T, t_stride, n_rays;
  const double *d_x, *d_y;                /* [M][T] */
  const double *d_dirs;                   /* [n_rays][2] unit fan about heading 0 */
  double r, fov_deg;
  const double *d_heading;                /* [M][K][2] or NULL */
  int32_t O, n_slices;
  const double *d_ocorn;                  /* [n_slices][O][4][2] */
  const uint8_t *d_oflags;                /* [n_slices][O] */
  const int32_t *d_occ_idx, *d_n_occ;     /* the occluded set of a fo_scene_visibility call ... */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* ... and its window */
  int32_t *d_revealed;                    /* [M][K] */
  double *d_area;                         /* [M][K] */
  int32_t *d_revealed_new;                /* [M][K] or NULL */
  int32_t *d_revealed_any;                /* [M] or NULL */
} fo_future_visibility_t;
int fo_scene_future_visibility_ex(fo_ctx *ctx, const fo_future_visibility_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic reach forecast -- where road users the ego cannot see
 * may be at each sample of the planning horizon, and which candidate trajectories sweep through such road.  Called after a
 * visibility stage (d_cls + window: that call's cell classes), on the caller's stream; nothing of it runs unless it is called.
 * All of it is integer arithmetic on cell indices except one point-in-rectangle test, so every output is an exact integer.
 *  Sources S(q), q a world-raster cell: inside the window d_hidden_or_null [ny][nx] (the H the occlusion memory wrote this
 *   step, fo_occlusion_memory_t::d_cur) or, when NULL, !(c & 2) && (c & 5) != 0 (what H is after a reset); outside the window
 *   on the raster the road bit; off the raster 0.
 *  Reach table h_r2 [J] (HOST memory, read before the call returns): R2[j] = floor((v_max j dt + margin)^2 / cs^2), the r2
 *   of fo_occlusion_memory_t for a step of j dt; non-decreasing, R2[0] >= 0.
 *  D2(g) = min over q with S(q) = 1 of (gx - qx)^2 + (gy - qy)^2, searched over the window grown by h = isqrt(R2[J-1]) cells
 *   on every side (nothing farther matters).  Euclidean, also across cells that are not road: an over-approximation;
 *   fo_scene_hidden_reach_road below bounds it by the distance along the road.
 *  d_arrival [ny][nx] uint8: A(g) = min { j : D2(g) <= R2[j] } for a road cell (c & 1), 255 = not within the horizon or not
 *   road.  A cell outside the window counts as A = 0 if it is on the raster and road, else 255.
 *  Footprint of trajectory m at sample k (time k dt): the sweep's ego rectangle -- centre (x + wb c, y + wb s), half extents
 *   hl, hw, (c, s) = d_heading [M][T][2], the UNIT heading per sample (the device takes no sine or cosine).  World-raster
 *   cell g with centre p = (x0 + (gx + 0.5) cs, y0 + (gy + 0.5) cs) is inside iff |u| <= hl and |w| <= hw with
 *   ex = px - cx, ey = py - cy, u = ex c + ey s, w = ey c - ex s (float64, this order, no contraction).
 *  d_cells [M][T] int32: footprint cells with A(g) <= k.  d_first [M] int32: smallest k with cells > 0, -1 = none.
 *  d_slack [M] int32: min over k and footprint cells with A(g) != 255 of A(g) - k, INT32_MAX = no such cell (slack <= 0 iff
 *   first >= 0).  d_len_or_null [M] int32: samples k >= len[m] contribute nothing and get cells = 0.
 * With M = 0 only the map is computed.  Two launches for the map (rows, columns), one for the trajectories.
 * FO_E_ARG (nothing is launched): J outside [1, 254]; T outside [1, J] with M > 0; h_r2 decreasing or negative;
 * isqrt(h_r2[J-1]) > FO_HIDDEN_REACH_MAX_HALO (never a silently shortened reach); no h_r2, d_cls or d_arrival; with M > 0 no
 * d_x / d_y / d_heading / d_cells / d_first / d_slack, or hl, hw or |wb| negative, NaN or above
 * FO_HIDDEN_REACH_MAX_HALF_EXTENT cell sizes (a pose scans its rectangle's bounding box: the bound keeps that scan short; no
 * road vehicle comes near it); a window outside [1, 32768]^2.  A heading that is not a unit vector is not detected: the
 * scanned box is that of the unit rectangle, the result then is not the definition's.
 * One call at a time per context: the row distances between the two map launches live in a workspace of the context (grown,
 * i.e. freed and allocated, when a call needs more), so calls on different streams must not overlap -- the rule of every
 * per-step workspace of the scene stage.
 * FO_HIDDEN_REACH_MAX_HALO: the distance along a row is kept in a byte, h + 1 standing for "none within h", next to the
 * arrival byte's 255 -- so h <= 254; the column pass then stages (16 + 2 h) x 64 bytes of LDS per workgroup (33 KB at 254). */
#define FO_HIDDEN_REACH_MAX_HALO 254
#define FO_HIDDEN_REACH_MAX_HALF_EXTENT 64
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* half length, half width (inflated by the caller), rear axle -> centre */
  int32_t J;
  const int32_t *h_r2;                      /* HOST [J] */
  const uint8_t *d_cls;                     /* [win_ny][win_nx] */
  const uint8_t *d_hidden_or_null;          /* [win_ny][win_nx] */
  int32_t win_ix0, win_iy0, win_nx, win_ny;
  uint8_t *d_arrival;                       /* [win_ny][win_nx] */
  int32_t *d_cells;                         /* [M][T] */
  int32_t *d_first, *d_slack;               /* [M] */
} fo_hidden_reach_t;
int fo_scene_hidden_reach(fo_ctx *ctx, const fo_hidden_reach_t *p, void *stream);

/* EXTENSION, not part of the reference: the same forecast with the ROAD metric (DESIGN.md §5.10 "Road metric") -- hidden traffic
 * arrives along passable cells, not through a building block.  Everything of fo_scene_hidden_reach holds (arguments, outputs,
 * limits, one call at a time per context); only the arrival map differs.  Integers only:
 *  Passable P(q) = S(q) or road(q); road(q) = c & 1 inside the window, and outside it P = S (the raster's road bit, every
 *   unobserved road cell being a source; off the raster 0).
 *  d(g) = min over 8-connected cell paths q0 .. qn = g with S(q0) = 1 and every qi passable of the sum of step weights, 12 for
 *   an axis step and 17 for a diagonal one (a diagonal step needs only its two end cells passable: the forecast must not
 *   under-reach); d = 0 on sources.  12 dx + 5 dy <= 13 sqrt(dx^2 + dy^2): d / 13 never exceeds the Euclidean length of the
 *   lattice path.
 *  L[j] = isqrt(169 R2[j]), the reach in these units.  Distances beyond L[J-1] are not propagated.
 *  A_geo(g) = min { j : d(g) <= L[j] } on road cells, 255 otherwise; d_arrival = max(A_geo, A of fo_scene_hidden_reach), 255
 *   counting as later than every step: both over-approximate the same truth, the later arrival still does, and on open road
 *   the two maps are equal.  d_cells, d_first, d_slack are computed from this map.
 *  d_dist_or_null [win_ny][win_nx] uint16: d, 65535 = impassable or beyond L[J-1].  NULL: the distances stay in a workspace of
 *   the context.
 * Launches: the two of the Euclidean map, ceil(L[J-1] / 192) distance bands (at least one; at most 18), one merge, one for the
 * trajectories with M > 0.  No launch waits for another workgroup, nothing is read back.  Refusals as fo_scene_hidden_reach,
 * messages prefixed "fo_scene_hidden_reach_road:". */
typedef struct {
  fo_hidden_reach_t base;
  uint16_t *d_dist_or_null;                 /* [win_ny][win_nx] d, 65535 = none */
} fo_hidden_reach_road_t;
int fo_scene_hidden_reach_road(fo_ctx *ctx, const fo_hidden_reach_road_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic CLEARANCE (DESIGN.md §5.10 "Clearance and critical speed") -- one key
 * map and one minimum per pose that answer the forecast above for EVERY hidden-user speed up to a cap, and the slowest hidden
 * road user that could meet a trajectory at all.  Called like fo_scene_hidden_reach, whose window, class bytes, hidden mask,
 * raster, sources S(q), passable set, road distance d (12 / 17 per step, permissive diagonals), footprint (headings handed
 * over as data), d_len_or_null and rule for cells outside the window it takes unchanged.  Integers only, apart from the
 * footprint test.  NONE = FO_HIDDEN_CLEARANCE_NONE = INT32_MAX.
 *  r2_cap >= 0, squared cells: h = isqrt(r2_cap) <= FO_HIDDEN_REACH_MAX_HALO, Lcap = isqrt(169 r2_cap).  The call serves every
 *   reach table with R2[J-1] <= r2_cap.
 *  d_key [ny][nx] int32: D2(g) is searched over the window grown by h and is exact whenever D2 <= r2_cap.  A cell that is not
 *   road (!(c & 1)) or has D2 > r2_cap gets NONE.  metric FO_HIDDEN_CLEARANCE_EUCLID: key = 169 D2(g).
 *   FO_HIDDEN_CLEARANCE_ROAD: key = max(169 D2(g), d(g)^2), NONE when d(g) > Lcap or g cannot be reached over passable cells.
 *   A cell outside the window counts as key = 0 if it is on the raster and road, else NONE.
 *   (169 * 2 * 254^2 and (13 * 254 + 12)^2 are below 2^31.)
 *  d_qmin [M][T] int32: min of key over the footprint cells of pose (m, k); NONE if the footprint holds no road cell within the
 *   cap, and for k >= len[m].
 *  The tie: for either metric and every non-decreasing table with R2[J-1] <= r2_cap, A(g) <= j iff key(g) <= 169 R2[j]
 *   (d <= isqrt(x) iff d^2 <= x), so with j(q) = min { j : q <= 169 R2[j] }, 255 = none:
 *   d_cells[m][k] > 0 iff qmin[m][k] <= 169 R2[k];  d_first[m] = min { k : qmin[m][k] <= 169 R2[k] }, -1 = none;
 *   d_slack[m] = min over k with j(qmin[m][k]) != 255 of j(qmin[m][k]) - k, INT32_MAX = none.
 *   The COUNT d_cells[m][k] is not derivable from qmin.
 *  d_dist_or_null [ny][nx] uint16 (road only): d, 65535 = impassable or beyond Lcap.  NULL: the distances stay in a workspace
 *   of the context.
 * With M = 0 only the map is computed.  Launches: rows and columns of the distance transform; road: ceil(Lcap / 192) distance
 * bands (at least one, at most 18) and one merge; one for the poses with M > 0.  No atomics, no launch waits for another
 * workgroup, nothing is read back.  One call at a time per context (the workspaces of fo_scene_hidden_reach).
 * FO_E_ARG (nothing is launched, messages prefixed "fo_scene_hidden_clearance:"): r2_cap negative or isqrt(r2_cap) >
 * FO_HIDDEN_REACH_MAX_HALO; an unknown metric; no d_cls or d_key; M < 0; with M > 0: T < 1, no d_x / d_y / d_heading / d_qmin, or
 * hl, hw or |wb| negative, NaN or above FO_HIDDEN_REACH_MAX_HALF_EXTENT cell sizes; a window outside [1, 32768]^2. */
#define FO_HIDDEN_CLEARANCE_NONE 2147483647
#define FO_HIDDEN_CLEARANCE_EUCLID 0
#define FO_HIDDEN_CLEARANCE_ROAD 1
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* half length, half width (inflated by the caller), rear axle -> centre */
  int32_t r2_cap, metric;
  const uint8_t *d_cls;                     /* [win_ny][win_nx] */
  const uint8_t *d_hidden_or_null;          /* [win_ny][win_nx] */
  int32_t win_ix0, win_iy0, win_nx, win_ny;
  int32_t *d_key;                           /* [win_ny][win_nx] */
  int32_t *d_qmin;                          /* [M][T] */
  uint16_t *d_dist_or_null;                 /* [win_ny][win_nx] d, 65535 = none (road only) */
} fo_hidden_clearance_t;
int fo_scene_hidden_clearance(fo_ctx *ctx, const fo_hidden_clearance_t *p, void *stream);

/* EXTENSION, not part of the reference: the road metric bound to the DRIVING DIRECTION of the lanes (DESIGN.md §5.10 "Lane
 * flow") -- a hidden vehicle that obeys the lanes does not come back down the ego's own lane, against a one-way street or out of
 * the lane that leads away from a junction.  Opt-in and additive: pedestrians are not bound to lanes and keep the two entries
 * above.  Integers only; the device computes no angle.
 *  Directions k = 0 .. 7 are the lattice steps E (1,0), NE (1,1), N (0,1), NW (-1,1), W (-1,0), SW (-1,-1), S (0,-1), SE (1,-1):
 *   step k points at k * 45 degrees.
 *  Move byte out(q), one uint8 per cell of the world raster: bit k is set when a lane-abiding vehicle in q may take step k.
 *   0xFF (every step) for a cell off the raster and, by the table's builder, for a cell whose centre lies in no lanelet: the
 *   occlusion memory's hidden cells beside the road stay free.  A cell inside several lanelets carries the union of their sets.
 *   The table is static map data, built on the host once per map.
 *  A step q -> g = q + dir_k is allowed iff g is passable (the road metric's set, unchanged), bit k is set in out(q) AND bit k is
 *   set in out(g): both ends decide -- a step only its origin allows would let oncoming traffic swerve into every cell of the
 *   ego's lane.  Neighbour lanes of one direction share directions (lane changes stay possible), opposite lanes share none.
 *  d_flow(g) = the cheapest path from a source over allowed steps, 12 per axis step and 17 per diagonal one, 0 on sources;
 *   nothing is propagated beyond L[J-1]; 65535 = none.  Sources, window, hidden mask, the rule outside the window, L[j], A_geo,
 *   d_arrival = max(A_geo, A_euclid), d_cells, d_first and d_slack are exactly those of fo_scene_hidden_reach_road with d_flow in
 *   the place of d.  d_flow >= d (65535 the largest), hence A_flow >= A_road >= A_euclid; with a table of 0xFF everywhere
 *   d_flow == d and every output equals that entry's bit for bit.
 *  Not claimed: wrong-way drivers, U-turns and reversing vehicles are outside the model ("no driving against the lane").  The
 *   occlusion memory is not given this metric: its hidden set is a superset of what a flow memory would keep, so it stays a
 *   conservative source set.
 *
 * fo_scene_set_lane_moves: h_moves [rny][rnx] of the map's raster (fo_scene_map_info), one-off after fo_scene_set_map; the table
 *  belongs to the map (a new fo_scene_set_map drops it) and is shared with it: upload it through the owner before
 *  fo_scene_share_map, FO_E_STATE while the map has more than one reader.  NULL drops the table.
 * fo_scene_hidden_reach_flow: the structure, outputs and refusals of fo_scene_hidden_reach_road (messages prefixed
 *  "fo_scene_hidden_reach_flow:"), d_dist_or_null receives d_flow; FO_E_STATE, nothing launched, when the map has no move table.
 *  Launches: the two of the Euclidean map, ceil(L[J-1] / 192) flow bands (at least one), the road entry's merge, one for the
 *  trajectories with M > 0.
 * fo_scene_hidden_clearance_flow: fo_scene_hidden_clearance with metric == FO_HIDDEN_CLEARANCE_ROAD (anything else: FO_E_ARG)
 *  and key = max(169 D2, d_flow^2); the tie holds with fo_scene_hidden_reach_flow in the place of the road entry.  FO_E_STATE
 *  without a move table. */
int fo_scene_set_lane_moves(fo_ctx *ctx, const uint8_t *h_moves /* [rny][rnx] */);
int fo_scene_hidden_reach_flow(fo_ctx *ctx, const fo_hidden_reach_road_t *p, void *stream);
int fo_scene_hidden_clearance_flow(fo_ctx *ctx, const fo_hidden_clearance_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic WITNESSES (DESIGN.md §5.10 "Witnesses") -- per candidate trajectory the
 * cell where hidden traffic first meets it, the hidden cell that traffic starts from and the cheapest route between them: what a
 * caller needs to put that road user in front of the metric sweep as a phantom agent.  Opt-in and additive: one launch, nothing
 * is read back, no other output changes.  Integers only, apart from the footprint test.
 *  Inputs: the outputs of ONE fo_scene_hidden_reach_road (flow = 0) or fo_scene_hidden_reach_flow (flow = 1) call of this step --
 *   A = base.d_arrival, d = d_dist (that call's d_dist_or_null), base.d_first [M] -- with the same trajectories, headings, hl, hw,
 *   wb, J, h_r2 and window.  base.d_cls, d_hidden_or_null, d_len_or_null, d_cells and d_slack are not read.
 *  Extension to every world-raster cell g: inside the window A(g), d(g) are the maps'; outside it a cell on the raster and road
 *   has A = 0, d = 0 (every unobserved road cell is a source), every other cell A = 255, d = 65535.  out(g) is the move table's
 *   byte on the raster (flow = 1) and 0xFF off it and with flow = 0.  Directions k = 0 .. 7, dir_k and the weights w_k = 12 / 17
 *   are those of the lane flow above.
 *  1. Conflict cell.  k* = first[m]; k* = -1 (or no sample of the batch): no witness -- steps = -1, wdist = -1, cell = src =
 *   (INT32_MIN, INT32_MIN), the row of dirs all 255.  Otherwise g* is, among the footprint cells of sample k* (the footprint and
 *   the clipping of fo_scene_hidden_reach, cells outside the window included) with A(g) <= k*, the one with the smallest
 *   (d(g), gy, gx), compared lexicographically.  (No such cell -- a first that is not these maps': steps = -2, the rest as without
 *   a witness.)
 *  2. Walk.  c_0 = g*, prev = none.  While d(c_i) > 0: K_i = { k : p = c_i - dir_k, d(p) != 65535, d(p) + w_k == d(c_i), bit k
 *   set in out(p) and in out(c_i) }; k_i = prev if prev is in K_i, else min K_i; prev = k_i; c_{i+1} = c_i - dir_{k_i};
 *   dirs[i] = k_i.  steps = n at the first c_n with d = 0, src = c_n.  On maps made by the two entries K_i is never empty (d is a
 *   shortest-path distance) and n <= isqrt(169 h_r2[J-1]) / 12.  If K_i is empty or i reaches path_cap the maps are not this
 *   definition's: steps = -2, src = c_i, the rest of the row 255 -- the walk is bounded whatever d holds, and reads only cells
 *   of the maps and of the raster.
 *  3. Outputs, every byte written by every call: d_cell [M][2] int32 the world-raster indices (gx, gy) of g*; d_src [M][2] those
 *   of the source; d_steps [M]; d_wdist [M] = d(g*); d_dirs [M][path_cap] uint8 in walk order (from g* back), 255 beyond steps.
 *   The hidden road user travels src -> g* by dir_{k_{n-1}}, .., dir_{k_0}; the step weights sum to wdist; every step is an
 *   allowed step of the metric that made d, and src is a source.
 *  Not claimed: the witness is the road user that is first by road distance, not the most harmful one.
 * path_cap: a multiple of 4 (a row is stored as dwords; d_dirs aligned to 4 bytes) with path_cap >= isqrt(169 h_r2[J-1]) / 12,
 *  at most FO_HIDDEN_WITNESS_MAX_STEPS at the halo cap.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, messages prefixed "fo_scene_hidden_witness:"): flow not 0 or
 * 1; J outside [1, 254]; no h_r2, base.d_arrival or d_dist; a window outside [1, 32768]^2; h_r2 refused as by
 * fo_scene_hidden_reach; M < 0; path_cap negative, too small or no multiple of 4; with M > 0: T outside [1, J], no d_x / d_y /
 * d_heading / d_first, no output buffer, or extents refused as by fo_scene_hidden_reach.  FO_E_STATE: flow = 1 without a move table. */
#define FO_HIDDEN_WITNESS_MAX_STEPS 276
typedef struct {
  fo_hidden_reach_t base;                   /* M, T, d_x, d_y, d_heading, hl, hw, wb, J, h_r2, window: those of the call that made
                                               the maps; d_arrival and d_first are INPUTS here */
  const uint16_t *d_dist;                   /* [win_ny][win_nx] the d_dist_or_null of that call (required) */
  int32_t flow;                             /* 0: road, 1: lanes */
  int32_t path_cap;
  int32_t *d_cell, *d_src;                  /* [M][2] */
  int32_t *d_steps, *d_wdist;               /* [M] */
  uint8_t *d_dirs;                          /* [M][path_cap] */
} fo_hidden_witness_t;
int fo_scene_hidden_witness(fo_ctx *ctx, const fo_hidden_witness_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic BRAKE CLEARANCE (DESIGN.md §5.10 "Brake clearance") -- if the ego follows
 * candidate m until sample b and then brakes, does it come to rest before it enters road that hidden traffic could have reached
 * by then?  commit[m] is the first b from which it does not: the fail-safe criterion that ranks the candidates where first >= 0
 * holds for the whole fan.  The manoeuvre is the reference's (metrics/be.py:84-146, _calc_deceleration_trajectory): the path is
 * kept, the speed ramps down, the poses are re-sampled by linear interpolation over the travelled chord length.  Opt-in and
 * additive: one launch, nothing is read back, no other output changes.  Integers everywhere except the pose arithmetic and the
 * footprint test; all float64 in the stated operation order, no contraction.
 *  Inputs: those of ONE forecast call of this step (fo_scene_hidden_reach, _road or _flow) -- trajectories, headings, d_len_or_null,
 *   hl, hw, wb, the window, J = T, h_r2 -- with its outputs A = base.d_arrival and first = base.d_first; d_v [M][T] the speed at
 *   each sample (m/s), d_arc [M][T] the travelled chord length, handed over as data like the headings (nothing depends on it
 *   being monotone); a_brake >= 0 (m/s^2), dt > 0.  base.d_cls, d_hidden_or_null, d_cells and d_slack are not read.
 *   Lm = T clipped by len[m], as in fo_scene_hidden_reach.
 *  For trajectory m and brake start b in 0 .. T-1:
 *  1. b >= Lm: brake_first[m][b] = -1 and stop[m][b] = -1.
 *  2. Speed profile, the speed held over a step: vn(i) = fmax(v[m][b] - a_brake * ((double)(i - b) * dt), 0.0) for i >= b.
 *   stop[m][b] = the smallest i in [b, Lm) with vn(i) == 0.0, or Lm if there is none.
 *  3. Poses.  Samples i <= b are the candidate's own (the forecast covers them).  For i = b+1 .. Lm-1, in this order:
 *   s = arc[b] once, then s = s + vn(i-1) * dt;  sc = fmin(s, arc[Lm-1]) (clamped to the end of the path, where the reference
 *   raises);  j = the first index in [0, Lm) with arc[j] >= sc, Lm if there is none;  idx = min(max(j, 1), Lm-1), xlo = arc[idx-1],
 *   xhi = arc[idx].  If xhi != xlo: w = sc - xlo, inv = xhi - xlo, xn = (x[idx] - x[idx-1]) / inv * w + x[idx-1], yn likewise;
 *   otherwise xn = x[idx-1], yn = y[idx-1].  Heading: the (c, s) of sample idx-1 if xhi == xlo or w + w <= inv, else that of
 *   sample idx (no new trigonometry).  These are be.py's interp1d semantics (searchsorted-left segment, clipped), anchored at
 *   arc[b] rather than at 0.
 *  4. Hit.  The footprint of (xn, yn, c, s) is that of fo_scene_hidden_reach, with its clipping and its rule outside the window
 *   (A = 0 on raster road, 255 elsewhere).  hit(i) iff some footprint cell has A <= i.  brake_first[m][b] = min { i : hit(i) }, -1 =
 *   none.
 *  5. commit[m] = the smallest b in [0, Lm) with 0 <= first[m] <= b (the candidate itself is already in reached road) or
 *   0 <= brake_first[m][b] < stop[m][b] (the braking ego meets reached road while it still moves), -1 = none.  A conflict at or
 *   after stop is a standing ego and does not count.
 *  Outputs, every byte written by every call: d_brake_first [M][T], d_stop [M][T], d_commit [M], int32.
 *  Safety of the data: the first-index rule is non-decreasing in sc and sc is non-decreasing in i, so a forward-only index is
 *   exact for any content of arc; idx is clamped before any read; NaN in v or arc goes wherever fmax / fmin / the comparisons
 *   send it and never reads out of range.
 *  Not claimed: the manoeuvre follows the candidate's own path only as far as that path goes (clamped at its end); manoeuvres
 *   still moving at the last sample (stop == Lm) are decided only within the horizon; the heading is that of the nearer sample,
 *   off by at most half a step's turn (the caller's inflation is the margin for it); the hidden road user is the forecast's
 *   (v_max, margin, metric and flow are baked into A).
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, messages prefixed "fo_scene_hidden_brake:"): J outside
 * [1, 254]; no h_r2 or base.d_arrival; a window outside [1, 32768]^2; h_r2 refused as by fo_scene_hidden_reach; M < 0; a_brake
 * negative or not finite; dt not positive and finite; with M > 0: T outside [1, J], no d_x / d_y / d_heading / d_first, no d_v or
 * d_arc, no output buffer, or extents refused as by fo_scene_hidden_reach. */
typedef struct {
  fo_hidden_reach_t base;                   /* M, T, d_x, d_y, d_heading, d_len_or_null, hl, hw, wb, J, h_r2, window: those of the call
                                               that made the map; d_arrival and d_first are INPUTS here */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  double a_brake, dt;
  int32_t *d_brake_first, *d_stop;          /* [M][T] */
  int32_t *d_commit;                        /* [M] */
} fo_hidden_brake_t;
int fo_scene_hidden_brake(fo_ctx *ctx, const fo_hidden_brake_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic BRAKE CLEARANCE BY CLASSES (DESIGN.md §5.10 "Brake clearance by classes")
 * -- the brake clearance above for up to FO_HIDDEN_BRAKE_MAX_CLASSES hidden road users of different speeds (a pedestrian, a
 * cyclist, a car) from ONE walk over the clearance's key map, in place of one forecast and one walk per speed.  Opt-in and
 * additive: one launch, nothing is read back, no other output changes.
 *  Inputs: those of ONE fo_scene_hidden_clearance or fo_scene_hidden_clearance_flow call of this step -- trajectories, headings,
 *   d_len_or_null, hl, hw, wb, the window and r2_cap -- with its outputs key = d_key [win_ny][win_nx] and qmin = d_qmin [M][T];
 *   d_v, d_arc [M][T], a_brake >= 0 and dt > 0 as in fo_scene_hidden_brake; C classes, 1 <= C <= FO_HIDDEN_BRAKE_MAX_CLASSES; the
 *   host table h_thr [C][T] int32, row c = 169 * R2_c[j] for the reach table R2_c of class c: every row non-decreasing with
 *   0 <= thr[c][j] and thr[c][T-1] <= 169 * r2_cap.  The table travels as a kernel argument (no transfer, no device buffer), hence
 *   C * T <= FO_HIDDEN_BRAKE_MAX_TABLE (3 584 bytes: with the other arguments under the 4 KB of a kernel's arguments) and
 *   T <= 254.  Lm = T clipped by len[m].
 *  For trajectory m, brake start b in 0 .. T-1 and class c:
 *  1. Steps 1 - 3 of fo_scene_hidden_brake word for word: stop[m][b], the speed profile vn, the re-sampled poses (xn, yn) and the
 *   heading rule.  None of them depends on the class.
 *  2. q(i) = the minimum of key over the footprint cells of the braking pose i, with the scan, the clipping and the rule outside
 *   the window of fo_scene_hidden_clearance (key 0 on raster road, FO_HIDDEN_CLEARANCE_NONE elsewhere); NONE for an empty footprint.
 *  3. hit_c(i) iff q(i) <= thr[c][i].
 *  4. brake_first[c][m][b] = min { i in (b, Lm) : hit_c(i) }, -1 = none (and for b >= Lm, where stop[m][b] = -1).
 *  5. first[c][m] = min { k < Lm : qmin[m][k] <= thr[c][k] }, -1 = none.
 *  6. commit[c][m] = the smallest b in [0, Lm) with 0 <= first[c][m] <= b or 0 <= brake_first[c][m][b] < stop[m][b], -1 = none.
 *  Outputs, every byte written by every call, int32: d_brake_first [C][M][T], d_stop [M][T], d_commit [C][M], d_first [C][M].
 *  The tie: for every class whose row is 169 times the reach table of some v_c, brake_first[c], stop, commit[c] and first[c] equal,
 *   bit for bit, what fo_scene_hidden_brake gives on the forecast of v_c with the same metric, flow, margin and hidden set.  Per
 *   cell A <= i iff key <= thr[c][i], outside the window too (0 <= every threshold < NONE); some cell qualifies iff the minimum
 *   does; after stop the pose is fixed and thr[c][.] does not decrease, so one scan answers the remaining samples of every class.
 *  Safety of the data: as fo_scene_hidden_brake; key, qmin and the table may hold anything the refusals let through, no index
 *   depends on them.
 *  Not claimed: what fo_scene_hidden_brake does not claim; a class speed above the clearance's cap is refused, not clipped.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, messages prefixed "fo_scene_hidden_brake_classes:"): C outside
 * [1, 8]; no h_thr; a window outside [1, 32768]^2; r2_cap negative or beyond FO_HIDDEN_REACH_MAX_HALO; M < 0; a_brake negative or
 * not finite; dt not positive and finite; with M > 0: T outside [1, 254]; C * T > FO_HIDDEN_BRAKE_MAX_TABLE; a row that is
 * negative, decreases or ends beyond 169 * r2_cap; no d_x / d_y / d_heading; no d_key or d_qmin; no d_v or d_arc; a missing output;
 * extents refused as by fo_scene_hidden_reach. */
#define FO_HIDDEN_BRAKE_MAX_CLASSES 8
#define FO_HIDDEN_BRAKE_MAX_TABLE 896
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* as handed to the clearance */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* the clearance's window */
  int32_t r2_cap;                           /* the clearance's cap: no row of h_thr ends beyond 169 * r2_cap */
  int32_t C;                                /* classes */
  const int32_t *d_key;                     /* [win_ny][win_nx] the clearance's key map (INPUT) */
  const int32_t *d_qmin;                    /* [M][T] the clearance's minimum per pose (INPUT) */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  double a_brake, dt;
  const int32_t *h_thr;                     /* HOST [C][T]: 169 * R2_c[j] */
  int32_t *d_brake_first;                   /* [C][M][T] */
  int32_t *d_stop;                          /* [M][T] */
  int32_t *d_commit, *d_first;              /* [C][M] */
} fo_hidden_brake_classes_t;
int fo_scene_hidden_brake_classes(fo_ctx *ctx, const fo_hidden_brake_classes_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic BRAKE CLEARANCE BY ROAD USERS (DESIGN.md §5.10 "Brake clearance by road
 * users") -- the brake clearance by classes for hidden road users that do not share a forecast: a pedestrian anywhere on the road, a
 * cyclist and a car along the lanes.  Every class names one of up to FO_HIDDEN_BRAKE_MAX_MAPS key maps; every manoeuvre is walked
 * ONCE and each braking pose's footprint is traversed once for all maps.  Opt-in and additive: one launch, nothing is read back, no
 * other output changes.
 *  Inputs: those of K clearance calls of this step over the same trajectories, headings, d_len_or_null, hl, hw, wb and window,
 *   1 <= K <= FO_HIDDEN_BRAKE_MAX_MAPS; per map k: d_key[k] [win_ny][win_nx], d_qmin[k] [M][T] and r2_cap[k], of
 *   fo_scene_hidden_clearance or fo_scene_hidden_clearance_flow, any metric; d_v, d_arc [M][T], a_brake >= 0 and dt > 0 as in
 *   fo_scene_hidden_brake_classes; C classes, 1 <= C <= FO_HIDDEN_BRAKE_MAX_CLASSES, C * T <= FO_HIDDEN_BRAKE_MAX_TABLE, T <= 254;
 *   map_of[c] in [0, K) per class; the host table h_thr [C][T] int32, every row non-decreasing with 0 <= thr[c][j] and
 *   thr[c][T-1] <= 169 * r2_cap[map_of[c]].  A map that no class names is allowed (it is not read); two maps
 *   may be the same buffer (the maps are only read, none of the outputs may overlap them).  Entries of d_key, d_qmin and
 *   r2_cap beyond K and of map_of beyond C are not looked at.  Lm = T clipped by len[m].
 *  For trajectory m, brake start b in 0 .. T-1 and class c with k = map_of[c]:
 *  1. Steps 1 - 3 of fo_scene_hidden_brake word for word: stop[m][b], the speed profile vn, the re-sampled poses (xn, yn) and the
 *   heading rule.  They depend on neither the class nor the map.
 *  2. q_k(i) = the minimum of key_k over the footprint cells of the braking pose i, with the scan, the clipping and the rule outside
 *   the window of fo_scene_hidden_clearance (key 0 on raster road, FO_HIDDEN_CLEARANCE_NONE elsewhere -- the same for every map); NONE
 *   for an empty footprint.
 *  3. hit_c(i) iff q_k(i) <= thr[c][i].
 *  4. brake_first[c][m][b] = min { i in (b, Lm) : hit_c(i) }, -1 = none (and for b >= Lm, where stop[m][b] = -1).
 *  5. first[c][m] = min { j < Lm : qmin_k[m][j] <= thr[c][j] }, -1 = none.
 *  6. commit[c][m] = the smallest b in [0, Lm) with 0 <= first[c][m] <= b or 0 <= brake_first[c][m][b] < stop[m][b], -1 = none.
 *  Outputs, every byte written by every call, int32: d_brake_first [C][M][T], d_stop [M][T], d_commit [C][M], d_first [C][M].
 *  The tie: row c of every output equals, bit for bit, what fo_scene_hidden_brake_classes gives on (key_k, qmin_k, r2_cap_k) with
 *   the single threshold row thr[c] -- and through that entry's tie fo_scene_hidden_brake on the forecast of that class's speed,
 *   metric and flow.  With K = 1 the whole result is fo_scene_hidden_brake_classes' on the same inputs.
 *  Safety of the data: as fo_scene_hidden_brake_classes; the keys, qmin, the table and map_of may hold anything the refusals let
 *   through, no index depends on them.
 *  Not claimed: what fo_scene_hidden_brake_classes does not claim; that the K maps belong to the same step, trajectories and window
 *   is the caller's word.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, messages prefixed "fo_scene_hidden_brake_users:"): K outside
 * [1, 3]; C outside [1, 8]; no h_thr; a window outside [1, 32768]^2; an r2_cap[k], k < K, negative or beyond
 * FO_HIDDEN_REACH_MAX_HALO; map_of[c], c < C, outside [0, K); M < 0; a_brake negative or not finite; dt not positive and finite; with
 * M > 0: T outside [1, 254]; C * T > FO_HIDDEN_BRAKE_MAX_TABLE; a row that is negative, decreases or ends beyond
 * 169 * r2_cap[map_of[c]]; no d_x / d_y / d_heading; no d_key[k] or d_qmin[k], k < K; no d_v or d_arc; a missing output; extents
 * refused as by fo_scene_hidden_reach.  FO_E_STATE: no scene. */
#define FO_HIDDEN_BRAKE_MAX_MAPS 3
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* as handed to the clearances */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* the clearances' window */
  int32_t K;                                /* maps */
  int32_t C;                                /* classes */
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];   /* [win_ny][win_nx] each: the clearances' key maps (INPUT) */
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];  /* [M][T] each: the clearances' minimum per pose (INPUT) */
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];         /* the clearances' caps */
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];      /* the map of class c, in [0, K) */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  double a_brake, dt;
  const int32_t *h_thr;                     /* HOST [C][T]: 169 * R2_c[j] */
  int32_t *d_brake_first;                   /* [C][M][T] */
  int32_t *d_stop;                          /* [M][T] */
  int32_t *d_commit, *d_first;              /* [C][M] */
} fo_hidden_brake_users_t;
int fo_scene_hidden_brake_users(fo_ctx *ctx, const fo_hidden_brake_users_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic BRAKE LADDER (DESIGN.md §5.10 "Brake ladder") -- the brake clearance above
 * at a ladder of K decelerations from ONE launch, and per candidate and brake start the first level of the ladder at which the
 * moving ego stays clear of road hidden traffic may have reached: a brake threat number against hidden traffic (the reference's
 * BE metric, metrics/be.py:31-82, asks it of phantom rectangles and searches by bisection; its manoeuvre routine takes a ladder,
 * be.py:106-107).  Harder braking is NOT always at least as safe against an arrival map -- a harder-braking ego may still crawl
 * through a cell when hidden traffic reaches it, which the gentler manoeuvre had left --, so every level is evaluated and
 * last_unclear says where a bisection's assumption fails.  Opt-in and additive: one launch, nothing is read back, no other
 * output changes.
 *  Inputs: those of fo_scene_hidden_brake -- one forecast call's trajectories, headings, d_len_or_null, extents, window, J = T, h_r2,
 *   A = base.d_arrival, first = base.d_first, d_v, d_arc, dt -- and in place of a_brake: h_levels [K], float64 on the HOST, read
 *   during the call as h_r2 is (they travel as a kernel argument), 1 <= K <= FO_HIDDEN_BRAKE_MAX_LEVELS, every level finite and
 *   >= 0, in any order, repeats allowed; B, the number of brake starts considered, b = 0 .. B-1, 1 <= B <= T.
 *  For trajectory m, brake start b < B and level k:
 *  1. Steps 1 - 4 of fo_scene_hidden_brake word for word with a_brake = levels[k]: brake_first[m][b][k] and stop[m][b][k], both -1
 *   where b >= Lm.
 *  2. unclear(m, b, k) iff 0 <= first[m] <= b or 0 <= brake_first[m][b][k] < stop[m][b][k].
 *  3. required[m][b] = the smallest k that is not unclear, -1 if every level is unclear.  last_unclear[m][b] = the largest k that
 *   is unclear, -1 if none is.  For b >= Lm both are -1: that pair cannot occur for a real manoeuvre, it marks "no manoeuvre".
 *  4. commit[m][k] = the smallest b < min(B, Lm) with unclear(m, b, k), -1 = none.
 *  Outputs, every byte written by every call, int32: d_brake_first [M][B][K], d_stop [M][B][K], d_required [M][B],
 *   d_last_unclear [M][B], d_commit [M][K] (K innermost: lanes dealt along the levels store next to each other).
 *  The tie: slice k of brake_first and stop equals, bit for bit, what fo_scene_hidden_brake gives with a_brake = levels[k] at the
 *   brake starts b < B; commit[.][k] is that entry's commit where it is < B, else -1.
 *  Safety of the data: as fo_scene_hidden_brake; the levels may hold anything the refusals let through, no index depends on them.
 *  Not claimed: what fo_scene_hidden_brake does not claim; the ladder's answer is only as fine as its levels; required is the
 *   first clear level BY INDEX, not a root of anything (with ascending levels it is the gentlest clear deceleration of the ladder).
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, messages prefixed "fo_scene_hidden_brake_ladder:"): J outside
 * [1, 254]; no h_r2 or base.d_arrival; a window outside [1, 32768]^2; h_r2 refused as by fo_scene_hidden_reach; M < 0; K outside
 * [1, 64]; no h_levels; a level negative or not finite; dt not positive and finite; with M > 0: T outside [1, J], B outside
 * [1, T], no d_x / d_y / d_heading / d_first, no d_v or d_arc, a missing output buffer, or extents refused as by
 * fo_scene_hidden_reach.  FO_E_STATE: no scene. */
#define FO_HIDDEN_BRAKE_MAX_LEVELS 64
typedef struct {
  fo_hidden_reach_t base;                   /* as in fo_hidden_brake_t: d_arrival and d_first are INPUTS here */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  const double *h_levels;                   /* HOST [K] decelerations, m/s^2 */
  int32_t K;                                /* levels */
  int32_t B;                                /* brake starts b = 0 .. B-1 */
  double dt;
  int32_t *d_brake_first, *d_stop;          /* [M][B][K] */
  int32_t *d_required, *d_last_unclear;     /* [M][B] */
  int32_t *d_commit;                        /* [M][K] */
} fo_hidden_brake_ladder_t;
int fo_scene_hidden_brake_ladder(fo_ctx *ctx, const fo_hidden_brake_ladder_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic BRAKE LADDER BY ROAD USERS (DESIGN.md §5.10 "Brake ladder by road users") --
 * the brake ladder above for hidden road users that do not share a forecast: per candidate and brake start the first level of a
 * ladder of L decelerations at which the moving ego stays clear of EVERY class of road user, each class held against the key map it
 * names, from ONE launch that walks every manoeuvre (m, b, level) once for all classes.  Harder braking is not always safer against
 * a map, so that level can lie above every single class's own: it is not a maximum over per-class ladders.  Opt-in and additive:
 * one launch, nothing is read back, no other output changes.
 *  Inputs: those of fo_scene_hidden_brake_users word for word -- K maps with d_key[k], d_qmin[k], r2_cap[k]; C classes, map_of[c],
 *   the host table h_thr [C][T]; trajectories, headings, d_len_or_null, extents and window; d_v, d_arc, dt -- and in place of
 *   a_brake: h_levels [L], float64 on the HOST, read during the call (they travel as a kernel argument, with the table),
 *   1 <= L <= FO_HIDDEN_BRAKE_MAX_LEVELS, every level finite and >= 0, in any order, repeats allowed; B, the number of brake starts
 *   considered, b = 0 .. B-1, 1 <= B <= T.  4 * C * T + 8 * L <= FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES.
 *  For trajectory m, brake start b < B, level l and class c with k = map_of[c]:
 *  1. Steps 1 - 5 of fo_scene_hidden_brake_users word for word with a_brake = levels[l]: stop[m][b][l] (the same for every class) and
 *   brake_first[c][m][b][l], both -1 where b >= Lm; first[c][m], which does not depend on the level.
 *  2. unclear(c, m, b, l) iff 0 <= first[c][m] <= b or 0 <= brake_first[c][m][b][l] < stop[m][b][l].
 *  3. Per class, for b < Lm: required[c][m][b] = the smallest l that is not unclear, -1 if every level is unclear;
 *   last_unclear[c][m][b] = the largest unclear l, -1 if none is; commit[c][m][l] = the smallest b < min(B, Lm) with
 *   unclear(c, m, b, l), -1 = none.
 *  4. Over the classes, for b < Lm: required_all[m][b] = the smallest l at which NO class is unclear, -1 if there is none;
 *   last_unclear_all[m][b] = the largest l at which some class is unclear, -1 if there is none; blocking[m][b] = a bit mask, bit c
 *   set iff class c is unclear at level required_all - 1 -- at level L - 1 where required_all = -1, and 0 where required_all = 0:
 *   the classes that keep the ego from the next gentler level.
 *  5. For b >= Lm required, last_unclear, required_all and last_unclear_all are -1 and blocking is 0: "no manoeuvre".
 *  Outputs, int32, every byte of every buffer handed over written by every call: d_required, d_last_unclear [C][M][B]; d_commit
 *   [C][M][L]; d_first [C][M]; d_required_all, d_last_unclear_all, d_blocking [M][B]; the detail d_brake_first_or_null
 *   [C][M][B][L] and d_stop_or_null [M][B][L]: both given or both null.
 *  The ties: slice l of brake_first and stop, and first, equal bit for bit what fo_scene_hidden_brake_users gives with
 *   a_brake = levels[l] at the brake starts b < B, commit[c][.][l] is that entry's commit where it is < B, else -1; row c of
 *   required, last_unclear and commit is what fo_scene_hidden_brake_ladder gives on the arrival map of class c's forecast.
 *  Safety of the data: as fo_scene_hidden_brake_users; the levels may hold anything the refusals let through, no index depends
 *   on them.
 *  Not claimed: what fo_scene_hidden_brake_users and fo_scene_hidden_brake_ladder do not claim; one ladder serves every class.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, no byte written, messages prefixed
 * "fo_scene_hidden_brake_ladder_users:"), in this order: K outside [1, 3]; C outside [1, 8]; no h_thr; a window outside
 * [1, 32768]^2; an r2_cap[k], k < K, negative or beyond FO_HIDDEN_REACH_MAX_HALO; map_of[c], c < C, outside [0, K); M < 0; L outside
 * [1, 64]; no h_levels; a level negative or not finite; dt not positive and finite; with M > 0: T outside [1, 254]; B outside
 * [1, T]; C * T > FO_HIDDEN_BRAKE_MAX_TABLE; 4 * C * T + 8 * L > FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES; a row that is negative,
 * decreases or ends beyond 169 * r2_cap[map_of[c]]; no d_x / d_y / d_heading; no d_key[k] or d_qmin[k], k < K; no d_v or d_arc; a
 * missing output; one detail buffer without the other; extents refused as by fo_scene_hidden_reach.  FO_E_STATE: no scene. */
#define FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES 3584
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* as handed to the clearances */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* the clearances' window */
  int32_t K;                                /* maps */
  int32_t C;                                /* classes */
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];   /* [win_ny][win_nx] each: the clearances' key maps (INPUT) */
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];  /* [M][T] each: the clearances' minimum per pose (INPUT) */
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];         /* the clearances' caps */
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];      /* the map of class c, in [0, K) */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  const double *h_levels;                   /* HOST [L] decelerations, m/s^2 */
  int32_t L;                                /* levels */
  int32_t B;                                /* brake starts b = 0 .. B-1 */
  double dt;
  const int32_t *h_thr;                     /* HOST [C][T]: 169 * R2_c[j] */
  int32_t *d_required, *d_last_unclear;     /* [C][M][B] */
  int32_t *d_commit;                        /* [C][M][L] */
  int32_t *d_first;                         /* [C][M] */
  int32_t *d_required_all, *d_last_unclear_all, *d_blocking;   /* [M][B] */
  int32_t *d_brake_first_or_null;           /* [C][M][B][L] the detail: both or neither */
  int32_t *d_stop_or_null;                  /* [M][B][L] */
} fo_hidden_brake_ladder_users_t;
int fo_scene_hidden_brake_ladder_users(fo_ctx *ctx, const fo_hidden_brake_ladder_users_t *p, void *stream);

/* EXTENSION, not part of the reference: DEVICE POSE PREPARATION of the hidden-traffic answers (DESIGN.md §5.10 "Fail-safe verdict")
 * -- what the brake entries above take as data, made on the device from candidates that live there: one launch, nothing is read
 * back.  Needs a context, no scene.
 *  Inputs: d_x, d_y, d_theta, d_v [M][T] float64, d_len_or_null [M]; Lm = T clipped by len[m].
 *  heading[m][k] = (cos, sin) of theta[m][k] from ONE sincos(theta, &s, &c) per sample: the bits the sweep's trajectory preparation
 *   rotates the ego rectangle by.  The forecast and the walks still take no trigonometry; a checker is handed this heading as data.
 *  arc[m][0] = 0, arc[m][k] = arc[m][k-1] + sqrt((x[k] - x[k-1])^2 + (y[k] - y[k-1])^2): be.py's
 *   insert(cumsum(sqrt(diff(x)^2 + diff(y)^2)), 0, 0) as a SEQUENTIAL float64 sum in index order, without contraction -- numpy's
 *   result on host arrays --, over all T samples whatever len says.
 *  finite[m] = 1 iff every x, y, theta, v of the samples k < Lm is finite (a non-finite value at k >= Lm does not count), else 0.
 *  Outputs, every byte written by every call: d_heading [M][T][2] float64, d_arc [M][T] float64, d_finite [M] uint8.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, messages prefixed "fo_scene_hidden_poses:"): no parameters;
 * M < 0; with M > 0: T outside [1, 254], a missing input or output.  FO_E_STATE: no context. */
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y, *d_theta, *d_v;  /* [M][T] */
  const int32_t *d_len_or_null;             /* [M] */
  double *d_heading;                        /* [M][T][2] unit (cos, sin) */
  double *d_arc;                            /* [M][T] travelled chord length, m */
  uint8_t *d_finite;                        /* [M] */
} fo_hidden_poses_t;
int fo_scene_hidden_poses(fo_ctx *ctx, const fo_hidden_poses_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic FAIL-SAFE VERDICT (DESIGN.md §5.10 "Fail-safe verdict") -- "is this candidate
 * still fail-safe against hidden traffic from every brake start up to the replanning interval?", folded into what a planner acts
 * on: the two reserved columns of the cost row and the safety flag that fo_step_run leaves in HBM.  The walk of
 * fo_scene_hidden_brake_users over the first B brake starts alone, without brake_first and stop.  Opt-in and additive: one launch on
 * the caller's stream, behind the step whose cost rows it folds into; nothing is read back.
 *  Inputs: those of fo_scene_hidden_brake_users word for word, and: B, the number of brake starts walked, 1 <= B <= T; commit_min,
 *   0 <= commit_min <= B; d_finite_or_null [M] uint8 (of fo_scene_hidden_poses; null: every candidate counts as finite);
 *   d_cost_or_null [M][FO_NC] and d_safe_or_null [M], the outputs of a sweep / step over the SAME M trajectories: both or neither.
 *  Write commit_users[c][m] and first_users[c][m] for what fo_scene_hidden_brake_users writes on the same inputs.
 *  1. commit[c][m] = commit_users[c][m] if 0 <= commit_users[c][m] < B, else -1; first[c][m] = first_users[c][m].
 *  2. fail_safe[m] = the smallest commit[c][m] >= 0 over the classes, B when there is none: the number of leading brake starts from
 *   which braking at a_brake keeps the moving ego clear of every user.  0 = "not even now", B = "throughout what was asked".
 *  3. user[m] = the lowest c with commit[c][m] == fail_safe[m], -1 when fail_safe[m] == B.
 *  4. finite[m] == 0: fail_safe[m] = 0 and user[m] = -2, whatever the walk found (a NaN pose fails every footprint comparison and
 *   would read as "no hit": this case fails CLOSED).
 *  5. With d_cost / d_safe: cost[m][FO_C_RES0] = (double)fail_safe[m], cost[m][FO_C_RES1] = (double)user[m]; if
 *   fail_safe[m] < commit_min: safe[m] = 0 and cost[m][FO_C_SAFE] = 0.0, otherwise both are left as found -- the stage only ever
 *   takes safety away; a row that a refused rule list or an unusable covariance poisoned keeps its NaNs and safe = 0 and gets the
 *   two columns.  No other column is touched.
 *  Outputs, int32, every byte written by every call: d_fail_safe [M], d_user [M], d_commit [C][M], d_first [C][M].
 *  Safety of the data: as fo_scene_hidden_brake_users; finite may hold anything, no index depends on it.
 *  Not claimed: what fo_scene_hidden_brake_users does not claim; brake starts b >= B are not looked at; that cost / safe belong to
 *   the same candidates is the caller's word.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, no byte written, messages prefixed
 * "fo_scene_hidden_brake_verdict:"), in this order: K outside [1, 3]; C outside [1, 8]; no h_thr; a window outside [1, 32768]^2; an
 * r2_cap[k], k < K, negative or beyond FO_HIDDEN_REACH_MAX_HALO; map_of[c], c < C, outside [0, K); M < 0; a_brake negative or not
 * finite; dt not positive and finite; with M > 0: T outside [1, 254]; B outside [1, T]; commit_min outside [0, B];
 * C * T > FO_HIDDEN_BRAKE_MAX_TABLE; a row that is negative, decreases or ends beyond 169 * r2_cap[map_of[c]]; no d_x / d_y /
 * d_heading; no d_key[k] or d_qmin[k], k < K; no d_v or d_arc; a missing output; only one of d_cost_or_null / d_safe_or_null;
 * extents refused as by fo_scene_hidden_reach.  FO_E_STATE: no scene. */
#define FO_HIDDEN_VERDICT_NOT_FINITE (-2)
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* as handed to the clearances */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* the clearances' window */
  int32_t K;                                /* maps */
  int32_t C;                                /* classes */
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];   /* [win_ny][win_nx] each: the clearances' key maps (INPUT) */
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];  /* [M][T] each: the clearances' minimum per pose (INPUT) */
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];         /* the clearances' caps */
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];      /* the map of class c, in [0, K) */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  double a_brake, dt;
  const int32_t *h_thr;                     /* HOST [C][T]: 169 * R2_c[j] */
  int32_t B;                                /* brake starts b = 0 .. B-1 */
  int32_t commit_min;                       /* fail_safe below it takes safety away */
  const uint8_t *d_finite_or_null;          /* [M] */
  double *d_cost_or_null;                   /* [M][FO_NC] of the step: both or neither */
  uint8_t *d_safe_or_null;                  /* [M] */
  int32_t *d_fail_safe, *d_user;            /* [M] */
  int32_t *d_commit, *d_first;              /* [C][M] */
} fo_hidden_brake_verdict_t;
int fo_scene_hidden_brake_verdict(fo_ctx *ctx, const fo_hidden_brake_verdict_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic LADDER VERDICT (DESIGN.md §5.10 "Ladder verdict") -- "how hard would the ego
 * have to brake, from the worst of the brake starts it executes before it replans, to stay clear of every hidden road user?", as a
 * graded term in what a planner acts on: the two reserved columns of the cost row and the safety flag that fo_step_run leaves in
 * HBM.  The walk of fo_scene_hidden_brake_ladder_users over the first B brake starts, reduced over them on the device: no [M][B]
 * or [M][B][L] buffer exists here.  Opt-in and additive: one launch on the caller's stream, behind the step whose cost rows it folds
 * into; nothing is read back.  It writes the SAME two reserved columns as fo_scene_hidden_brake_verdict: a step runs one stage or
 * the other, never both.
 *  Inputs: those of fo_scene_hidden_brake_ladder_users word for word -- K maps with d_key[k], d_qmin[k], r2_cap[k]; C classes,
 *   map_of[c], h_thr [C][T]; trajectories, d_heading, d_len_or_null, extents and window; d_v, d_arc, dt; h_levels [L]; B -- with the
 *   levels STRICTLY ASCENDING (the answer is a maximum over brake starts and means "the gentlest sufficient deceleration"), and:
 *   a_limit, float64, >= 0, +inf allowed, not NaN; d_finite_or_null [M] uint8 (of fo_scene_hidden_poses; null: every candidate counts
 *   as finite); d_cost_or_null [M][FO_NC] and d_safe_or_null [M], the outputs of a sweep / step over the SAME M trajectories: both or
 *   neither.
 *  Write ra[m][b], blk[m][b], req[c][m][b] and first[c][m] for what fo_scene_hidden_brake_ladder_users writes as required_all,
 *   blocking, required and first on the same inputs, and ends = min(B, Lm).
 *  1. rank(m, b) = ra[m][b] if ra[m][b] >= 0, else L ("no level of this ladder"); need[m] = the maximum of rank(m, b) over b < ends,
 *   -1 when ends = 0 ("nothing asked").
 *  2. at[m] = the smallest b < ends with rank(m, b) == need[m], -1 when need[m] = -1.
 *  3. blocking[m] = blk[m][at[m]], 0 when at[m] = -1; user[m] = the lowest set bit of blocking[m], -1 if none.
 *  4. Per class need_of[c][m] = the same maximum over b < ends formed from req[c][m][b] (-1 -> L), -1 when ends = 0; first[c][m] is
 *   the ladder-users entry's.
 *  5. decel[m] (float64) = levels[need[m]] for 0 <= need[m] < L, +inf for need[m] == L, 0.0 for need[m] == -1.
 *  6. finite[m] == 0: need[m] = L, at[m] = 0, blocking[m] = 0, user[m] = FO_HIDDEN_VERDICT_NOT_FINITE and decel[m] = +inf, whatever
 *   the walk found (a NaN pose fails every footprint comparison and would read as "no hit": this case fails CLOSED); need_of and first
 *   stay the walk's.
 *  7. With d_cost / d_safe: cost[m][FO_C_RES0] = decel[m], cost[m][FO_C_RES1] = (double)user[m]; if need[m] == L or
 *   decel[m] > a_limit: safe[m] = 0 and cost[m][FO_C_SAFE] = 0.0, otherwise both are left as found -- the stage only ever takes
 *   safety away; with a_limit = +inf only "no level" and non-finite candidates lose it; a row that a refused rule list or an
 *   unusable covariance poisoned keeps its NaNs and safe = 0 and gets the two columns.  No other column is touched.
 *  Outputs, every byte written by every call: d_need, d_at, d_blocking, d_user [M] int32; d_decel [M] float64; d_need_of, d_first
 *   [C][M] int32.
 *  Safety of the data: as fo_scene_hidden_brake_ladder_users; finite may hold anything, no index depends on it.
 *  Not claimed: what fo_scene_hidden_brake_ladder_users does not claim; brake starts b >= B are not looked at; the answer is only as
 *   fine as the ladder; that cost / safe belong to the same candidates is the caller's word.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, no byte written, messages prefixed
 * "fo_scene_hidden_brake_ladder_verdict:"), in this order: K outside [1, 3]; C outside [1, 8]; no h_thr; a window outside
 * [1, 32768]^2; an r2_cap[k], k < K, negative or beyond FO_HIDDEN_REACH_MAX_HALO; map_of[c], c < C, outside [0, K); M < 0; L outside
 * [1, 64]; no h_levels; a level negative or not finite; levels that are not strictly ascending; dt not positive and finite; a_limit
 * negative or NaN; with M > 0: T outside [1, 254]; B outside [1, T]; C * T > FO_HIDDEN_BRAKE_MAX_TABLE;
 * 4 * C * T + 8 * L > FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES; a row that is negative, decreases or ends beyond
 * 169 * r2_cap[map_of[c]]; no d_x / d_y / d_heading; no d_key[k] or d_qmin[k], k < K; no d_v or d_arc; a missing output; only one of
 * d_cost_or_null / d_safe_or_null; extents refused as by fo_scene_hidden_reach.  FO_E_STATE: no scene. */
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* as handed to the clearances */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* the clearances' window */
  int32_t K;                                /* maps */
  int32_t C;                                /* classes */
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];   /* [win_ny][win_nx] each: the clearances' key maps (INPUT) */
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];  /* [M][T] each: the clearances' minimum per pose (INPUT) */
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];         /* the clearances' caps */
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];      /* the map of class c, in [0, K) */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  const double *h_levels;                   /* HOST [L] decelerations, m/s^2, strictly ascending */
  int32_t L;                                /* levels */
  int32_t B;                                /* brake starts b = 0 .. B-1 */
  double dt;
  const int32_t *h_thr;                     /* HOST [C][T]: 169 * R2_c[j] */
  double a_limit;                           /* decel above it takes safety away; +inf: only "no level" does */
  const uint8_t *d_finite_or_null;          /* [M] */
  double *d_cost_or_null;                   /* [M][FO_NC] of the step: both or neither */
  uint8_t *d_safe_or_null;                  /* [M] */
  int32_t *d_need, *d_at, *d_blocking, *d_user;     /* [M] */
  double *d_decel;                          /* [M] */
  int32_t *d_need_of, *d_first;             /* [C][M] */
} fo_hidden_brake_ladder_verdict_t;
int fo_scene_hidden_brake_ladder_verdict(fo_ctx *ctx, const fo_hidden_brake_ladder_verdict_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic IMPACT VERDICT (DESIGN.md §5.10 "Impact verdict") -- "if hidden traffic is
 * there, how bad is what braking cannot avoid?": per candidate the worst harm that remains after braking from one of the brake
 * starts it executes before it replans, in the reference's own unit (the MAIS3+ probability of metrics/utils/harm_model.py), as a
 * finite, graded term in the two reserved columns of the cost row and the safety flag that fo_step_run leaves in HBM.  It still
 * orders a fan of candidates where "can it stop clear?" is "no" for every one.  The walk of fo_scene_hidden_brake_verdict, which
 * keeps the speed the ego has left where a manoeuvre is hit.  Opt-in and additive: one launch on the caller's stream, behind the
 * step whose cost rows it folds into; nothing is read back.  It writes the SAME two reserved columns as the two verdicts above: a
 * step runs one of the three stages.
 *  Inputs: those of fo_scene_hidden_brake_verdict word for word, without commit_min, and: d_speed_of [C] float64, the speed of class
 *   c in m/s; d_harm_rows [C][4] float64, the rows (p0, p1, p2, p3) of the classes (fo_hidden_impact_row; what a row means stands in
 *   csrc/fo_hidden_impact.hpp: the reference's harm head-on and at the worst area of impact); harm_limit, float64, >= 0, +inf
 *   allowed, not NaN.  Both buffers live on the device: the caller builds them once per set of users and keeps them.
 *  Write Lm for the length as in the verdict entry, ends = min(B, Lm), v for d_v, and fm[c] = first[c][m], bf[c], st for the first
 *   hit of class c on the manoeuvre that brakes from b and that manoeuvre's stop sample, as fo_scene_hidden_brake_users writes them
 *   (brake_first[c][m][b], stop[m][b]).
 *  1. Brake start b < ends is HIT by class c iff (0 <= fm[c] <= b) or (0 <= bf[c] < st): the commit rule of the verdict entry.
 *  2. The ego speed at the hit u(c, b): if 0 <= fm[c] <= b, u = v[m][fm[c]] (the candidate itself is met at sample fm[c], before
 *   braking from b changes anything); otherwise u = max(v[m][b] - a_brake * ((bf[c] - b) * dt), 0), the manoeuvre's speed at its
 *   first hit -- positive, since bf[c] < st.
 *  3. speed[c][m] = the greatest u(c, b) over the hit starts b (compared by >: a NaN never wins; -inf is the value before the first
 *   one), at[c][m] = the lowest b that attains it; with no hit start (or none whose u compares): speed = 0.0, at = -1.
 *   commit[c][m] and first[c][m] are fo_scene_hidden_brake_verdict's, bit for bit.
 *  4. With w = speed[c][m] + speed_of[c]: obstacle harm of class c = 1 / (1 + exp(p0 + p1 * w)), ego harm = 1 / (1 + exp(p2 + p3 * w));
 *   float64, plain exp, no contraction.
 *  5. user[m] = the lowest c with at[c][m] >= 0 whose obstacle harm is greatest (compared by >), -1 where no class has a hit;
 *   harm[m] = (obstacle harm, ego harm) of that class, (0.0, 0.0) for -1.
 *  6. finite[m] == 0: harm[m] = (1.0, 1.0) and user[m] = FO_HIDDEN_VERDICT_NOT_FINITE, whatever the walk found (a NaN pose fails
 *   every footprint comparison and would read as "no hit": this case fails CLOSED); speed, at, commit and first stay the walk's.
 *  7. With d_cost / d_safe: cost[m][FO_C_RES0] = harm[m][0], cost[m][FO_C_RES1] = (double)user[m]; if harm[m][0] > harm_limit or
 *   the candidate is not finite: safe[m] = 0 and cost[m][FO_C_SAFE] = 0.0, otherwise both are left as found -- the stage only ever
 *   takes safety away; a row that a refused rule list or an unusable covariance poisoned keeps its NaNs and safe = 0 and gets the
 *   two columns.  No other column is touched.
 *  Outputs, every byte written by every call: d_harm [M][2] float64; d_user [M] int32; d_speed [C][M] float64; d_at, d_commit,
 *   d_first [C][M] int32.
 *  Safety of the data: as fo_scene_hidden_brake_users; finite, speed_of and the rows may hold anything, no index depends on them.
 *  Not claimed: what fo_scene_hidden_brake_users does not claim; the bound is head-on and worst-area for every user (a lane-bound
 *   vehicle that can only arrive from the side is still priced head-on: fo_scene_hidden_brake_impact_lanes below prices it by the
 *   angle the lanes allow); a standing ego that is reached carries no harm (the
 *   family's "moving ego" convention), so the quantity jumps where a manoeuvre just comes to rest; brake starts b >= B are not
 *   looked at; there is no collision probability -- this is harm, not risk; that cost / safe belong to the same candidates is the
 *   caller's word.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, no byte written, messages prefixed
 * "fo_scene_hidden_brake_impact:"), in this order: K outside [1, 3]; C outside [1, 8]; no h_thr; a window outside [1, 32768]^2; an
 * r2_cap[k], k < K, negative or beyond FO_HIDDEN_REACH_MAX_HALO; map_of[c], c < C, outside [0, K); M < 0; a_brake negative or not
 * finite; dt not positive and finite; harm_limit negative or NaN; with M > 0: T outside [1, 254]; B outside [1, T];
 * C * T > FO_HIDDEN_BRAKE_MAX_TABLE; a row of h_thr that is negative, decreases or ends beyond 169 * r2_cap[map_of[c]]; no d_x /
 * d_y / d_heading; no d_key[k] or d_qmin[k], k < K; no d_v or d_arc; no d_speed_of or d_harm_rows; a missing output; only one of
 * d_cost_or_null / d_safe_or_null; extents refused as by fo_scene_hidden_reach.  FO_E_STATE: no scene. */
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* as handed to the clearances */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* the clearances' window */
  int32_t K;                                /* maps */
  int32_t C;                                /* classes */
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];   /* [win_ny][win_nx] each: the clearances' key maps (INPUT) */
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];  /* [M][T] each: the clearances' minimum per pose (INPUT) */
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];         /* the clearances' caps */
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];      /* the map of class c, in [0, K) */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  double a_brake, dt;
  const int32_t *h_thr;                     /* HOST [C][T]: 169 * R2_c[j] */
  int32_t B;                                /* brake starts b = 0 .. B-1 */
  const double *d_speed_of;                 /* [C] speed of class c, m/s */
  const double *d_harm_rows;                /* [C][4] (p0, p1, p2, p3) */
  double harm_limit;                        /* obstacle harm above it takes safety away; +inf: only non-finite candidates lose it */
  const uint8_t *d_finite_or_null;          /* [M] */
  double *d_cost_or_null;                   /* [M][FO_NC] of the step: both or neither */
  uint8_t *d_safe_or_null;                  /* [M] */
  double *d_harm;                           /* [M][2] (obstacle, ego) */
  int32_t *d_user;                          /* [M] */
  double *d_speed;                          /* [C][M] */
  int32_t *d_at, *d_commit, *d_first;       /* [C][M] */
} fo_hidden_brake_impact_t;
int fo_scene_hidden_brake_impact(fo_ctx *ctx, const fo_hidden_brake_impact_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic IMPACT VERDICT BY APPROACH ANGLE (DESIGN.md §5.10 "Impact verdict by approach
 * angle") -- the impact verdict above with every LANE-BOUND class of road user priced at the worst closing speed the lanes' driving
 * directions allow at the cells where it meets the ego, instead of the worst that is conceivable at all: the reference's
 * dv = sqrt(v_ego^2 + v_obs^2 + 2 v_ego v_obs cos(pdof)), pdof = yaw_obs - theta_ego + pi (metrics/utils/harm_model.py:81-95), at the
 * greatest cos(pdof) over the headings the map's move table (fo_scene_set_lane_moves) leaves a lane-abiding vehicle there.  Classes
 * that are not lane-bound, off-lane cells and every byte that says nothing stay head-on: no output is above the head-on entry's, and
 * where nothing is known every output is that entry's.  One launch; opt-in and additive like the entry above.
 *  A move byte and a heading: bit k of a cell's byte is set iff cos(k * 45deg - yaw) >= cos(67.5deg) for a lanelet of heading yaw
 *   that contains the cell (the union over those lanelets, 0xFF off-lane).  Direction k is CENTRAL in a byte when bits k - 1, k and
 *   k + 1 (mod 8) are all set; every heading that generates a byte with a central direction lies within 22.5deg of a central one.
 *   The headings a byte leaves are H = the union over its central k of [k * 45deg - h, k * 45deg + h], h = 22.5deg + heading_slack;
 *   a byte without a central direction says nothing.
 *  Inputs: those of fo_scene_hidden_brake_impact word for word, and: dir_mask, bit c set = class c is lane-bound; cos_h, sin_h,
 *   float64, the cosine and sine of h as the caller's host computed them, both in [-1, 1]; cos_h <= -1 states h >= pi: every class
 *   is head-on.  With dir_mask != 0 the context's map must have a move table.
 *  Steps 1, 6 and 7, the commit rule, commit, first, the fail-closed rule and the fold are fo_scene_hidden_brake_impact's word for
 *   word.  Steps 2 - 5 become:
 *  2. The hit pose of a hit start b of class c, its sample i and its cells: if 0 <= fm[c] <= b the candidate's own pose at sample
 *   i = fm[c]; otherwise the manoeuvre's pose at sample i = bf[c] (the pose the walk of fo_scene_hidden_brake_users held when it set
 *   bf[c]).  The HIT CELLS are the cells the footprint scan of that pose visits -- centre inside the rectangle by the scan's float64
 *   test -- whose key on map map_of[c] is <= thr[c][i]; outside the window a cell carries 0 on raster road and NONE elsewhere, as in
 *   the walk.  mv(c, b) = the OR of the move bytes of the hit cells: the table's byte for a cell on the raster, 0xFF for one off it.
 *  3. The approach cosine cm(c, b), the greatest cos(pdof) the lanes allow: cm = 1.0 exactly if class c is not in dir_mask, or mv
 *   has no central direction, or cos_h <= -1.  Otherwise with (ct, st) the hit pose's unit heading and (ck, sk) the lattice unit
 *   vector of direction k (0, +-1, +-sqrt(0.5)): g_k = -(ct * ck + st * sk); c_k = 1.0 if g_k >= cos_h, else
 *   g_k * cos_h + sqrt(fmax(0, 1 - g_k * g_k)) * sin_h; cm = the greatest c_k over the central k, compared by >, starting from the
 *   first central k.  float64, this operation order, no contraction, no trigonometric call.
 *  4. The closing speed w(c, b): with u the ego speed at the hit exactly as step 2 of the entry above and s = speed_of[c]:
 *   w = u + s if cm == 1.0 (bit for bit the head-on entry's), otherwise w = sqrt(fmax(0, u * u + s * s + 2 * u * s * cm)).
 *  5. closing[c][m] = the greatest w(c, b) over the hit starts b < ends (compared by >: a NaN never wins), at[c][m] = the lowest b
 *   that attains it, cosine[c][m] = cm at that start; without a hit start (or none whose w compares) 0.0, -1 and 1.0.  The harms
 *   of class c are the two logistics of its row at w = closing[c][m] -- the rows still carry the mass split and the worst area of
 *   impact.  user, harm, the non-finite rule and the fold as in the entry above.
 *  Consequences: closing <= speed + speed_of of the head-on entry for every (c, m), hence harm <= its harm (the rows' speed
 *   coefficients are negative); with dir_mask == 0, a table of 0xFF alone or cos_h <= -1 every output shared with the head-on entry
 *   is that entry's bit for bit and closing == speed + speed_of bit for bit.
 *  Outputs, every byte written by every call: d_harm [M][2] float64; d_user [M] int32; d_closing, d_cosine [C][M] float64; d_at,
 *   d_commit, d_first [C][M] int32.
 *  Not claimed: what fo_scene_hidden_brake_impact does not claim, but for the head-on pricing of lane-bound classes; a lane-abiding
 *   vehicle is taken to head along its lane -- lane changes and swerves are what heading_slack is for; the area of impact stays
 *   worst-case (the relative position at the hit is unknown); at an intersection cell the union of the lanelets widens the sector;
 *   the maximum is over the closing speed per class, so the start `at` names can differ from the head-on entry's; the ego speed at
 *   that start is not an output -- closing and cosine are.
 * Refusals: those of fo_scene_hidden_brake_impact in its order (messages prefixed "fo_scene_hidden_brake_impact_lanes:"), and, after
 * harm_limit: FO_E_ARG for a dir_mask with bits at or above C, cos_h or sin_h not finite or outside [-1, 1]; where that entry asks for
 * d_speed: d_closing and d_cosine.  FO_E_STATE: no scene; dir_mask != 0 and the map has no move table. */
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;
  int32_t win_ix0, win_iy0, win_nx, win_ny;
  int32_t K;
  int32_t C;
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];
  const double *d_v;
  const double *d_arc;
  double a_brake, dt;
  const int32_t *h_thr;                     /* HOST [C][T] */
  int32_t B;
  const double *d_speed_of;                 /* [C] */
  const double *d_harm_rows;                /* [C][4] */
  double harm_limit;
  const uint8_t *d_finite_or_null;          /* [M] */
  double *d_cost_or_null;                   /* [M][FO_NC]: both or neither */
  uint8_t *d_safe_or_null;                  /* [M] */
  double *d_harm;                           /* [M][2] (obstacle, ego) */
  int32_t *d_user;                          /* [M] */
  double *d_closing;                        /* [C][M] the closing speed that is priced, m/s */
  int32_t *d_at, *d_commit, *d_first;       /* [C][M] */
  uint32_t dir_mask;                        /* bit c: class c is lane-bound */
  double cos_h, sin_h;                      /* of h = 22.5deg + heading_slack */
  double *d_cosine;                         /* [C][M] the approach cosine at `at` */
} fo_hidden_brake_impact_lanes_t;
int fo_scene_hidden_brake_impact_lanes(fo_ctx *ctx, const fo_hidden_brake_impact_lanes_t *p, void *stream);

/* The harm row of a class of hidden road user, on the host (needs no context and no device): row = (p0, p1, p2, p3) for a road
 * user of `type` (FO_TYPE_*) and `size` = length * width in m^2 against an ego of ego_mass kg (csrc/fo_hidden_impact.hpp, where what
 * a row means stands).  FO_OK, or FO_E_ARG: no hc / row, a type whose protection entry is None (FO_TYPE_STRUCTURE and anything
 * outside the FO_TYPE_* codes), size or ego_mass not positive and finite. */
int fo_hidden_impact_row(int type, double size, double ego_mass, const fo_harm_coeff_t *hc, double *row);

/* EXTENSION, not part of the reference: hidden-traffic HARM LADDER (DESIGN.md §5.10 "Harm ladder") -- "how hard must the ego be
 * prepared to brake, from the worst of the brake starts it executes before it replans, so that the harm of what still hits it stays
 * within harm_limit?": the reference's brake threat number (metrics/be.py:56) against hidden road users with "no collision" relaxed
 * to "harm within the threshold" (metrics/metric.py:63-68).  It lies between the two stages above: finite where the ladder verdict
 * says "no level", graded over the decelerations where the impact verdict prices one.  The walk of
 * fo_scene_hidden_brake_ladder_verdict; every hit is priced on the spot as fo_scene_hidden_brake_impact prices it.  Opt-in and
 * additive: one launch on the caller's stream, behind the step whose cost rows it folds into; nothing is read back.  It writes the
 * SAME two reserved columns as the three stages above: a step runs one of the four.
 *  Inputs: those of fo_scene_hidden_brake_ladder_verdict word for word -- h_levels [L] strictly ascending, B, a_limit,
 *   d_finite_or_null, d_cost_or_null / d_safe_or_null both or neither -- and, from fo_scene_hidden_brake_impact: d_speed_of [C],
 *   d_harm_rows [C][4] (device buffers, float64) and harm_limit, float64, >= 0, +inf allowed, not NaN.
 *  Write bf, st and fm for what fo_scene_hidden_brake_ladder_users writes on the same inputs as brake_first[c][m][b][l],
 *   stop[m][b][l] and first[c][m], v for d_v, and ends = min(B, Lm).
 *  1. Hit: brake start b < ends at level l is HIT by class c iff (0 <= fm <= b) or (0 <= bf < st), the family's commit rule.
 *  2. The ego speed at the hit: u = v[m][fm] where 0 <= fm <= b, else max(v[m][b] - levels[l] * ((bf - b) * dt), 0): step 2 of
 *   fo_scene_hidden_brake_impact at a_brake = levels[l].
 *  3. The harm at the hit: ho(c, m, b, l) = 1 / (1 + exp(rows[c][0] + rows[c][1] * (u + speed_of[c]))): head-on, float64, plain exp,
 *   no contraction.
 *  4. over(c, m, b, l) = hit and ho > harm_limit.  A NaN never counts as over.
 *  5. The ladder reduction: steps 1 - 7 of fo_scene_hidden_brake_ladder_verdict with `over` in the place of "unclear" -- ra, blk and
 *   req are formed from `over` by the rules fo_scene_hidden_brake_ladder_users forms required_all, blocking and required by; need, at,
 *   blocking, user, decel, need_of, first (the walk's, unchanged), the fail-closed row of a non-finite candidate and the fold
 *   (cost[m][FO_C_RES0] = decel[m], cost[m][FO_C_RES1] = (double)user[m]; safety is lost where need[m] == L or decel[m] > a_limit)
 *   are that entry's with their meanings unchanged.
 *  6. The curve: harm_at[m][l] (float64) = the greatest ho(c, m, b, l) over the hit (c, b < ends), compared by > from -1.0, which is
 *   below every harm (a NaN never wins); user_at[m][l] (int32) = the lowest class that attains it; 0.0 and -1 without a hit (or
 *   none whose harm compares).  finite[m] == 0: harm_at[m][l] = 1.0 and user_at[m][l] = FO_HIDDEN_VERDICT_NOT_FINITE at every level.
 *  Consequences: harm_limit = 0.0 gives fo_scene_hidden_brake_ladder_verdict bit for bit on the shared outputs (every logistic is
 *   positive); harm_limit = +inf gives need = 0 wherever ends > 0; harm_at[m][l] <= harm_limit implies need[m] <= l, and need[m] == L
 *   implies harm_at[m][l] > harm_limit at every l; need never rises with harm_limit and never exceeds the ladder verdict's;
 *   harm_at[:, l] is the obstacle harm of fo_scene_hidden_brake_impact at a_brake = levels[l].
 *  Outputs, every byte written by every call: d_need, d_at, d_blocking, d_user [M] int32; d_decel [M] float64; d_need_of, d_first
 *   [C][M] int32; d_harm_at [M][L] float64; d_user_at [M][L] int32.
 *  Safety of the data: as fo_scene_hidden_brake_ladder_users; finite, speed_of and the rows may hold anything, no index depends on
 *   them.
 *  Not claimed: what the ladder verdict and the impact verdict do not claim; every user is priced HEAD-ON and at the worst area of
 *   impact (the approach angle of fo_scene_hidden_brake_impact_lanes is not taken here: fo_scene_hidden_brake_harm_ladder_lanes below
 *   takes it); harder braking is not always safer against an
 *   arrival map, so harm_at need not fall with l -- need is the first sufficient level of every start, not the last insufficient one.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, no byte written, messages prefixed
 * "fo_scene_hidden_brake_harm_ladder:"): those of fo_scene_hidden_brake_ladder_verdict in its order (a missing output includes
 * d_harm_at and d_user_at), then, with M > 0: no d_speed_of; no d_harm_rows; harm_limit negative or NaN.  FO_E_STATE: no scene. */
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;                        /* as handed to the clearances */
  int32_t win_ix0, win_iy0, win_nx, win_ny; /* the clearances' window */
  int32_t K;                                /* maps */
  int32_t C;                                /* classes */
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];   /* [win_ny][win_nx] each: the clearances' key maps (INPUT) */
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];  /* [M][T] each: the clearances' minimum per pose (INPUT) */
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];         /* the clearances' caps */
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];      /* the map of class c, in [0, K) */
  const double *d_v;                        /* [M][T] speed at each sample, m/s */
  const double *d_arc;                      /* [M][T] travelled chord length, m */
  const double *h_levels;                   /* HOST [L] decelerations, m/s^2, strictly ascending */
  int32_t L;                                /* levels */
  int32_t B;                                /* brake starts b = 0 .. B-1 */
  double dt;
  const int32_t *h_thr;                     /* HOST [C][T]: 169 * R2_c[j] */
  double a_limit;                           /* decel above it takes safety away; +inf: only "no level" does */
  const uint8_t *d_finite_or_null;          /* [M] */
  double *d_cost_or_null;                   /* [M][FO_NC] of the step: both or neither */
  uint8_t *d_safe_or_null;                  /* [M] */
  int32_t *d_need, *d_at, *d_blocking, *d_user;     /* [M] */
  double *d_decel;                          /* [M] */
  int32_t *d_need_of, *d_first;             /* [C][M] */
  const double *d_speed_of;                 /* [C] speed of class c, m/s */
  const double *d_harm_rows;                /* [C][4] (p0, p1, p2, p3); p0 and p1 are read */
  double harm_limit;                        /* a hit at a harm above it counts; 0: every hit does, +inf: none */
  double *d_harm_at;                        /* [M][L] the greatest harm level l leaves */
  int32_t *d_user_at;                       /* [M][L] the lowest class that attains it */
} fo_hidden_brake_harm_ladder_t;
int fo_scene_hidden_brake_harm_ladder(fo_ctx *ctx, const fo_hidden_brake_harm_ladder_t *p, void *stream);

/* EXTENSION, not part of the reference: hidden-traffic HARM LADDER BY APPROACH ANGLE (DESIGN.md §5.10 "Harm ladder by approach
 * angle") -- the harm ladder above with every LANE-BOUND class of road user priced at the worst closing speed the lanes' driving
 * directions allow at the cells where it meets the ego, as fo_scene_hidden_brake_impact_lanes prices it, instead of head-on: the
 * deceleration the ego must be prepared for is no longer an upper bound for a vehicle that can only arrive from the side.  One
 * launch; opt-in and additive like the entry above.  It writes the SAME two reserved columns as the four stages above: a step runs
 * one of the five.
 *  Inputs: those of fo_scene_hidden_brake_harm_ladder word for word, and: dir_mask, cos_h, sin_h with the meaning they have in
 *   fo_scene_hidden_brake_impact_lanes (bit c set = class c is lane-bound; the cosine and sine of h = 22.5deg + heading_slack from
 *   the caller's host, both in [-1, 1]; cos_h <= -1 states h >= pi: every class is head-on).  With dir_mask != 0 the context's map
 *   must have a move table.
 *  Steps 1, 2, 4, 5 and 6 of fo_scene_hidden_brake_harm_ladder hold word for word.  Step 3 becomes:
 *  3. For a hit (c, m, b, l) the hit pose, its sample i, its hit cells and mv are step 2 of fo_scene_hidden_brake_impact_lanes at
 *   a_brake = levels[l]: where 0 <= fm[c] <= b the candidate's own pose at i = fm[c], otherwise the manoeuvre's pose at
 *   i = bf[c][m][b][l].  cm is that entry's step 3; w is its step 4 with u from this entry's step 2; the harm at the hit is
 *   ho(c, m, b, l) = 1 / (1 + exp(rows[c][0] + rows[c][1] * w)).  float64, this operation order, no contraction.
 *  Consequences:
 *   (a) with dir_mask == 0, a move table of 0xFF alone or cos_h <= -1 every output is fo_scene_hidden_brake_harm_ladder's bit for
 *    bit (cm == 1.0 and w = u + speed_of[c] exactly); hence harm_limit = 0.0 then gives fo_scene_hidden_brake_ladder_verdict bit
 *    for bit on the shared outputs;
 *   (b) w <= u + speed_of[c] and the rows' speed coefficients are negative, so ho <= the head-on ho for every (c, m, b, l):
 *    harm_at <= the head-on entry's harm_at for every (m, l), and need <= its need -- `over` is a subset per (c, m, b, l) and the
 *    ladder reduction is monotone in it (the same argument by which need never rises with harm_limit);
 *   (c) harm_at[:, l] is the obstacle harm of fo_scene_hidden_brake_impact_lanes at a_brake = levels[l] and the same B, user_at its
 *    user wherever no two classes tie;
 *   (d) harm_limit = +inf gives need = 0 wherever ends > 0; harm_at[m][l] <= harm_limit implies need[m] <= l, and need[m] == L
 *    implies harm_at[m][l] > harm_limit at every l, as in the head-on entry.
 *  Outputs, every byte written by every call: those of fo_scene_hidden_brake_harm_ladder.
 *  Safety of the data: as fo_scene_hidden_brake_harm_ladder; the move table is read at cells tested against the raster alone, and
 *   only for a class of dir_mask.
 *  Not claimed: what fo_scene_hidden_brake_harm_ladder does not claim, but for the head-on pricing of lane-bound classes; what
 *   fo_scene_hidden_brake_impact_lanes does not claim about a lane-abiding vehicle (it heads along its lane; the area of impact stays
 *   worst-case; at an intersection cell the union of the lanelets widens the sector); the cosine and the closing speed of a hit
 *   are not outputs -- fo_scene_hidden_brake_impact_lanes at a_brake = levels[l] names them for the worst start of a class.
 * M = 0: FO_OK, nothing launched.  FO_E_ARG (nothing is launched, no byte written, messages prefixed
 * "fo_scene_hidden_brake_harm_ladder_lanes:"): those of fo_scene_hidden_brake_harm_ladder in its order, then, behind harm_limit: a
 * dir_mask with bits at or above C; cos_h or sin_h not finite or outside [-1, 1].  FO_E_STATE: no scene; behind those, dir_mask != 0
 * and the map has no move table. */
typedef struct {
  int32_t M, T;
  const double *d_x, *d_y;                  /* [M][T] */
  const double *d_heading;                  /* [M][T][2] unit (cos, sin) */
  const int32_t *d_len_or_null;             /* [M] */
  double hl, hw, wb;
  int32_t win_ix0, win_iy0, win_nx, win_ny;
  int32_t K;
  int32_t C;
  const int32_t *d_key[FO_HIDDEN_BRAKE_MAX_MAPS];
  const int32_t *d_qmin[FO_HIDDEN_BRAKE_MAX_MAPS];
  int32_t r2_cap[FO_HIDDEN_BRAKE_MAX_MAPS];
  int32_t map_of[FO_HIDDEN_BRAKE_MAX_CLASSES];
  const double *d_v;
  const double *d_arc;
  const double *h_levels;                   /* HOST [L] */
  int32_t L;
  int32_t B;
  double dt;
  const int32_t *h_thr;                     /* HOST [C][T] */
  double a_limit;
  const uint8_t *d_finite_or_null;          /* [M] */
  double *d_cost_or_null;                   /* [M][FO_NC]: both or neither */
  uint8_t *d_safe_or_null;                  /* [M] */
  int32_t *d_need, *d_at, *d_blocking, *d_user;     /* [M] */
  double *d_decel;                          /* [M] */
  int32_t *d_need_of, *d_first;             /* [C][M] */
  const double *d_speed_of;                 /* [C] */
  const double *d_harm_rows;                /* [C][4] */
  double harm_limit;
  double *d_harm_at;                        /* [M][L] */
  int32_t *d_user_at;                       /* [M][L] */
  uint32_t dir_mask;                        /* bit c: class c is lane-bound */
  double cos_h, sin_h;                      /* of h = 22.5deg + heading_slack */
} fo_hidden_brake_harm_ladder_lanes_t;
int fo_scene_hidden_brake_harm_ladder_lanes(fo_ctx *ctx, const fo_hidden_brake_harm_ladder_lanes_t *p, void *stream);

/* Phantom sampling in the occluded cells + constant-velocity predictions (replaces the cell-based core of
 * SpawnLocator.find_spawn_points, spawn_locator.py:80-139, and agent.py:451-536).  Candidates: occluded cells at least
 * min_ahead ahead of the ego and within max_dist, on the visible/occluded frontier (all_occluded = 0) or anywhere in
 * the occluded set (all_occluded = 1); evenly spaced ranks are kept.  Prediction slots: R = max(routes, 1) per
 * agent, slot j * R + r; with routes > 0 (needs fo_scene_set_routes) a vehicle on a lanelet gets one prediction per
 * candidate route r (constant speed along the route, lateral offset kept; replaces route_planner.py:31-90 +
 * utils/frenetix_handler.py + agent.py:283-426), everything else one straight constant-velocity prediction in r = 0.
 * The per-prediction outputs (d_pos ... d_len) therefore hold max_agents * R slots.  Agent j takes pattern slot j % 4
 * (type4/speed4/raw/inflated dims: HOST arrays of 4).  d_path [n_path][2] = ego reference path.  Outputs for
 * max_agents slots, directly in the layout fo_sweep_set_agents consumes (slots >= *d_n have len 0 = inactive). */
int fo_scene_spawn(fo_ctx *ctx, const uint8_t *d_cls, int win_ix0, int win_iy0, int win_nx, int win_ny, double ego_x,
                   double ego_y, double head_x, double head_y, double min_ahead, double max_dist, int all_occluded,
                   int max_agents, int routes, const int32_t *type4, const double *speed4, const double *raw_l4, const double *raw_w4,
                   const double *infl_l4, const double *infl_w4, int n_path, const double *d_path, int T, double dt,
                   double var0, double var_factor, int32_t *d_cell, double *d_pos0, double *d_yaw0, int32_t *d_n,
                   double *d_pos, double *d_yaw, double *d_v, double *d_cov, double *d_shape, double *d_raw_dims,
                   int32_t *d_type, int32_t *d_len, void *stream);
int fo_scene_candidate_count(fo_ctx *ctx, int32_t *h_n, void *stream);

/* ---- the reference's three spawn rule families on the cell classes (replaces SpawnLocator.find_spawn_points' rule
 *      functions: pedestrian behind a visible static obstacle, spawn_locator.py:323-476; pedestrian behind a turn,
 *      :481-578; Car / Bicycle behind a visible dynamic obstacle, :145-317 with the rectangle fit of :695-726).  The
 *      reference asks shapely for intersections with the visible / occluded polygons; here the same predicates are asked
 *      of the cell classes.  The curvilinear frame is the polyline frame of the ego's reference path. */

/* One-off, after fo_scene_set_map (HOST arrays, lanelet index = order of the polygons): first vertex of every lanelet's
 * left bound [P][2] (spawn_locator.py:424), index of predecessors[0] and of adj_left per lanelet (-1 = none; :249-252,
 * :196-202), and the intersections: entries [off[i], off[i+1]) of (lanelet index, kind: 0 incoming, 1 inner = the left /
 * right / straight successors of an incoming element) for intersection i (:171-195). */
int fo_scene_set_topology(fo_ctx *ctx, int P, const double *h_left0, const int32_t *h_pred0, const int32_t *h_adj_left,
                          int n_inter, const int32_t *h_inter_off, const int32_t *h_inter_lanelet,
                          const uint8_t *h_inter_kind);

/* per-step scalars of the rules: ego pose, its curvilinear position, s_threshold = s_ego + max(4 v_ego, 25)
 * (spawn_locator.py:65-66,113), the ego's intention (0 straight ahead, 1 left turn, 2 right turn: curvature of the next
 * 40 m of the reference path, :678-693,729-741) and that window as vertex range [win_i0, win_i1) of the path table, the
 * switches and maxima of the YAML (spawn_locator section), the pedestrian's width / length (agent_manager section).
 * n_dynamic_plus1 (ABI 11): 1 + the number of this step's obstacles whose flags allow the dynamic-obstacle rule at all -- present
 * (bit0), dynamic role (bit2), neither bicycle nor pedestrian (bit3 clear) -- or 0 = not told (every obstacle is assumed to).  The
 * rule's helper workgroups (fifteen per obstacle, a CU each) are launched for that many obstacles only -- the first ones in list
 * order whose flags qualify; one beyond the count is treated as if the rule did not apply to it -- and for none at all when no
 * obstacle qualifies: the flags are the caller's own data, whether such an obstacle is visible stays a decision of the device.
 * frame: the table d_path6 holds -- 0 the polyline frame of the reference path, 1 a table sampled from the caller's own
 * curvilinear frame (see d_path6 below); any other value is FO_E_ARG.  (It was a reserved zero word: callers that leave it 0
 * get what they got before.) */
typedef struct {
  double ego_x, ego_y, ego_yaw, ego_s, ego_d, s_threshold;
  double ped_width, ped_length;
  int32_t intention, win_i0, win_i1;
  int32_t behind_static, behind_turn, behind_dynamic, max_static, max_dynamic;
  int32_t n_dynamic_plus1, frame;
} fo_spawn_rule_params_t;

/* Per step, after fo_scene_visibility on the same stream.  d_cls + window: that call's cell classes.  d_path6 [n_path][6]:
 * with params->frame = 0, the polyline frame of the reference path: x, y, arc length, segment length, unit tangent (last row:
 * tangent unused).  With params->frame = 1, the caller's frame sampled at the path's vertices p_i: x, y of p_i (the base point),
 * the caller's s_i (strictly increasing), the polyline arc length of p_i from the path's first vertex (the s at which the turn
 * rule asks the caller's frame for its shifted line, as the reference does), the caller's normal n_i = cart(s_i, 1) - cart(s_i, 0)
 * (not normalised); between two rows base point and normal are interpolated linearly in s, (s, d) <-> b(s) + d n(s), a point
 * without a root of cross(q - b, n) = 0 on any segment is outside the domain.  Obstacles at this
 * step: d_ocorn [O][4][2], d_ocen [O][2], d_oyaw [O], d_odims [O][2] (length, width), d_oflags [O] (bit0 present, bit1
 * occludes, bit2 dynamic role, bit3 type bicycle or pedestrian), d_obst_vis [O] = visible_objects_timestep of
 * fo_scene_visibility.  Output d_out [max_out][8]: type (FO_TYPE_*), x, y, orientation (NaN = to be derived,
 * agent.py:475-481), curvilinear s, d (NaN = none), source (1 behind dynamic obstacle, 2 behind static obstacle, 3 left
 * turn, 4 right turn), obstacle index (-1 = none), in the reference's order (dynamic, static, turn); d_n_out [1].
 * max_out must hold what the maxima allow -- (max_dynamic + 2) + (max_static + 1) + 1 points with all three families
 * switched on: the reference compares its maxima before it appends, and one dynamic obstacle can yield a Car and a Bicycle
 * (spawn_locator.py:212,304-309,365) -- else FO_E_ARG (a short buffer would drop the last points unnoticed).
 * Table space: the turn rule holds a reference window of <= 1 536 path vertices, the dynamic-obstacle rule flags for <= 9 409
 * lanelets and every fifth of <= 2 560 window vertices, max_static <= 15 -- beyond: FO_E_ARG.  What only the device can tell: an
 * obstacle's centre on more than sixteen lanelets or on more than seven relevant ones, a line a rule samples (cell size / 8
 * apart: the 40 m window, an obstacle's cross line: its extent across the path + 1.6 m) of more than 1 024 samples -- then
 * *d_n_out = -1 and there is no list.  Only a record the selection consumes can refuse the step: the turn record with the
 * turn rule on, an obstacle the distance-ordered selection visits before max_dynamic / max_static end it (the reference's
 * list does not depend on the obstacles behind that point).
 * What the library guarantees for a refused step: fo_scene_spawn_rule_agents and fo_step_run add no rule agents and mark
 * the agent set, and every sweep over it fails closed -- NaN costs, safe = 0, FO_E_STATE from fo_sweep_check ("A refused
 * rule list" at fo_sweep_check).  What is left to the caller: d_out and the pair / list buffers of such a step are
 * unspecified, and a host that reads the spawn-point list itself must refuse a negative count (the Python host view
 * raises RuntimeError). */
int fo_scene_spawn_rules(fo_ctx *ctx, const uint8_t *d_cls, int win_ix0, int win_iy0, int win_nx, int win_ny, int n_path,
                         const double *d_path6, int O, const double *d_ocorn, const double *d_ocen, const double *d_oyaw,
                         const double *d_odims, const uint8_t *d_oflags, const uint8_t *d_obst_vis,
                         const fo_spawn_rule_params_t *params, int max_out, double *d_out, int32_t *d_n_out, void *stream);

/* One-off, optional, after fo_scene_set_map (HOST arrays, lanelet index = order of the polygons): the centre line of every
 * lanelet, vertices xy[off[p] .. off[p+1]).  Read by fo_scene_spawn_rule_agents: a pedestrian spawned behind a turn heads
 * for the centre of the lanelet it stands on (mode 'lane_center', agent.py:459-467; interface.py:194).  Part of the
 * static map (FO_E_STATE while the map is shared, like fo_scene_set_routes). */
int fo_scene_set_centerlines(fo_ctx *ctx, int P, const int32_t *h_off, const double *h_xy);

/* per agent type the rule families spawn -- index 0 Car, 1 Bicycle, 2 Pedestrian: default speed, un-inflated and inflated
 * dimensions (YAML agent_manager section; agent.py:69-140,402-409,523-524) */
typedef struct { double speed[3], raw_l[3], raw_w[3], infl_l[3], infl_w[3]; } fo_rule_agent_types_t;

/* Per step, after fo_scene_spawn_rules on the same stream: the rule families' spawn points become phantom agents ON THE
 * DEVICE (replaces the loop over spawn points of FOInterface.evaluate_scenario, interface.py:186-198, with
 * FOAgentManager.add_agent, agent.py:46-141, OAPPedestrianAgent, :429-536, and OAPVehicleAgent, :283-426, behind it).
 * d_points [max_points][8] / d_n_points [1]: the records fo_scene_spawn_rules wrote (read in HBM, never on the host).
 * Point i owns R = max(routes, 1) prediction slots i * R + r of the outputs, which have the layout
 * fo_sweep_set_agents consumes (slots of points >= *d_n_points and unused route slots get len 0):
 *   Pedestrian -> heading = the record's (static-obstacle rule: lanelet heading + 90 deg, spawn_locator.py:459-460) or,
 *     when the record carries none, the unit normal towards a curve (agent.py:475-481): the centre line of the first
 *     lanelet that holds the point for the turn rules (mode 'lane_center'; the ego reference path when the point is on
 *     no lanelet -- the reference's latent None there is not reproduced, Q12), the ego reference path d_path
 *     [n_path][2] otherwise (mode 'ref_path'); straight constant-velocity prediction in slot r = 0 (agent.py:483-505);
 *   Car / Bicycle -> the first lanelet that holds the point; with routes > 0 (fo_scene_set_routes) one prediction per
 *     candidate route of that lanelet (the min-var(v) Frenet sample, see fo_scene_spawn), heading of record = first
 *     segment of route 0; off-lanelet or without a route table: heading towards d_path, one straight prediction.
 * d_pos0 [max_points][2] / d_yaw0 [max_points]: spawn position and initial heading per point (host views read them
 * lazily).
 * A refused list (*d_n_points < 0): every slot is inactive, and d_len[0] -- the first rule slot -- is FO_LEN_REFUSED instead
 * of 0: fo_sweep_set_agents reads that as "this set cannot be judged" and the sweep fails closed ("A refused rule list" at
 * fo_sweep_check); everybody else treats it as 0 live samples. */
int fo_scene_spawn_rule_agents(fo_ctx *ctx, int max_points, const double *d_points, const int32_t *d_n_points, int routes,
                               const fo_rule_agent_types_t *types, int n_path, const double *d_path, int T, double dt,
                               double var0, double var_factor, double *d_pos0, double *d_yaw0, double *d_pos, double *d_yaw,
                               double *d_v, double *d_cov, double *d_shape, double *d_raw_dims, int32_t *d_type,
                               int32_t *d_len, void *stream);

/* ---- one planning step in one call: fo_scene_fan -> fo_scene_visibility -> fo_scene_spawn -> fo_sweep_set_agents ->
 *      fo_sweep_run on one stream, with the arguments of those five entry points (same names, same meaning) in one
 *      structure.  What it replaces is the reference's FOInterface.evaluate_scenario + M x trajectory_safety_assessment
 *      (interface.py:148-219) for a host that calls through an FFI: a planning step of the reference's own size (2 000
 *      candidates x 32 phantoms) is twelve kernel launches of a few microseconds each, and five FFI crossings with
 *      ~90 arguments cost the host more than the GPU needs for the step.  The structure is filled once (every pointer
 *      and size of a planning loop is stable); per step the caller updates the ego pose, the window origin and the
 *      spawn range.  NULL-able members are the NULL-able arguments of the single calls.  Stops at the first failing
 *      stage and returns its code.  Every output buffer ends up with the bits the five calls would have written; the
 *      step itself runs in eight launches instead of twelve (the ray fan is worked out inside the ray kernel, whose spare
 *      workgroups also write the sweep's tile table of the candidates; the sampler's candidate cells are flagged during
 *      the compaction of the occluded cells; the prediction kernel writes its slots' rows of the sweep's agent table).
 *      FO_STEP_STAGES=1 in the environment: the plain stage calls.
 *      With spawn_mode FO_SPAWN_RULES / FO_SPAWN_BOTH the rule families run between the visibility and the sweep:
 *      fo_scene_spawn_rules (two launches) and fo_scene_spawn_rule_agents (one, which also writes its slots' rows of the
 *      agent table) -- the reference's find_spawn_points -> add_agent flow (interface.py:186-198) without leaving HBM.
 *      A step whose rule list is refused (*d_n_rule_points = -1) still returns FO_OK -- nothing is read back -- and fails
 *      closed on the device: d_cost is NaN, d_safe 0, in both forms, also with the cell sampler's agents in the set
 *      (FO_SPAWN_BOTH); d_pair_f / d_pair_i / d_lists are unspecified ("A refused rule list" at fo_sweep_check). */
typedef struct {
  /* fo_scene_fan */
  int32_t n_rays, polygon_footprint;
  double ego_yaw, fov_deg, r;
  double *d_dirs, *d_rmax, *d_half;
  /* fo_scene_visibility (d_dirs / d_rmax / d_half as above) */
  double ego_x, ego_y, head_x, head_y;
  int32_t full_circle, exact_cells, O;
  const uint8_t *d_edge_skip;
  const double *d_ocorn, *d_ocen;
  const uint8_t *d_oflags;
  int32_t win_ix0, win_iy0, win_nx, win_ny;
  double *d_range;
  int32_t *d_hit_id;
  double *d_ring;
  uint8_t *d_obst_vis, *d_cls;
  int32_t *d_occ_idx, *d_n_occ;
  /* fo_scene_spawn (d_cls + window as above; its per-prediction outputs are the agent arrays of the sweep) */
  double min_ahead, max_dist;
  int32_t all_occluded, max_agents, routes, n_path, T_agents;
  int32_t type4[4];
  double speed4[4], raw_l4[4], raw_w4[4], infl_l4[4], infl_w4[4];
  const double *d_path;
  double dt, var0, var_factor;
  int32_t *d_cell;
  double *d_pos0, *d_yaw0;
  int32_t *d_n;
  double *d_pos, *d_yaw, *d_v, *d_cov, *d_shape, *d_raw_dims;
  int32_t *d_type, *d_len;
  /* fo_sweep_set_agents takes max_agents * max(routes, 1) prediction slots from the arrays above; fo_sweep_run: */
  int32_t M, T;
  const double *d_x, *d_y, *d_theta, *d_vel, *d_acc;
  double *d_cost;
  uint8_t *d_safe;
  double *d_pair_f;
  int32_t *d_pair_i;
  double *d_lists;
  /* element type of d_lists for THIS run (FO_LISTS_F64 / FO_LISTS_F32 / FO_LISTS_F32_EXACT); the step sets the context's format to it before
   * the sweep, so a stale fo_sweep_set_list_format of another caller cannot make the kernel write the other width */
  int32_t list_format;
  /* Which spawn stage feeds the sweep (interface.py:186-198).  FO_SPAWN_CELLS: fo_scene_spawn, the build's own sampling in
   * the occluded cells.  FO_SPAWN_RULES: the reference's three rule families, fo_scene_spawn_rules ->
   * fo_scene_spawn_rule_agents, device resident (no read-back, no host add_agent).  FO_SPAWN_BOTH: cells first, then
   * rules.  Slot layout of the prediction arrays d_pos ... d_len: [max_agents * R] cell slots (FO_SPAWN_RULES: none),
   * then [max_rule_points * R] rule slots, R = max(routes, 1); d_pos0 / d_yaw0 hold max_agents (+ max_rule_points)
   * entries the same way. */
  int32_t spawn_mode;
  /* fo_scene_spawn_rules (d_cls + window, obstacles as above; d_oflags then carries the rule bits 2 and 3 as well) and
   * fo_scene_spawn_rule_agents (d_path, T_agents, dt, var0, var_factor, routes as above) */
  int32_t n_path6, max_rule_points;
  const double *d_path6, *d_oyaw, *d_odims;
  fo_spawn_rule_params_t rule;
  fo_rule_agent_types_t rule_types;
  double *d_rule_points;
  int32_t *d_n_rule_points;
  /* ABI 12 -- the step's two host transfers, queued by the step itself (NULL / 0: none; what the reference does on the host
   * around sensor_model.py:41-101 without noticing: its obstacles and its visible-object bookkeeping live in host memory).
   * h_obstacles: the obstacle rows of this step in host memory, any kind (d_ocorn / d_ocen / d_oflags / d_oyaw / d_odims
   * point into d_obstacles); copied into a pinned staging slot of the context and from there to d_obstacles in front of the
   * first launch -- the caller's buffer is free again when fo_step_run returns; at most 64 KB.
   * h_mirror: PINNED, device-mapped host memory (hipHostMalloc / a pinned torch tensor) that receives mirror_bytes from
   * d_mirror by the end of the step (the interface mirrors d_hit_id and d_obst_vis, which it allocates back to back: that
   * pair is stored into the mirror by the kernels that produce it -- posted writes, no copy command; any other region is
   * copied behind the last launch); complete when fo_step_mirror_wait returns.  The next fo_step_run on the same stream
   * overwrites it.  COHERENCE: the direct stores need host-coherent pinned memory -- hipHostMalloc with the default flags
   * (or hipHostMallocCoherent / a pinned torch tensor); the event the wait synchronises on releases to system scope
   * (hipEventReleaseToSystem).  Memory from hipHostMallocNonCoherent or hipHostRegister carries no such guarantee: pass it
   * with FO_STEP_MIRROR_COPY=1 in the environment (the copy command instead of the direct stores) or not at all. */
  const void *h_obstacles;
  void *d_obstacles;
  int64_t obstacles_bytes;
  void *h_mirror;
  const void *d_mirror;
  int64_t mirror_bytes;
} fo_step_t;
enum { FO_SPAWN_CELLS = 0, FO_SPAWN_RULES = 1, FO_SPAWN_BOTH = 2 };
int fo_step_run(fo_ctx *ctx, const fo_step_t *step, void *stream);
/* blocks until the mirror copy of the latest fo_step_run with h_mirror has landed (returns at once when there was none) */
int fo_step_mirror_wait(fo_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
