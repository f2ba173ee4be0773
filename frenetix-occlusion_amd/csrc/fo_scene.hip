// fo_scene.hip -- visibility ray fan, occluded-cell grid, phantom spawn sampling and constant-velocity predictions
// for gfx950.  Replaces, per planning step, SensorModel.calc_visible_and_occluded_area (ref: sensor_model.py:41-193),
// the cell-based core of SpawnLocator.find_spawn_points (ref: spawn_locator.py:80-139) and the pedestrian-style
// prediction generator (ref: agent.py:451-536).  The reference does this with GEOS polygon algebra (one
// `difference` per boundary vertex); there is no ray or cell in it -- the discretisation is defined in
// DESIGN.md and is the same one oracle/ restates on the CPU.
//
// Compiled with -ffp-contract=off: every integer output (hit ids, cell classes, occluded-cell indices, spawn cells)
// must be bit-identical to the CPU restatement, so only + - * / sqrt and comparisons on float64 are used and no
// FMA is formed.
//
// This file is the scene stage's one translation unit and its host side: the C entry points, their argument checks, the map
// upload and the step chain.  The kernels live in the parts included below, each with its argument structs and, where a kernel
// has forms, the launch helper that picks one; the picking rules are plain functions of integers in fo_scene_plan.hpp.
//
// Kernels (all latency-bound at one ego; launch count matters more than bandwidth here -- eight launches per step):
//   fo_scene_rays.hpp        fo_fan_kernel   ray directions, footprint range per ray, half fan of the occluded area
//                            fo_rays_kernel  ray fan + obstacle-visibility probes in one launch: a workgroup per ray / per probe;
//                                            the boundary pieces come in 64-piece chunks with bounding boxes, culled a lane per
//                                            box; lexicographic (t, id) minimum by cross-lane shuffles = first hit
//   fo_scene_grid.hpp        fo_raster_kernel  one-off: world-aligned road raster (cell centre inside any lanelet polygon)
//                            fo_grid_kernel  one thread per cell: fan sector by binary search on cross products, inside-the-chord
//                                            test, half-fan test -> class bits; cells the fan cannot decide go to a list; also
//                                            the per-block counts of the occluded-cell compaction
//                            fo_settle_kernel  a workgroup per undecided cell (does an occluder cross the segment ego -> centre)
//                                            and a workgroup per obstacle (5 mm skin)
//   fo_scene_compact.hpp     fo_flag_compact_kernel  deterministic stream compaction in one launch (ballot prefix inside a block,
//                                            every block sums the counts before it; fo_flag_scan_kernel / fo_flag_scatter_kernel
//                                            for very large windows); fo_spawn_flag_kernel  candidate cells (+ block counts)
//   fo_spawn_predict.hpp     fo_spawn_predict_kernel  evenly spaced pick + heading + predictions in the sweep's agent layout
//   fo_spawn_rules.hpp       fo_spawn_rules_kernel, fo_spawn_rules_select_kernel, fo_spawn_rule_predict_kernel  the reference's
//                                            three spawn rule families on the cell classes, and their agents (the families and
//                                            what they ask of cells, polygons and frames: fo_rule_*.hpp; fo_rule_plan.hpp: the
//                                            entry's decisions as plain functions of integers)
//   fo_occlusion_memory.hpp  fo_occlusion_memory_kernel  occlusion memory, an extension: one launch between the settlement and
//                                            the compaction when armed (fo_occlusion_memory_road_kernel, the road metric:
//                                            fo_occlusion_memory_road.hpp)
//   fo_occlusion_memory_flow.hpp  fo_occlusion_memory_flow_kernel  its vehicle layer: a second hidden set bound to the lanes'
//                                            driving direction, one more launch behind the memory's when armed
//   fo_future_visibility.hpp fo_future_visibility_kernel  an extension outside the step: what a candidate trajectory comes to see
//   fo_hidden_reach.hpp      fo_hr_*_kernel  hidden-traffic reach forecast, an extension outside the step
//   fo_hidden_reach_road.hpp fo_hr_road_*_kernel  its road metric: distance bands along the road, arrival merge
//   fo_hidden_reach_flow.hpp fo_hr_flow_band_kernel  the road metric bound to the lanes' driving direction: directed distance bands
//   fo_hidden_witness.hpp    fo_hr_witness_kernel  the route behind each candidate's finding: conflict cell, walk back along d
//   fo_hidden_brake.hpp      fo_hr_brake_kernel  brake clearance: follow a candidate until sample b, then brake -- a lane per (m, b)
//   fo_hidden_clearance.hpp  fo_hc_*_kernel  hidden-traffic clearance: the key map behind every reach table, its minimum per pose
//   fo_hidden_brake_classes.hpp  fo_hr_brake_classes_kernel  brake clearance for several hidden-user speeds: one walk over the key map
//   fo_hidden_brake_users.hpp  fo_hr_brake_users_kernel  ... for road users on different forecasts: one walk over up to three key maps
//   fo_hidden_brake_ladder.hpp  fo_hr_brake_ladder_kernel  brake clearance at a ladder of decelerations: a lane per (m, b, level)
//   fo_hidden_brake_ladder_users.hpp  fo_hr_brake_ladder_users_kernel  ... the ladder for road users on different forecasts in one walk
//   fo_hidden_poses.hpp      fo_hidden_poses_kernel  (cos, sin), travelled arc and finite flag of the candidates, on the device
//   fo_hidden_brake_verdict.hpp  fo_hr_brake_verdict_kernel  the fail-safe verdict: the users walk over the first B brake starts,
//                                            folded into the reserved cost columns and the safety flag (fo_hidden_verdict.hpp: the
//                                            fold as plain functions of values)
// State between calls (the static map, the per-step workspace): fo_scene_state.hpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fo_ctx.hpp"
#include "fo_scene_plan.hpp"
#include "fo_scene_state.hpp"
#include "fo_hidden_reach.hpp"
#include "fo_hidden_reach_road.hpp"
#include "fo_hidden_reach_flow.hpp"
#include "fo_hidden_witness.hpp"
#include "fo_hidden_brake.hpp"
#include "fo_hidden_clearance.hpp"
#include "fo_hidden_brake_classes.hpp"
#include "fo_hidden_brake_users.hpp"
#include "fo_hidden_brake_ladder.hpp"
#include "fo_hidden_brake_ladder_users.hpp"
#include "fo_hidden_poses.hpp"
#include "fo_hidden_brake_verdict.hpp"
#include "fo_hidden_brake_ladder_verdict.hpp"
#include "fo_scene_rays.hpp"
#include "fo_scene_grid.hpp"
#include "fo_future_visibility.hpp"
#include "fo_scene_compact.hpp"
#include "fo_spawn_predict.hpp"
#include "fo_occlusion_memory.hpp"
#include "fo_occlusion_memory_flow.hpp"
#include "fo_spawn_rules.hpp"

// (fo_reserve's instantiations are part of the library's dynamic symbols; this one has a single caller, which would inline it away)
template int fo_reserve<uint16_t>(fo_ctx *, uint16_t **, size_t *, size_t);

extern "C" {

void fo_scene_destroy_(fo_ctx *ctx) {
  if (!ctx || !ctx->scene) return;
  Scene *sc = (Scene *)ctx->scene;
  sc->free_tables();
  map_release(sc->map);
  delete sc;
  ctx->scene = nullptr;
}

// Let `ctx` read the static map another context of the same device has uploaded (edge soup, chunk boxes, road and
// lane-heading rasters, route table) instead of holding a copy: several egos planning on one scenario on one GPU
// (BASELINE configs[4]).  The per-step workspace stays per context.  The map is reference counted; a later
// fo_scene_set_map on either context gives that context a map of its own again.
int fo_scene_share_map(fo_ctx *ctx, fo_ctx *owner) {
  if (!ctx || !owner || !owner->scene) return fo_fail(ctx, FO_E_ARG, "fo_scene_share_map: the owner has no map");
  if (ctx->device != owner->device) return fo_fail(ctx, FO_E_ARG, "fo_scene_share_map: contexts live on different devices");
  Scene *dst = scene_of(ctx), *src = (Scene *)owner->scene;
  if (dst->map == src->map) return FO_OK;
  if (src->map->P < 1) return fo_fail(ctx, FO_E_STATE, "fo_scene_share_map: the owner has not called fo_scene_set_map");
  map_release(dst->map);
  dst->map = src->map;
  dst->map->refs.fetch_add(1);
  return FO_OK;
}

int fo_scene_set_map(fo_ctx *ctx, int P, const int32_t *h_poly_off, const double *h_poly_xy, int E,
                     const double *h_edges, double cs, double margin, const double *h_lane_yaw_or_null,
                     const double *h_raster_origin_or_null, const int32_t *h_raster_dims_or_null) {
  if (!ctx) return FO_E_ARG;
  if (P < 1 || !h_poly_off || !h_poly_xy || E < 0 || (E > 0 && !h_edges) || !(cs > 0))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_set_map: bad arguments (P=%d E=%d cs=%g)", P, E, cs);
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  Scene *sc = scene_of(ctx);
  if (sc->map->refs > 1) {  // shared with other contexts: this one gets a map of its own
    map_release(sc->map);
    sc->map = new StaticMap();
  }
  const int V = h_poly_off[P];
  double xmin = INFINITY, ymin = INFINITY, xmax = -INFINITY, ymax = -INFINITY;
  double *pbox = new double[4 * (size_t)P];
  for (int p = 0; p < P; ++p) {
    double bx0 = INFINITY, by0 = INFINITY, bx1 = -INFINITY, by1 = -INFINITY;
    for (int i = h_poly_off[p]; i < h_poly_off[p + 1]; ++i) {
      bx0 = fmin(bx0, h_poly_xy[2 * i]); bx1 = fmax(bx1, h_poly_xy[2 * i]);
      by0 = fmin(by0, h_poly_xy[2 * i + 1]); by1 = fmax(by1, h_poly_xy[2 * i + 1]);
    }
    pbox[4 * p] = bx0; pbox[4 * p + 1] = by0; pbox[4 * p + 2] = bx1; pbox[4 * p + 3] = by1;
    xmin = fmin(xmin, bx0); ymin = fmin(ymin, by0); xmax = fmax(xmax, bx1); ymax = fmax(ymax, by1);
  }
  if (h_raster_origin_or_null && h_raster_dims_or_null) {
    sc->map->x0 = h_raster_origin_or_null[0]; sc->map->y0 = h_raster_origin_or_null[1];
    sc->map->rnx = h_raster_dims_or_null[0]; sc->map->rny = h_raster_dims_or_null[1];
  } else {  // origin snapped to whole cells so that windows of different steps share cell boundaries
    sc->map->x0 = floor((xmin - margin) / cs) * cs;
    sc->map->y0 = floor((ymin - margin) / cs) * cs;
    sc->map->rnx = (int)ceil((xmax + margin - sc->map->x0) / cs);
    sc->map->rny = (int)ceil((ymax + margin - sc->map->y0) / cs);
  }
  if (sc->map->rnx < 1 || sc->map->rny < 1 || (long)sc->map->rnx * sc->map->rny > (1L << 28)) {
    delete[] pbox;
    return fo_fail(ctx, FO_E_ARG, "fo_scene_set_map: raster %d x %d out of range", sc->map->rnx, sc->map->rny);
  }
  sc->map->P = P; sc->map->E = E; sc->map->cs = cs;
  sc->map->R = 0;  // a new raster invalidates the route table
  sc->map->free_tables(MAP_ALL & ~MAP_ROUTES);   // (the route tables wait for the next fo_scene_set_routes)
  int32_t *d_off = nullptr;
  double *d_xy = nullptr, *d_box = nullptr;
  const size_t cells = (size_t)sc->map->rnx * sc->map->rny;
  FO_HIP_TRY(ctx, hipMalloc((void **)&d_off, sizeof(int32_t) * (P + 1)));
  FO_HIP_TRY(ctx, hipMalloc((void **)&d_xy, sizeof(double) * 2 * V));
  FO_HIP_TRY(ctx, hipMalloc((void **)&d_box, sizeof(double) * 4 * P));
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_raster, cells));
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_edges, sizeof(double) * 4 * (size_t)(E > 0 ? E : 1)));
  FO_HIP_TRY(ctx, hipMemcpy(d_off, h_poly_off, sizeof(int32_t) * (P + 1), hipMemcpyHostToDevice));
  FO_HIP_TRY(ctx, hipMemcpy(d_xy, h_poly_xy, sizeof(double) * 2 * V, hipMemcpyHostToDevice));
  FO_HIP_TRY(ctx, hipMemcpy(d_box, pbox, sizeof(double) * 4 * P, hipMemcpyHostToDevice));
  delete[] pbox;
  if (E > 0) FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_edges, h_edges, sizeof(double) * 4 * (size_t)E, hipMemcpyHostToDevice));
  // bounding boxes the scans cull by (tight when the caller's order is spatially coherent): of the 64-piece chunks, and of
  // the four 16-piece quarters of each chunk (empty quarters get an empty box)
  const int nc = (E + SCENE_CHUNK - 1) / SCENE_CHUNK;
  const auto upload_boxes = [&](int per, int count, double **d_box) -> hipError_t {
    double *hb = new double[4 * (size_t)(count > 0 ? count : 1)];
    for (int c = 0; c < count; ++c) {
      double bx0 = INFINITY, by0 = INFINITY, bx1 = -INFINITY, by1 = -INFINITY;
      for (int e = per * c; e < E && e < per * (c + 1); ++e) {
        const double *q = h_edges + 4 * (size_t)e;
        bx0 = fmin(bx0, fmin(q[0], q[2])); bx1 = fmax(bx1, fmax(q[0], q[2]));
        by0 = fmin(by0, fmin(q[1], q[3])); by1 = fmax(by1, fmax(q[1], q[3]));
      }
      hb[4 * c] = bx0; hb[4 * c + 1] = by0; hb[4 * c + 2] = bx1; hb[4 * c + 3] = by1;
    }
    hipError_t e1 = hipMalloc((void **)d_box, sizeof(double) * 4 * (size_t)(count > 0 ? count : 1));
    if (e1 == hipSuccess && count > 0) e1 = hipMemcpy(*d_box, hb, sizeof(double) * 4 * (size_t)count, hipMemcpyHostToDevice);
    delete[] hb;
    return e1;
  };
  FO_HIP_TRY(ctx, upload_boxes(SCENE_CHUNK, nc, &sc->map->d_chunk_box));
  FO_HIP_TRY(ctx, upload_boxes(SCENE_CHUNK / 4, 4 * nc, &sc->map->d_sub_box));
  hipLaunchKernelGGL(fo_raster_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, 0, P, d_off, d_xy, d_box,
                     sc->map->x0, sc->map->y0, cs, sc->map->rnx, sc->map->rny, sc->map->d_raster);
  FO_HIP_TRY(ctx, hipGetLastError());
  FO_HIP_TRY(ctx, hipDeviceSynchronize());
  sc->map->d_poly_off = d_off; sc->map->d_poly_xy = d_xy; sc->map->d_poly_box = d_box;   // kept: the rule families test points against them
  sc->map->n_inter = 0;
  if (h_lane_yaw_or_null) {
    FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_lane_yaw, sizeof(double) * cells));
    FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_lane_yaw, h_lane_yaw_or_null, sizeof(double) * cells, hipMemcpyHostToDevice));
  }
  return FO_OK;
}

int fo_scene_set_routes(fo_ctx *ctx, int P, int R, const int32_t *h_first, const int32_t *h_count, int NV,
                        const double *h_xy, const double *h_s, const int32_t *h_lanelet_raster) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_set_routes: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  if (P < 1 || R < 1 || !h_first || !h_count || NV < 0 || (NV > 0 && (!h_xy || !h_s)) || !h_lanelet_raster)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_set_routes: bad arguments (P=%d R=%d NV=%d)", P, R, NV);
  for (int i = 0; i < P * R; ++i)
    if (h_count[i] < 0 || h_first[i] < 0 || (long)h_first[i] + h_count[i] > NV)
      return fo_fail(ctx, FO_E_ARG, "fo_scene_set_routes: route %d leaves the vertex table", i);
  // the tables belong to the map: while other contexts read it, freeing them here would pull them away under their
  // kernels (and change the route count R for every ego)
  if (sc->map->refs.load() > 1)
    return fo_fail(ctx, FO_E_STATE, "fo_scene_set_routes: the static map is shared (fo_scene_share_map); set the routes on "
                                    "the owner before sharing, or give this context its own map with fo_scene_set_map");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  sc->map->free_tables(MAP_ROUTES | MAP_LANELET_RASTER);
  const size_t cells = (size_t)sc->map->rnx * sc->map->rny, nvs = (size_t)(NV > 0 ? NV : 1);
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_route_first, sizeof(int32_t) * P * R));
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_route_count, sizeof(int32_t) * P * R));
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_lanelet_raster, sizeof(int32_t) * cells));
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_route_xy, sizeof(double) * 2 * nvs));
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_route_s, sizeof(double) * nvs));
  FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_route_first, h_first, sizeof(int32_t) * P * R, hipMemcpyHostToDevice));
  FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_route_count, h_count, sizeof(int32_t) * P * R, hipMemcpyHostToDevice));
  FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_lanelet_raster, h_lanelet_raster, sizeof(int32_t) * cells, hipMemcpyHostToDevice));
  if (NV > 0) {
    FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_route_xy, h_xy, sizeof(double) * 2 * NV, hipMemcpyHostToDevice));
    FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_route_s, h_s, sizeof(double) * NV, hipMemcpyHostToDevice));
  }
  sc->map->R = R;
  sc->map->n_lanelets = P;
  return FO_OK;
}

// the lanelet topology and the centre lines the spawn rule families read (fo_spawn_rules.hpp)
int fo_scene_set_topology(fo_ctx *ctx, int P, const double *h_left0, const int32_t *h_pred0, const int32_t *h_adj_left,
                          int n_inter, const int32_t *h_inter_off, const int32_t *h_inter_lanelet,
                          const uint8_t *h_inter_kind) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_set_topology: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  if (P != sc->map->P || !h_left0 || !h_pred0 || !h_adj_left || n_inter < 0 || (n_inter > 0 && (!h_inter_off || !h_inter_lanelet || !h_inter_kind)))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_set_topology: bad arguments (P=%d, the map has %d lanelets)", P, sc->map->P);
  if (sc->map->refs.load() > 1)
    return fo_fail(ctx, FO_E_STATE, "fo_scene_set_topology: the static map is shared (fo_scene_share_map); set the topology on the owner before sharing");
  for (int p = 0; p < P; ++p)
    if (h_pred0[p] < -1 || h_pred0[p] >= P || h_adj_left[p] < -1 || h_adj_left[p] >= P)
      return fo_fail(ctx, FO_E_ARG, "fo_scene_set_topology: lanelet index out of range at %d", p);
  const int n_e = n_inter > 0 ? h_inter_off[n_inter] : 0;
  for (int e = 0; e < n_e; ++e)
    if (h_inter_lanelet[e] < 0 || h_inter_lanelet[e] >= P) return fo_fail(ctx, FO_E_ARG, "fo_scene_set_topology: intersection entry %d out of range", e);
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  StaticMap *m = sc->map;
  m->free_tables(MAP_TOPOLOGY);
  FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_left0, sizeof(double) * 2 * P));
  FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_pred0, sizeof(int32_t) * P));
  FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_adj_left, sizeof(int32_t) * P));
  FO_HIP_TRY(ctx, hipMemcpy(m->d_left0, h_left0, sizeof(double) * 2 * P, hipMemcpyHostToDevice));
  FO_HIP_TRY(ctx, hipMemcpy(m->d_pred0, h_pred0, sizeof(int32_t) * P, hipMemcpyHostToDevice));
  FO_HIP_TRY(ctx, hipMemcpy(m->d_adj_left, h_adj_left, sizeof(int32_t) * P, hipMemcpyHostToDevice));
  m->n_inter = n_inter;
  if (n_inter > 0) {
    FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_inter_off, sizeof(int32_t) * (n_inter + 1)));
    FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_inter_lanelet, sizeof(int32_t) * (n_e > 0 ? n_e : 1)));
    FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_inter_kind, (size_t)(n_e > 0 ? n_e : 1)));
    FO_HIP_TRY(ctx, hipMemcpy(m->d_inter_off, h_inter_off, sizeof(int32_t) * (n_inter + 1), hipMemcpyHostToDevice));
    if (n_e > 0) {
      FO_HIP_TRY(ctx, hipMemcpy(m->d_inter_lanelet, h_inter_lanelet, sizeof(int32_t) * n_e, hipMemcpyHostToDevice));
      FO_HIP_TRY(ctx, hipMemcpy(m->d_inter_kind, h_inter_kind, (size_t)n_e, hipMemcpyHostToDevice));
    }
  }
  return FO_OK;
}

int fo_scene_set_centerlines(fo_ctx *ctx, int P, const int32_t *h_off, const double *h_xy) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_set_centerlines: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  StaticMap *m = sc->map;
  if (P != m->P || !h_off || h_off[0] != 0) return fo_fail(ctx, FO_E_ARG, "fo_scene_set_centerlines: bad arguments (P=%d, the map has %d lanelets)", P, m->P);
  for (int p = 0; p < P; ++p)
    if (h_off[p + 1] < h_off[p]) return fo_fail(ctx, FO_E_ARG, "fo_scene_set_centerlines: offsets must not decrease (lanelet %d)", p);
  const int NV = h_off[P];
  if (NV > 0 && !h_xy) return fo_fail(ctx, FO_E_ARG, "fo_scene_set_centerlines: null vertex table");
  if (m->refs.load() > 1)
    return fo_fail(ctx, FO_E_STATE, "fo_scene_set_centerlines: the static map is shared (fo_scene_share_map); set the centre lines on the owner before sharing");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  m->free_tables(MAP_CENTERLINES);
  FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_center_off, sizeof(int32_t) * (P + 1)));
  FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_center_xy, sizeof(double) * 2 * (size_t)(NV > 0 ? NV : 1)));
  FO_HIP_TRY(ctx, hipMemcpy(m->d_center_off, h_off, sizeof(int32_t) * (P + 1), hipMemcpyHostToDevice));
  if (NV > 0) FO_HIP_TRY(ctx, hipMemcpy(m->d_center_xy, h_xy, sizeof(double) * 2 * (size_t)NV, hipMemcpyHostToDevice));
  return FO_OK;
}

// the move bytes of the lane flow (fo_hidden_reach_flow.hpp): a table of the map, uploaded by its owner before sharing
int fo_scene_set_lane_moves(fo_ctx *ctx, const uint8_t *h_moves) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_set_lane_moves: call fo_scene_set_map first");
  StaticMap *m = ((Scene *)ctx->scene)->map;
  if (m->P < 1 || !m->d_raster) return fo_fail(ctx, FO_E_STATE, "fo_scene_set_lane_moves: call fo_scene_set_map first");
  if (m->refs.load() > 1)
    return fo_fail(ctx, FO_E_STATE, "fo_scene_set_lane_moves: the static map is shared (fo_scene_share_map); set the move table on the owner before sharing");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  m->free_tables(MAP_LANE_MOVES);
  if (!h_moves) return FO_OK;           // NULL drops the table
  const size_t cells = (size_t)m->rnx * m->rny;
  FO_HIP_TRY(ctx, hipMalloc((void **)&m->d_lane_moves, cells));
  FO_HIP_TRY(ctx, hipMemcpy(m->d_lane_moves, h_moves, cells, hipMemcpyHostToDevice));
  return FO_OK;
}

int fo_scene_set_shadow_length(fo_ctx *ctx, double length) {
  if (!ctx) return FO_E_ARG;
  if (length != length) return fo_fail(ctx, FO_E_ARG, "fo_scene_set_shadow_length: NaN");
  scene_of(ctx)->shadow_length = length;
  return FO_OK;
}

int fo_scene_map_info(fo_ctx *ctx, double *x0, double *y0, double *cs, int *nx, int *ny, int *n_edges) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_map_info: no map set");
  Scene *sc = (Scene *)ctx->scene;
  if (x0) *x0 = sc->map->x0;
  if (y0) *y0 = sc->map->y0;
  if (cs) *cs = sc->map->cs;
  if (nx) *nx = sc->map->rnx;
  if (ny) *ny = sc->map->rny;
  if (n_edges) *n_edges = sc->map->E;
  return FO_OK;
}

int fo_scene_copy_raster(fo_ctx *ctx, uint8_t *h_out) {
  if (!ctx || !ctx->scene || !h_out) return fo_fail(ctx, FO_E_STATE, "fo_scene_copy_raster: no map set");
  Scene *sc = (Scene *)ctx->scene;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  FO_HIP_TRY(ctx, hipMemcpy(h_out, sc->map->d_raster, (size_t)sc->map->rnx * sc->map->rny, hipMemcpyDeviceToHost));
  return FO_OK;
}

int fo_scene_set_edge_lines(fo_ctx *ctx, int E, const int32_t *h_line) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_set_edge_lines: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  if (E != sc->map->E || (E > 0 && !h_line)) return fo_fail(ctx, FO_E_ARG, "fo_scene_set_edge_lines: E must match the map");
  if (sc->map->refs.load() > 1)
    return fo_fail(ctx, FO_E_STATE, "fo_scene_set_edge_lines: the static map is shared (fo_scene_share_map); set the labels "
                                    "on the owner before sharing, or give this context its own map with fo_scene_set_map");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  sc->map->free_tables(MAP_EDGE_LINES);
  if (E == 0) return FO_OK;
  for (int e = 0; e < E; ++e)
    if (h_line[e] < 0 || h_line[e] >= E) return fo_fail(ctx, FO_E_ARG, "fo_scene_set_edge_lines: label out of [0, E)");
  FO_HIP_TRY(ctx, hipMalloc((void **)&sc->map->d_edge_line, sizeof(int32_t) * (size_t)E));
  FO_HIP_TRY(ctx, hipMemcpy(sc->map->d_edge_line, h_line, sizeof(int32_t) * (size_t)E, hipMemcpyHostToDevice));
  return FO_OK;
}

int fo_scene_fan(fo_ctx *ctx, int n_rays, double ego_yaw, double fov_deg, double r, int polygon_footprint,
                 double *d_dirs, double *d_rmax, double *d_half, void *stream) {
  if (!ctx) return FO_E_ARG;
  if (n_rays < 4 || !d_dirs || !(r > 0) || !(fov_deg > 0))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_fan: bad arguments");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int full = fov_deg >= 359.9;
  hipLaunchKernelGGL(fo_fan_kernel, dim3((n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_rays, ego_yaw,
                     fov_deg * (3.14159265358979323846 / 180.0), full, r, polygon_footprint, d_dirs, d_rmax, d_half);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// fo_scene_visibility on the step's own structure (the members fo_step_t lists under fo_scene_visibility); fan / sf / prep
// (fo_step_run): the ray fan of fo_scene_fan inside the ray kernel, the candidate flags of fo_scene_spawn inside the
// compaction, the sweep's tile table in the ray launch -- launches less, the same bits
static int scene_visibility(fo_ctx *ctx, const fo_step_t &p, void *stream, const FanArgs *fan_in, const SpawnFlagArgs *sf_in,
                            const fo_prep_args_t *prep_in) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_visibility: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  const StaticMap *m = sc->map;
  sc->cand_flags_ready = false;
  const bool om_on = sc->om_armed;   // (fo_scene_set_occlusion_memory arms this call only)
  sc->om_armed = false;
  const bool ov_on = om_on && sc->ov_armed;   // (the vehicle layer rides on the main memory of the same stage)
  sc->ov_armed = false;
  const int O = p.O;
  if (p.n_rays < 4 || !p.d_dirs || !p.d_range || !p.d_hit_id || O < 0 || (O > 0 && (!p.d_ocorn || !p.d_ocen || !p.d_oflags)) ||
      p.win_nx < 1 || p.win_ny < 1 || !p.d_cls || !p.d_occ_idx || !p.d_n_occ || !(p.r > 0))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_visibility: bad arguments");
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const bool probes = O > 0 && p.d_obst_vis;
  if (probes && (size_t)O > sc->cap_vis32) {
    if ((rc = fo_reserve(ctx, &sc->d_vis32, &sc->cap_vis32, (size_t)O))) return rc;
    FO_HIP_TRY(ctx, hipMemsetAsync(sc->d_vis32, 0, sizeof(int32_t) * sc->cap_vis32, s));
  }
  const int cells = p.win_nx * p.win_ny;
  if (probes && O > cells) return fo_fail(ctx, FO_E_ARG, "fo_scene_visibility: more obstacles than window cells");
  if (om_on && sc->om.cur_bytes < (int64_t)cells)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_visibility: the occlusion memory's buffer holds %lld bytes, the window %d cells",
                   (long long)sc->om.cur_bytes, cells);
  if (ov_on && sc->ov.cur_bytes < (int64_t)cells)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_visibility: the vehicle layer's buffer holds %lld bytes, the window %d cells",
                   (long long)sc->ov.cur_bytes, cells);
  if (ov_on && !m->d_lane_moves)
    return fo_fail(ctx, FO_E_STATE, "fo_scene_visibility: the vehicle layer is armed and the map has lost its move table");
  if ((rc = ensure_cells(ctx, sc, (size_t)cells))) return rc;
  const FanArgs fan = fan_in ? *fan_in : FanArgs();
  fo_prep_args_t prep = prep_in ? *prep_in : fo_prep_args_t();
  // one wave per ray / probe / undecided cell or five (ray_waves; the knob is looked at on every call); with one, the tile
  // table's spare workgroups take horizon slices of two samples (a lane handles two elements, as in the 256-thread shape)
  const int nw = ray_waves(m->E, O, fo_getenv(fo_env_any("FO_SCENE_"), "FO_SCENE_FIVE_WAVES") != nullptr);
  if (nw == 1 && prep.on) { prep.tz = prep.T > 2 ? 2 : prep.T; prep.nz = (prep.T + prep.tz - 1) / prep.tz; }
  launch_rays(m, p, nw, probes ? sc->d_vis32 : nullptr, sc->d_namb, fan, prep, s);
  // where the obstacles' shadows end: worked out by the grid kernel (a thread per obstacle), read by the settle kernel
  double *far = nullptr;
  if (p.exact_cells && O > 0 && sc->shadow_length > 0.0 && sc->shadow_length < INFINITY) {
    if ((size_t)16 * O > (size_t)(cells + 255) / 256 * 256)
      return fo_fail(ctx, FO_E_ARG, "fo_scene_visibility: more than a sixteenth as many obstacles as window cells");
    if ((rc = fo_reserve(ctx, &sc->d_ofar, &sc->cap_ofar, (size_t)3 * O))) return rc;
    far = sc->d_ofar;
  }
  hipLaunchKernelGGL(fo_grid_kernel, dim3((cells + 255) / 256), dim3(256), 0, s, m->d_raster, m->rnx, m->rny, m->x0, m->y0, m->cs,
                     p.win_ix0, p.win_iy0, p.win_nx, p.win_ny, p.ego_x, p.ego_y, p.head_x, p.head_y, p.r, p.full_circle, p.n_rays, p.d_dirs,
                     p.d_range, p.d_cls, sc->d_flags, sc->d_blk, probes ? O : 0, sc->d_vis32, probes ? p.d_obst_vis : nullptr,
                     p.exact_cells ? 1 : 0, m->E, p.d_hit_id, p.d_rmax, sc->d_amb, sc->d_namb, p.d_half, m->d_edge_line, p.d_ocorn,
                     p.d_oflags, sc->shadow_length, far, O, probes ? fan.vis_host : nullptr);
  if (p.exact_cells) {
    if ((uintptr_t)p.d_cls & 3) return fo_fail(ctx, FO_E_ARG, "fo_scene_visibility: d_cls must be 4-byte aligned");
    launch_settle(m, sc, p, nw, far, s);
  }
  if (om_on) launch_occlusion_memory(sc, p, s);
  if (ov_on) launch_occlusion_memory_flow(sc, p, s);
  FO_HIP_TRY(ctx, hipGetLastError());
  if (!sf_in) return compact(ctx, sc, sc->d_flags, sc->d_blk, cells, p.d_occ_idx, p.d_n_occ, s);
  if ((rc = fo_reserve(ctx, &sc->d_flags2, &sc->cap_cells2, (size_t)cells))) return rc;
  if ((rc = fo_reserve(ctx, &sc->d_blk2, &sc->cap_blk2, (size_t)(cells + 255) / 256 + 1))) return rc;
  SpawnFlagArgs sf = *sf_in;
  sf.on = 1; sf.cls = p.d_cls; sf.nx = p.win_nx; sf.ny = p.win_ny; sf.ix0 = p.win_ix0; sf.iy0 = p.win_iy0;
  sf.rx0 = m->x0; sf.ry0 = m->y0; sf.cs = m->cs; sf.ex = p.ego_x; sf.ey = p.ego_y; sf.hx = p.head_x; sf.hy = p.head_y;
  sf.flag = sc->d_flags2; sf.blk = sc->d_blk2;
  return compact(ctx, sc, sc->d_flags, sc->d_blk, cells, p.d_occ_idx, p.d_n_occ, s, &sf, &sc->cand_flags_ready);
}

int fo_scene_visibility(fo_ctx *ctx, double ego_x, double ego_y, double head_x, double head_y, double r, int full_circle,
                        int exact_cells, int n_rays, const double *d_dirs, const double *d_rmax, const double *d_half,
                        const uint8_t *d_edge_skip, int O, const double *d_ocorn, const double *d_ocen,
                        const uint8_t *d_oflags, int win_ix0, int win_iy0, int win_nx, int win_ny, double *d_range,
                        int32_t *d_hit_id, double *d_ring, uint8_t *d_obst_vis, uint8_t *d_cls, int32_t *d_occ_idx,
                        int32_t *d_n_occ, void *stream) {
  fo_step_t p{};
  p.ego_x = ego_x; p.ego_y = ego_y; p.head_x = head_x; p.head_y = head_y; p.r = r; p.full_circle = full_circle;
  p.exact_cells = exact_cells; p.n_rays = n_rays;
  // (the stage only reads the fan's tables; the step's structure holds them writable for the fused fan)
  p.d_dirs = const_cast<double *>(d_dirs); p.d_rmax = const_cast<double *>(d_rmax); p.d_half = const_cast<double *>(d_half);
  p.d_edge_skip = d_edge_skip; p.O = O; p.d_ocorn = d_ocorn; p.d_ocen = d_ocen; p.d_oflags = d_oflags;
  p.win_ix0 = win_ix0; p.win_iy0 = win_iy0; p.win_nx = win_nx; p.win_ny = win_ny;
  p.d_range = d_range; p.d_hit_id = d_hit_id; p.d_ring = d_ring; p.d_obst_vis = d_obst_vis; p.d_cls = d_cls;
  p.d_occ_idx = d_occ_idx; p.d_n_occ = d_n_occ;
  return scene_visibility(ctx, p, stream, nullptr, nullptr, nullptr);
}

// fo_scene_set_occlusion_memory / _road: the same structure, checks and refusals; the later call decides the metric
static int set_occlusion_memory(fo_ctx *ctx, const fo_occlusion_memory_t *om, bool road, const char *fn) {
  if (!ctx) return FO_E_ARG;
  if (ctx->scene) ((Scene *)ctx->scene)->om_armed = ((Scene *)ctx->scene)->ov_armed = false;   // (a main arming call drops the vehicle layer)
  if (!om) return FO_OK;   // off
  if (!ctx->scene) return fo_fail(ctx, FO_E_STATE, "%s: call fo_scene_set_map first", fn);
  Scene *sc = (Scene *)ctx->scene;
  constexpr int cap = FO_OCCLUSION_MEMORY_MAX_HALO;
  if (om->r2 < 0 || om->r2 > cap * cap)
    return fo_fail(ctx, FO_E_ARG, "%s: r2 = %d outside [0, %d] (a reach of at most %d cells)", fn, om->r2,
                   cap * cap, cap);
  if (!om->d_cur || om->cur_bytes < 1) return fo_fail(ctx, FO_E_ARG, "%s: no buffer for this step", fn);
  if (!om->reset) {
    if (!om->d_prev || om->d_prev == om->d_cur || om->prev_nx < 1 || om->prev_ny < 1)
      return fo_fail(ctx, FO_E_ARG, "%s: the previous step needs a window and a buffer of its own", fn);
    if (om->prev_bytes < (int64_t)om->prev_nx * om->prev_ny)
      return fo_fail(ctx, FO_E_ARG, "%s: the previous buffer holds %lld bytes, its window %d x %d cells",
                     fn, (long long)om->prev_bytes, om->prev_nx, om->prev_ny);
  }
  sc->om = *om;
  sc->om_armed = true;
  sc->om_road = road;
  return FO_OK;
}

int fo_scene_set_occlusion_memory(fo_ctx *ctx, const fo_occlusion_memory_t *om) {
  return set_occlusion_memory(ctx, om, false, "fo_scene_set_occlusion_memory");
}

int fo_scene_set_occlusion_memory_road(fo_ctx *ctx, const fo_occlusion_memory_t *om) {
  return set_occlusion_memory(ctx, om, true, "fo_scene_set_occlusion_memory_road");
}

// the vehicle layer: valid on top of an armed main memory only, and only with the map's move table
int fo_scene_set_occlusion_memory_vehicles(fo_ctx *ctx, const fo_occlusion_memory_t *vm) {
  const char *fn = "fo_scene_set_occlusion_memory_vehicles";
  if (!ctx) return FO_E_ARG;
  if (ctx->scene) ((Scene *)ctx->scene)->ov_armed = false;
  if (!vm) return FO_OK;   // off
  if (!ctx->scene) return fo_fail(ctx, FO_E_STATE, "%s: call fo_scene_set_map first", fn);
  Scene *sc = (Scene *)ctx->scene;
  if (!sc->om_armed)
    return fo_fail(ctx, FO_E_STATE, "%s: arm the main memory of the stage first (fo_scene_set_occlusion_memory or its _road form)", fn);
  if (!sc->map->d_lane_moves) return fo_fail(ctx, FO_E_STATE, "%s: the map has no move table (call fo_scene_set_lane_moves first)", fn);
  constexpr int cap = FO_OCCLUSION_MEMORY_MAX_HALO;
  if (vm->r2 < 0 || vm->r2 > cap * cap)
    return fo_fail(ctx, FO_E_ARG, "%s: r2 = %d outside [0, %d] (a reach of at most %d cells)", fn, vm->r2, cap * cap, cap);
  if ((vm->reset != 0) != (sc->om.reset != 0))
    return fo_fail(ctx, FO_E_ARG, "%s: reset = %d, the main memory's is %d (both sets reset together)", fn, vm->reset, sc->om.reset);
  if (vm->r2 > sc->om.r2)
    return fo_fail(ctx, FO_E_ARG, "%s: r2 = %d above the main memory's %d (V would not stay inside H)", fn, vm->r2, sc->om.r2);
  if (!vm->d_cur || vm->cur_bytes < 1 || vm->d_cur == sc->om.d_cur) return fo_fail(ctx, FO_E_ARG, "%s: no buffer of its own for this step", fn);
  if (!vm->reset) {
    if (!vm->d_prev || vm->d_prev == vm->d_cur || vm->prev_nx < 1 || vm->prev_ny < 1)
      return fo_fail(ctx, FO_E_ARG, "%s: the previous step needs a window and a buffer of its own", fn);
    if (vm->prev_bytes < (int64_t)vm->prev_nx * vm->prev_ny)
      return fo_fail(ctx, FO_E_ARG, "%s: the previous buffer holds %lld bytes, its window %d x %d cells",
                     fn, (long long)vm->prev_bytes, vm->prev_nx, vm->prev_ny);
  }
  sc->ov = *vm;
  sc->ov_armed = true;
  return FO_OK;
}

int fo_scene_future_visibility(fo_ctx *ctx, int M, int T, const double *d_x, const double *d_y, int t_stride, int n_rays,
                               const double *d_dirs, double r, int O, const double *d_ocorn, const uint8_t *d_oflags,
                               const int32_t *d_occ_idx, const int32_t *d_n_occ, int win_ix0, int win_iy0, int win_nx,
                               int32_t *d_revealed, double *d_area, void *stream) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_future_visibility: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  if (M < 0 || T < 1 || !d_x || !d_y || t_stride < 1 || n_rays < 4 || n_rays > FV_THREADS * FV_MAX_RPT || !d_dirs || !(r > 0) || O < 0 ||
      (O > 0 && (!d_ocorn || !d_oflags)) || !d_occ_idx || !d_n_occ || win_nx < 1 || !d_revealed || !d_area)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_future_visibility: bad arguments (4 <= n_rays <= %d)", FV_THREADS * FV_MAX_RPT);
  if (M == 0) return FO_OK;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int K = (T + t_stride - 1) / t_stride;
  // a thread per ray up to 256 rays (the form of rounds 1-5, unchanged), two or three rays per thread beyond
  const FvArgs a{T, t_stride, K, n_rays, d_x, d_y, d_dirs, nullptr, r, sc->map->E, sc->map->d_edges, sc->map->d_sub_box,
                 O, 1, d_ocorn, d_oflags, d_occ_idx, d_n_occ, sc->map->x0, sc->map->y0, sc->map->cs, win_ix0, win_iy0, win_nx,
                 d_revealed, d_area, nullptr, nullptr};
  return launch_future_visibility(ctx, a, M, false, false, 0, stream);
}

int fo_scene_future_visibility_ex(fo_ctx *ctx, const fo_future_visibility_t *p, void *stream) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_future_visibility_ex: call fo_scene_set_map first");
  if (!p) return fo_fail(ctx, FO_E_ARG, "fo_scene_future_visibility_ex: no parameters");
  Scene *sc = (Scene *)ctx->scene;
  if (p->M < 0 || p->T < 1 || !p->d_x || !p->d_y || p->t_stride < 1 || p->n_rays < 4 || p->n_rays > FV_THREADS * FV_MAX_RPT ||
      !p->d_dirs || !(p->r > 0) || p->O < 0 || (p->O > 0 && (!p->d_ocorn || !p->d_oflags)) || !p->d_occ_idx || !p->d_n_occ ||
      p->win_nx < 1 || p->win_ny < 1 || !p->d_revealed || !p->d_area)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_future_visibility_ex: bad arguments (4 <= n_rays <= %d)", FV_THREADS * FV_MAX_RPT);
  if (p->n_slices < 1)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_future_visibility_ex: n_slices = %d (at least one occluder slice)", p->n_slices);
  if (!(p->fov_deg > 0))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_future_visibility_ex: fov_deg must be positive");
  const bool sector = !(p->fov_deg >= 359.9);
  if (sector && !p->d_heading)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_future_visibility_ex: a %.3g deg sector fan needs d_heading", p->fov_deg);
  const bool fs = p->d_revealed_new || p->d_revealed_any;
  const int64_t cells = (int64_t)p->win_nx * p->win_ny;
  if (fs && cells > FO_FUTURE_VISIBILITY_MAX_CELLS)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_future_visibility_ex: first-seen outputs need a window of <= %d cells (%d x %d given)",
                   FO_FUTURE_VISIBILITY_MAX_CELLS, p->win_nx, p->win_ny);
  if (p->M == 0) return FO_OK;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int K = (p->T + p->t_stride - 1) / p->t_stride;
  const FvArgs a{p->T, p->t_stride, K, p->n_rays, p->d_x, p->d_y, p->d_dirs, p->d_heading, p->r, sc->map->E, sc->map->d_edges,
                 sc->map->d_sub_box, p->O, p->n_slices, p->d_ocorn, p->d_oflags, p->d_occ_idx, p->d_n_occ, sc->map->x0,
                 sc->map->y0, sc->map->cs, p->win_ix0, p->win_iy0, p->win_nx, p->d_revealed, p->d_area, p->d_revealed_new,
                 p->d_revealed_any};
  // seen set: whole 1 KB rows for the largest list the window can hold
  const size_t seen_bytes = (size_t)((cells + FV_SEEN_CELLS - 1) / FV_SEEN_CELLS) * FV_THREADS * sizeof(uint32_t);
  return launch_future_visibility(ctx, a, p->M, sector, fs, seen_bytes, stream);
}

// ---- what the reach forecast and the clearance ask alike (fn: the entry's name; every refusal precedes the first device call)
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
  if ((rc = hr_check_table(ctx, p->J, p->h_r2, fn))) return rc;
  if (!p->d_arrival) return fo_fail(ctx, FO_E_ARG, "%s: no buffer for the arrival map (d_arrival is required)", fn);
  if ((rc = hr_check_window(ctx, p->d_cls, p->win_nx, p->win_ny, fn))) return rc;
  if ((rc = hr_check_table_values(ctx, p->J, p->h_r2, fn))) return rc;
  const int h = reach_cells(p->h_r2[p->J - 1]);
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (p->M > 0) {
    if (p->T < 1 || p->T > p->J)
      return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, J = %d] (every sample needs its reach)", fn, p->T, p->J);
    if (!p->d_x || !p->d_y || !p->d_heading)
      return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
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
  if ((rc = hr_check_table(ctx, b.J, b.h_r2, fn))) return rc;
  if (!b.d_arrival || !p->d_dist)
    return fo_fail(ctx, FO_E_ARG, "%s: the maps of the forecast are required (base.d_arrival and d_dist [win_ny][win_nx])", fn);
  if ((rc = hr_check_extent(ctx, b.win_nx, b.win_ny, fn))) return rc;
  if ((rc = hr_check_table_values(ctx, b.J, b.h_r2, fn))) return rc;
  if (b.M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, b.M);
  const int min_cap = witness_min_cap(b.h_r2[b.J - 1]);
  if (p->path_cap < 0 || p->path_cap % 4 != 0 || p->path_cap < min_cap)
    return fo_fail(ctx, FO_E_ARG, "%s: path_cap = %d, a multiple of 4 that is >= isqrt(169 h_r2[J-1]) / 12 = %d is needed "
                   "(FO_HIDDEN_WITNESS_MAX_STEPS = %d always serves)", fn, p->path_cap, min_cap, FO_HIDDEN_WITNESS_MAX_STEPS);
  if (b.M > 0) {
    if (b.T < 1 || b.T > b.J)
      return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, J = %d] (every sample needs its reach)", fn, b.T, b.J);
    if (!b.d_x || !b.d_y || !b.d_heading || !b.d_first)
      return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T], d_heading [M][T][2] and d_first [M] of the forecast are required with M > 0", fn);
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
  if ((rc = hr_check_table(ctx, b.J, b.h_r2, fn))) return rc;
  if (!b.d_arrival)
    return fo_fail(ctx, FO_E_ARG, "%s: the map of the forecast is required (base.d_arrival [win_ny][win_nx])", fn);
  if ((rc = hr_check_extent(ctx, b.win_nx, b.win_ny, fn))) return rc;
  if ((rc = hr_check_table_values(ctx, b.J, b.h_r2, fn))) return rc;
  if (b.M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, b.M);
  if (!(p->a_brake >= 0.0) || !std::isfinite(p->a_brake))      // (NaN fails every comparison)
    return fo_fail(ctx, FO_E_ARG, "%s: a_brake = %g, a finite deceleration >= 0 is needed", fn, p->a_brake);
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, p->dt);
  if (b.M > 0) {
    if (b.T < 1 || b.T > b.J)
      return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, J = %d] (every sample needs its reach)", fn, b.T, b.J);
    if (!b.d_x || !b.d_y || !b.d_heading || !b.d_first)
      return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T], d_heading [M][T][2] and d_first [M] of the forecast are required with M > 0", fn);
    if (!p->d_v || !p->d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
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
    if (!p->d_x || !p->d_y || !p->d_heading)
      return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
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
  if (p->C < 1 || p->C > FO_HIDDEN_BRAKE_MAX_CLASSES)
    return fo_fail(ctx, FO_E_ARG, "%s: C = %d outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = %d]", fn, p->C, FO_HIDDEN_BRAKE_MAX_CLASSES);
  if (!p->h_thr) return fo_fail(ctx, FO_E_ARG, "%s: no threshold table h_thr [C][T]", fn);
  if ((rc = hr_check_extent(ctx, p->win_nx, p->win_ny, fn))) return rc;
  if (p->r2_cap < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap = %d is negative", fn, p->r2_cap);
  if ((rc = hr_check_halo(ctx, p->r2_cap, "r2_cap", "v_cap", fn))) return rc;
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (!(p->a_brake >= 0.0) || !std::isfinite(p->a_brake))      // (NaN fails every comparison)
    return fo_fail(ctx, FO_E_ARG, "%s: a_brake = %g, a finite deceleration >= 0 is needed", fn, p->a_brake);
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, p->dt);
  if (p->M == 0) return FO_OK;
  const int T = p->T, C = p->C;
  if (T < 1 || T > HR_MAX_J) return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, %d]", fn, T, HR_MAX_J);
  if (C * T > FO_HIDDEN_BRAKE_MAX_TABLE)
    return fo_fail(ctx, FO_E_ARG, "%s: C * T = %d * %d = %d entries, the table is a kernel argument of at most "
                   "FO_HIDDEN_BRAKE_MAX_TABLE = %d", fn, C, T, C * T, FO_HIDDEN_BRAKE_MAX_TABLE);
  const int64_t cap = (int64_t)169 * p->r2_cap;
  for (int c = 0; c < C; ++c) {
    const int32_t *row = p->h_thr + (size_t)c * T;
    if (row[0] < 0) return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][0] = %d is negative", fn, c, row[0]);
    for (int j = 1; j < T; ++j)
      if (row[j] < row[j - 1])
        return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d] decreases at entry %d (%d after %d)", fn, c, j, row[j], row[j - 1]);
    if (row[T - 1] > cap)
      return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][T-1] = %d lies beyond 169 r2_cap = %lld (the key map ends at the cap)", fn, c,
                     row[T - 1], (long long)cap);
  }
  if (!p->d_x || !p->d_y || !p->d_heading)
    return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
  if (!p->d_key || !p->d_qmin)
    return fo_fail(ctx, FO_E_ARG, "%s: d_key [win_ny][win_nx] and d_qmin [M][T] of the clearance are required with M > 0", fn);
  if (!p->d_v || !p->d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
  if (!p->d_brake_first || !p->d_stop || !p->d_commit || !p->d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_brake_first [C][M][T], d_stop [M][T], d_commit and d_first [C][M] are required with M > 0", fn);
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const HrBrakeClassesArgs a{p->M, T, brake_group(T), C, p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb,
                             sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0,
                             p->win_iy0, p->win_nx, p->win_ny, p->d_key, p->d_qmin, p->d_v, p->d_arc, p->a_brake, p->dt,
                             p->d_brake_first, p->d_stop, p->d_commit, p->d_first};
  HbThr thr;
  for (int t = 0; t < FO_HIDDEN_BRAKE_MAX_TABLE; ++t) thr.v[t] = t < C * T ? p->h_thr[t] : 0;
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
  if (p->K < 1 || p->K > FO_HIDDEN_BRAKE_MAX_MAPS)
    return fo_fail(ctx, FO_E_ARG, "%s: K = %d outside [1, FO_HIDDEN_BRAKE_MAX_MAPS = %d]", fn, p->K, FO_HIDDEN_BRAKE_MAX_MAPS);
  if (p->C < 1 || p->C > FO_HIDDEN_BRAKE_MAX_CLASSES)
    return fo_fail(ctx, FO_E_ARG, "%s: C = %d outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = %d]", fn, p->C, FO_HIDDEN_BRAKE_MAX_CLASSES);
  if (!p->h_thr) return fo_fail(ctx, FO_E_ARG, "%s: no threshold table h_thr [C][T]", fn);
  if ((rc = hr_check_extent(ctx, p->win_nx, p->win_ny, fn))) return rc;
  const int K = p->K, C = p->C;
  for (int k = 0; k < K; ++k) {
    if (p->r2_cap[k] < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap[%d] = %d is negative", fn, k, p->r2_cap[k]);
    static const char *const names[FO_HIDDEN_BRAKE_MAX_MAPS] = {"r2_cap[0]", "r2_cap[1]", "r2_cap[2]"};
    if ((rc = hr_check_halo(ctx, p->r2_cap[k], names[k], "v_cap", fn))) return rc;
  }
  for (int c = 0; c < C; ++c)
    if (p->map_of[c] < 0 || p->map_of[c] >= K)
      return fo_fail(ctx, FO_E_ARG, "%s: map_of[%d] = %d outside [0, K = %d)", fn, c, p->map_of[c], K);
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (!(p->a_brake >= 0.0) || !std::isfinite(p->a_brake))      // (NaN fails every comparison)
    return fo_fail(ctx, FO_E_ARG, "%s: a_brake = %g, a finite deceleration >= 0 is needed", fn, p->a_brake);
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, p->dt);
  if (p->M == 0) return FO_OK;
  const int T = p->T;
  if (T < 1 || T > HR_MAX_J) return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, %d]", fn, T, HR_MAX_J);
  if (C * T > FO_HIDDEN_BRAKE_MAX_TABLE)
    return fo_fail(ctx, FO_E_ARG, "%s: C * T = %d * %d = %d entries, the table is a kernel argument of at most "
                   "FO_HIDDEN_BRAKE_MAX_TABLE = %d", fn, C, T, C * T, FO_HIDDEN_BRAKE_MAX_TABLE);
  for (int c = 0; c < C; ++c) {
    const int32_t *row = p->h_thr + (size_t)c * T;
    const int64_t cap = (int64_t)169 * p->r2_cap[p->map_of[c]];
    if (row[0] < 0) return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][0] = %d is negative", fn, c, row[0]);
    for (int j = 1; j < T; ++j)
      if (row[j] < row[j - 1])
        return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d] decreases at entry %d (%d after %d)", fn, c, j, row[j], row[j - 1]);
    if (row[T - 1] > cap)
      return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][T-1] = %d lies beyond 169 r2_cap[%d] = %lld (the key map of class %d ends at its cap)",
                     fn, c, row[T - 1], p->map_of[c], (long long)cap, c);
  }
  if (!p->d_x || !p->d_y || !p->d_heading)
    return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
  for (int k = 0; k < K; ++k)
    if (!p->d_key[k] || !p->d_qmin[k])
      return fo_fail(ctx, FO_E_ARG, "%s: d_key[%d] [win_ny][win_nx] and d_qmin[%d] [M][T] of clearance %d are required with M > 0", fn,
                     k, k, k);
  if (!p->d_v || !p->d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
  if (!p->d_brake_first || !p->d_stop || !p->d_commit || !p->d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_brake_first [C][M][T], d_stop [M][T], d_commit and d_first [C][M] are required with M > 0", fn);
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  HrBrakeUsersArgs a{p->M, T, brake_group(T), C, p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb,
                     sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0,
                     p->win_iy0, p->win_nx, p->win_ny, p->d_key[0], K > 1 ? p->d_key[1] : nullptr, K > 2 ? p->d_key[2] : nullptr, p->d_qmin[0],
                     K > 1 ? p->d_qmin[1] : nullptr, K > 2 ? p->d_qmin[2] : nullptr, 0u, p->d_v, p->d_arc, p->a_brake, p->dt,
                     p->d_brake_first, p->d_stop, p->d_commit, p->d_first};
  for (int c = 0; c < C; ++c) a.map_of |= (uint32_t)p->map_of[c] << (2 * c);
  HbThr thr;
  for (int t = 0; t < FO_HIDDEN_BRAKE_MAX_TABLE; ++t) thr.v[t] = t < C * T ? p->h_thr[t] : 0;
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
  if ((rc = hr_check_table(ctx, b.J, b.h_r2, fn))) return rc;
  if (!b.d_arrival)
    return fo_fail(ctx, FO_E_ARG, "%s: the map of the forecast is required (base.d_arrival [win_ny][win_nx])", fn);
  if ((rc = hr_check_extent(ctx, b.win_nx, b.win_ny, fn))) return rc;
  if ((rc = hr_check_table_values(ctx, b.J, b.h_r2, fn))) return rc;
  if (b.M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, b.M);
  if (p->K < 1 || p->K > FO_HIDDEN_BRAKE_MAX_LEVELS)
    return fo_fail(ctx, FO_E_ARG, "%s: K = %d outside [1, FO_HIDDEN_BRAKE_MAX_LEVELS = %d]", fn, p->K, FO_HIDDEN_BRAKE_MAX_LEVELS);
  if (!p->h_levels) return fo_fail(ctx, FO_E_ARG, "%s: no decelerations h_levels [K]", fn);
  for (int k = 0; k < p->K; ++k)
    if (!(p->h_levels[k] >= 0.0) || !std::isfinite(p->h_levels[k]))      // (NaN fails every comparison)
      return fo_fail(ctx, FO_E_ARG, "%s: h_levels[%d] = %g, a finite deceleration >= 0 is needed", fn, k, p->h_levels[k]);
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, p->dt);
  if (b.M > 0) {
    if (b.T < 1 || b.T > b.J)
      return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, J = %d] (every sample needs its reach)", fn, b.T, b.J);
    if (p->B < 1 || p->B > b.T) return fo_fail(ctx, FO_E_ARG, "%s: B = %d outside [1, T = %d]", fn, p->B, b.T);
    if (!b.d_x || !b.d_y || !b.d_heading || !b.d_first)
      return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T], d_heading [M][T][2] and d_first [M] of the forecast are required with M > 0", fn);
    if (!p->d_v || !p->d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
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
  if (p->K < 1 || p->K > FO_HIDDEN_BRAKE_MAX_MAPS)
    return fo_fail(ctx, FO_E_ARG, "%s: K = %d outside [1, FO_HIDDEN_BRAKE_MAX_MAPS = %d]", fn, p->K, FO_HIDDEN_BRAKE_MAX_MAPS);
  if (p->C < 1 || p->C > FO_HIDDEN_BRAKE_MAX_CLASSES)
    return fo_fail(ctx, FO_E_ARG, "%s: C = %d outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = %d]", fn, p->C, FO_HIDDEN_BRAKE_MAX_CLASSES);
  if (!p->h_thr) return fo_fail(ctx, FO_E_ARG, "%s: no threshold table h_thr [C][T]", fn);
  if ((rc = hr_check_extent(ctx, p->win_nx, p->win_ny, fn))) return rc;
  const int K = p->K, C = p->C;
  for (int k = 0; k < K; ++k) {
    if (p->r2_cap[k] < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap[%d] = %d is negative", fn, k, p->r2_cap[k]);
    static const char *const names[FO_HIDDEN_BRAKE_MAX_MAPS] = {"r2_cap[0]", "r2_cap[1]", "r2_cap[2]"};
    if ((rc = hr_check_halo(ctx, p->r2_cap[k], names[k], "v_cap", fn))) return rc;
  }
  for (int c = 0; c < C; ++c)
    if (p->map_of[c] < 0 || p->map_of[c] >= K)
      return fo_fail(ctx, FO_E_ARG, "%s: map_of[%d] = %d outside [0, K = %d)", fn, c, p->map_of[c], K);
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (p->L < 1 || p->L > FO_HIDDEN_BRAKE_MAX_LEVELS)
    return fo_fail(ctx, FO_E_ARG, "%s: L = %d outside [1, FO_HIDDEN_BRAKE_MAX_LEVELS = %d]", fn, p->L, FO_HIDDEN_BRAKE_MAX_LEVELS);
  if (!p->h_levels) return fo_fail(ctx, FO_E_ARG, "%s: no decelerations h_levels [L]", fn);
  const int L = p->L;
  for (int l = 0; l < L; ++l)
    if (!(p->h_levels[l] >= 0.0) || !std::isfinite(p->h_levels[l]))      // (NaN fails every comparison)
      return fo_fail(ctx, FO_E_ARG, "%s: h_levels[%d] = %g, a finite deceleration >= 0 is needed", fn, l, p->h_levels[l]);
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, p->dt);
  if (p->M == 0) return FO_OK;
  const int T = p->T, B = p->B;
  if (T < 1 || T > HR_MAX_J) return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, %d]", fn, T, HR_MAX_J);
  if (B < 1 || B > T) return fo_fail(ctx, FO_E_ARG, "%s: B = %d outside [1, T = %d]", fn, B, T);
  if (C * T > FO_HIDDEN_BRAKE_MAX_TABLE)
    return fo_fail(ctx, FO_E_ARG, "%s: C * T = %d * %d = %d entries, the table is a kernel argument of at most "
                   "FO_HIDDEN_BRAKE_MAX_TABLE = %d", fn, C, T, C * T, FO_HIDDEN_BRAKE_MAX_TABLE);
  if (4 * C * T + 8 * L > FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES)
    return fo_fail(ctx, FO_E_ARG, "%s: %d thresholds (C * T = %d * %d) and %d levels take 4 * %d + 8 * %d = %d bytes, they travel as a "
                   "kernel argument of at most FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES = %d", fn, C * T, C, T, L, C * T, L,
                   4 * C * T + 8 * L, FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES);
  for (int c = 0; c < C; ++c) {
    const int32_t *row = p->h_thr + (size_t)c * T;
    const int64_t cap = (int64_t)169 * p->r2_cap[p->map_of[c]];
    if (row[0] < 0) return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][0] = %d is negative", fn, c, row[0]);
    for (int j = 1; j < T; ++j)
      if (row[j] < row[j - 1])
        return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d] decreases at entry %d (%d after %d)", fn, c, j, row[j], row[j - 1]);
    if (row[T - 1] > cap)
      return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][T-1] = %d lies beyond 169 r2_cap[%d] = %lld (the key map of class %d ends at its cap)",
                     fn, c, row[T - 1], p->map_of[c], (long long)cap, c);
  }
  if (!p->d_x || !p->d_y || !p->d_heading)
    return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
  for (int k = 0; k < K; ++k)
    if (!p->d_key[k] || !p->d_qmin[k])
      return fo_fail(ctx, FO_E_ARG, "%s: d_key[%d] [win_ny][win_nx] and d_qmin[%d] [M][T] of clearance %d are required with M > 0", fn,
                     k, k, k);
  if (!p->d_v || !p->d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
  if (!p->d_required || !p->d_last_unclear || !p->d_commit || !p->d_first || !p->d_required_all || !p->d_last_unclear_all || !p->d_blocking)
    return fo_fail(ctx, FO_E_ARG, "%s: d_required, d_last_unclear [C][M][B], d_commit [C][M][L], d_first [C][M], d_required_all, "
                   "d_last_unclear_all and d_blocking [M][B] are required with M > 0", fn);
  if (!p->d_brake_first_or_null != !p->d_stop_or_null)
    return fo_fail(ctx, FO_E_ARG, "%s: the detail d_brake_first_or_null [C][M][B][L] and d_stop_or_null [M][B][L] is given whole or not "
                   "at all (%s is missing)", fn, p->d_stop_or_null ? "d_brake_first_or_null" : "d_stop_or_null");
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  HrBrakeLadderUsersArgs a{p->M, T, B, L, C, brake_ladder_users_width(L), brake_ladder_users_group(T, K, L, B), p->d_x, p->d_y, p->d_heading,
                           p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx,
                           sc->map->rny, p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, p->d_key[0], K > 1 ? p->d_key[1] : nullptr,
                           K > 2 ? p->d_key[2] : nullptr, p->d_qmin[0], K > 1 ? p->d_qmin[1] : nullptr, K > 2 ? p->d_qmin[2] : nullptr, 0u,
                           p->d_v, p->d_arc, p->dt, p->d_required, p->d_last_unclear, p->d_commit, p->d_first, p->d_required_all,
                           p->d_last_unclear_all, p->d_blocking, p->d_brake_first_or_null, p->d_stop_or_null};
  for (int c = 0; c < C; ++c) a.map_of |= (uint32_t)p->map_of[c] << (2 * c);
  HbluPack pk;
  memset(pk.w, 0, sizeof pk.w);
  memcpy(pk.w, p->h_levels, (size_t)L * sizeof(double));        // (little endian: low word first)
  memcpy(pk.w + 2 * L, p->h_thr, (size_t)C * T * sizeof(int32_t));
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
  if (p->T < 1 || p->T > HR_MAX_J) return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, %d]", fn, p->T, HR_MAX_J);
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
  if (p->K < 1 || p->K > FO_HIDDEN_BRAKE_MAX_MAPS)
    return fo_fail(ctx, FO_E_ARG, "%s: K = %d outside [1, FO_HIDDEN_BRAKE_MAX_MAPS = %d]", fn, p->K, FO_HIDDEN_BRAKE_MAX_MAPS);
  if (p->C < 1 || p->C > FO_HIDDEN_BRAKE_MAX_CLASSES)
    return fo_fail(ctx, FO_E_ARG, "%s: C = %d outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = %d]", fn, p->C, FO_HIDDEN_BRAKE_MAX_CLASSES);
  if (!p->h_thr) return fo_fail(ctx, FO_E_ARG, "%s: no threshold table h_thr [C][T]", fn);
  if ((rc = hr_check_extent(ctx, p->win_nx, p->win_ny, fn))) return rc;
  const int K = p->K, C = p->C;
  for (int k = 0; k < K; ++k) {
    if (p->r2_cap[k] < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap[%d] = %d is negative", fn, k, p->r2_cap[k]);
    static const char *const names[FO_HIDDEN_BRAKE_MAX_MAPS] = {"r2_cap[0]", "r2_cap[1]", "r2_cap[2]"};
    if ((rc = hr_check_halo(ctx, p->r2_cap[k], names[k], "v_cap", fn))) return rc;
  }
  for (int c = 0; c < C; ++c)
    if (p->map_of[c] < 0 || p->map_of[c] >= K)
      return fo_fail(ctx, FO_E_ARG, "%s: map_of[%d] = %d outside [0, K = %d)", fn, c, p->map_of[c], K);
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (!(p->a_brake >= 0.0) || !std::isfinite(p->a_brake))      // (NaN fails every comparison)
    return fo_fail(ctx, FO_E_ARG, "%s: a_brake = %g, a finite deceleration >= 0 is needed", fn, p->a_brake);
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, p->dt);
  if (p->M == 0) return FO_OK;
  const int T = p->T, B = p->B;
  if (T < 1 || T > HR_MAX_J) return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, %d]", fn, T, HR_MAX_J);
  if (B < 1 || B > T) return fo_fail(ctx, FO_E_ARG, "%s: B = %d outside [1, T = %d]", fn, B, T);
  if (p->commit_min < 0 || p->commit_min > B)
    return fo_fail(ctx, FO_E_ARG, "%s: commit_min = %d outside [0, B = %d]", fn, p->commit_min, B);
  if (C * T > FO_HIDDEN_BRAKE_MAX_TABLE)
    return fo_fail(ctx, FO_E_ARG, "%s: C * T = %d * %d = %d entries, the table is a kernel argument of at most "
                   "FO_HIDDEN_BRAKE_MAX_TABLE = %d", fn, C, T, C * T, FO_HIDDEN_BRAKE_MAX_TABLE);
  for (int c = 0; c < C; ++c) {
    const int32_t *row = p->h_thr + (size_t)c * T;
    const int64_t cap = (int64_t)169 * p->r2_cap[p->map_of[c]];
    if (row[0] < 0) return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][0] = %d is negative", fn, c, row[0]);
    for (int j = 1; j < T; ++j)
      if (row[j] < row[j - 1])
        return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d] decreases at entry %d (%d after %d)", fn, c, j, row[j], row[j - 1]);
    if (row[T - 1] > cap)
      return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][T-1] = %d lies beyond 169 r2_cap[%d] = %lld (the key map of class %d ends at its cap)",
                     fn, c, row[T - 1], p->map_of[c], (long long)cap, c);
  }
  if (!p->d_x || !p->d_y || !p->d_heading)
    return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
  for (int k = 0; k < K; ++k)
    if (!p->d_key[k] || !p->d_qmin[k])
      return fo_fail(ctx, FO_E_ARG, "%s: d_key[%d] [win_ny][win_nx] and d_qmin[%d] [M][T] of clearance %d are required with M > 0", fn,
                     k, k, k);
  if (!p->d_v || !p->d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
  if (!p->d_fail_safe || !p->d_user || !p->d_commit || !p->d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_fail_safe, d_user [M], d_commit and d_first [C][M] are required with M > 0", fn);
  if (!p->d_cost_or_null != !p->d_safe_or_null)
    return fo_fail(ctx, FO_E_ARG, "%s: d_cost_or_null [M][FO_NC] and d_safe_or_null [M] go together (%s is missing)", fn,
                   p->d_safe_or_null ? "d_cost_or_null" : "d_safe_or_null");
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  HrBrakeVerdictArgs a{p->M, T, brake_verdict_group(B), brake_verdict_per_block(T, K, B), C, B, p->commit_min, p->d_x, p->d_y, p->d_heading,
                       p->d_len_or_null, p->hl, p->hw, p->wb, sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx,
                       sc->map->rny, p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, p->d_key[0], K > 1 ? p->d_key[1] : nullptr,
                       K > 2 ? p->d_key[2] : nullptr, p->d_qmin[0], K > 1 ? p->d_qmin[1] : nullptr, K > 2 ? p->d_qmin[2] : nullptr, 0u,
                       p->d_v, p->d_arc, p->a_brake, p->dt, p->d_finite_or_null, p->d_cost_or_null, p->d_safe_or_null, p->d_fail_safe,
                       p->d_user, p->d_commit, p->d_first};
  for (int c = 0; c < C; ++c) a.map_of |= (uint32_t)p->map_of[c] << (2 * c);
  HbThr thr;
  for (int t = 0; t < FO_HIDDEN_BRAKE_MAX_TABLE; ++t) thr.v[t] = t < C * T ? p->h_thr[t] : 0;
  const dim3 grid((unsigned)brake_verdict_blocks(p->M, T, K, B)), block(HB_THREADS);
  const size_t lds = brake_verdict_lds_bytes(T, K, C, B);
  hipStream_t s = (hipStream_t)stream;
  if (brake_users_width(C) == 4) hbv_launch<4>(K, grid, block, lds, s, a, thr);
  else hbv_launch<8>(K, grid, block, lds, s, a, thr);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// the ladder verdict of every trajectory over its first B brake starts against every class of road user on the key map it names --
// the level the worst start needs, folded into the reserved cost columns and the safety flag: one launch
// (fo_hidden_brake_ladder_verdict.hpp); the levels, map_of and the table travel as kernel arguments
int fo_scene_hidden_brake_ladder_verdict(fo_ctx *ctx, const fo_hidden_brake_ladder_verdict_t *p, void *stream) {
  const char *fn = "fo_scene_hidden_brake_ladder_verdict";
  int rc;
  if ((rc = hr_check_scene(ctx, p, fn))) return rc;
  Scene *sc = (Scene *)ctx->scene;
  if (p->K < 1 || p->K > FO_HIDDEN_BRAKE_MAX_MAPS)
    return fo_fail(ctx, FO_E_ARG, "%s: K = %d outside [1, FO_HIDDEN_BRAKE_MAX_MAPS = %d]", fn, p->K, FO_HIDDEN_BRAKE_MAX_MAPS);
  if (p->C < 1 || p->C > FO_HIDDEN_BRAKE_MAX_CLASSES)
    return fo_fail(ctx, FO_E_ARG, "%s: C = %d outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = %d]", fn, p->C, FO_HIDDEN_BRAKE_MAX_CLASSES);
  if (!p->h_thr) return fo_fail(ctx, FO_E_ARG, "%s: no threshold table h_thr [C][T]", fn);
  if ((rc = hr_check_extent(ctx, p->win_nx, p->win_ny, fn))) return rc;
  const int K = p->K, C = p->C;
  for (int k = 0; k < K; ++k) {
    if (p->r2_cap[k] < 0) return fo_fail(ctx, FO_E_ARG, "%s: r2_cap[%d] = %d is negative", fn, k, p->r2_cap[k]);
    static const char *const names[FO_HIDDEN_BRAKE_MAX_MAPS] = {"r2_cap[0]", "r2_cap[1]", "r2_cap[2]"};
    if ((rc = hr_check_halo(ctx, p->r2_cap[k], names[k], "v_cap", fn))) return rc;
  }
  for (int c = 0; c < C; ++c)
    if (p->map_of[c] < 0 || p->map_of[c] >= K)
      return fo_fail(ctx, FO_E_ARG, "%s: map_of[%d] = %d outside [0, K = %d)", fn, c, p->map_of[c], K);
  if (p->M < 0) return fo_fail(ctx, FO_E_ARG, "%s: M = %d", fn, p->M);
  if (p->L < 1 || p->L > FO_HIDDEN_BRAKE_MAX_LEVELS)
    return fo_fail(ctx, FO_E_ARG, "%s: L = %d outside [1, FO_HIDDEN_BRAKE_MAX_LEVELS = %d]", fn, p->L, FO_HIDDEN_BRAKE_MAX_LEVELS);
  if (!p->h_levels) return fo_fail(ctx, FO_E_ARG, "%s: no decelerations h_levels [L]", fn);
  const int L = p->L;
  for (int l = 0; l < L; ++l)
    if (!(p->h_levels[l] >= 0.0) || !std::isfinite(p->h_levels[l]))      // (NaN fails every comparison)
      return fo_fail(ctx, FO_E_ARG, "%s: h_levels[%d] = %g, a finite deceleration >= 0 is needed", fn, l, p->h_levels[l]);
  for (int l = 1; l < L; ++l)
    if (!(p->h_levels[l] > p->h_levels[l - 1]))
      return fo_fail(ctx, FO_E_ARG, "%s: h_levels[%d] = %g after %g: the levels must be strictly ascending (the answer is the gentlest "
                     "sufficient one)", fn, l, p->h_levels[l], p->h_levels[l - 1]);
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fo_fail(ctx, FO_E_ARG, "%s: dt = %g, a finite step > 0 is needed", fn, p->dt);
  if (!(p->a_limit >= 0.0))                                      // (NaN fails the comparison; +inf passes)
    return fo_fail(ctx, FO_E_ARG, "%s: a_limit = %g, a deceleration >= 0 (or +inf) is needed", fn, p->a_limit);
  if (p->M == 0) return FO_OK;
  const int T = p->T, B = p->B;
  if (T < 1 || T > HR_MAX_J) return fo_fail(ctx, FO_E_ARG, "%s: T = %d outside [1, %d]", fn, T, HR_MAX_J);
  if (B < 1 || B > T) return fo_fail(ctx, FO_E_ARG, "%s: B = %d outside [1, T = %d]", fn, B, T);
  if (C * T > FO_HIDDEN_BRAKE_MAX_TABLE)
    return fo_fail(ctx, FO_E_ARG, "%s: C * T = %d * %d = %d entries, the table is a kernel argument of at most "
                   "FO_HIDDEN_BRAKE_MAX_TABLE = %d", fn, C, T, C * T, FO_HIDDEN_BRAKE_MAX_TABLE);
  if (4 * C * T + 8 * L > FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES)
    return fo_fail(ctx, FO_E_ARG, "%s: %d thresholds (C * T = %d * %d) and %d levels take 4 * %d + 8 * %d = %d bytes, they travel as a "
                   "kernel argument of at most FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES = %d", fn, C * T, C, T, L, C * T, L,
                   4 * C * T + 8 * L, FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES);
  for (int c = 0; c < C; ++c) {
    const int32_t *row = p->h_thr + (size_t)c * T;
    const int64_t cap = (int64_t)169 * p->r2_cap[p->map_of[c]];
    if (row[0] < 0) return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][0] = %d is negative", fn, c, row[0]);
    for (int j = 1; j < T; ++j)
      if (row[j] < row[j - 1])
        return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d] decreases at entry %d (%d after %d)", fn, c, j, row[j], row[j - 1]);
    if (row[T - 1] > cap)
      return fo_fail(ctx, FO_E_ARG, "%s: h_thr[%d][T-1] = %d lies beyond 169 r2_cap[%d] = %lld (the key map of class %d ends at its cap)",
                     fn, c, row[T - 1], p->map_of[c], (long long)cap, c);
  }
  if (!p->d_x || !p->d_y || !p->d_heading)
    return fo_fail(ctx, FO_E_ARG, "%s: d_x, d_y [M][T] and d_heading [M][T][2] are required with M > 0", fn);
  for (int k = 0; k < K; ++k)
    if (!p->d_key[k] || !p->d_qmin[k])
      return fo_fail(ctx, FO_E_ARG, "%s: d_key[%d] [win_ny][win_nx] and d_qmin[%d] [M][T] of clearance %d are required with M > 0", fn,
                     k, k, k);
  if (!p->d_v || !p->d_arc) return fo_fail(ctx, FO_E_ARG, "%s: d_v and d_arc [M][T] are required with M > 0", fn);
  if (!p->d_need || !p->d_at || !p->d_blocking || !p->d_user || !p->d_decel || !p->d_need_of || !p->d_first)
    return fo_fail(ctx, FO_E_ARG, "%s: d_need, d_at, d_blocking, d_user, d_decel [M], d_need_of and d_first [C][M] are required with M > 0", fn);
  if (!p->d_cost_or_null != !p->d_safe_or_null)
    return fo_fail(ctx, FO_E_ARG, "%s: d_cost_or_null [M][FO_NC] and d_safe_or_null [M] go together (%s is missing)", fn,
                   p->d_safe_or_null ? "d_cost_or_null" : "d_safe_or_null");
  if ((rc = hr_check_footprint(ctx, p->hl, p->hw, p->wb, fn))) return rc;
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  HrBrakeLadderVerdictArgs a{p->M, T, B, L, C, brake_ladder_users_width(L), brake_ladder_verdict_group(L, B),
                             brake_ladder_verdict_per_block(T, K, L, B), p->d_x, p->d_y, p->d_heading, p->d_len_or_null, p->hl, p->hw, p->wb,
                             sc->map->x0, sc->map->y0, sc->map->cs, sc->map->d_raster, sc->map->rnx, sc->map->rny, p->win_ix0, p->win_iy0,
                             p->win_nx, p->win_ny, p->d_key[0], K > 1 ? p->d_key[1] : nullptr, K > 2 ? p->d_key[2] : nullptr, p->d_qmin[0],
                             K > 1 ? p->d_qmin[1] : nullptr, K > 2 ? p->d_qmin[2] : nullptr, 0u, p->d_v, p->d_arc, p->dt, p->a_limit,
                             p->d_finite_or_null, p->d_cost_or_null, p->d_safe_or_null, p->d_need, p->d_at, p->d_blocking, p->d_user,
                             p->d_decel, p->d_need_of, p->d_first};
  for (int c = 0; c < C; ++c) a.map_of |= (uint32_t)p->map_of[c] << (2 * c);
  HbluPack pk;
  memset(pk.w, 0, sizeof pk.w);
  memcpy(pk.w, p->h_levels, (size_t)L * sizeof(double));        // (little endian: low word first)
  memcpy(pk.w + 2 * L, p->h_thr, (size_t)C * T * sizeof(int32_t));
  const dim3 grid((unsigned)brake_ladder_verdict_blocks(p->M, T, K, L, B)), block(HB_THREADS);
  const size_t lds = brake_ladder_verdict_lds_bytes(T, K, C, L, B);
  hipStream_t s = (hipStream_t)stream;
  if (brake_users_width(C) == 4) hblv_launch<4>(K, grid, block, lds, s, a, pk);
  else hblv_launch<8>(K, grid, block, lds, s, a, pk);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// fo_scene_spawn on the step's own structure (the members fo_step_t lists under fo_scene_spawn); at (fo_step_run): the
// prediction kernel also writes its slots' rows of the sweep's agent table, and the candidate flags may already be there
// (scene_visibility with sf)
static int scene_spawn(fo_ctx *ctx, const fo_step_t &p, void *stream, const fo_agent_table_t *at) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  const StaticMap *m = sc->map;
  if (!p.d_cls || p.max_agents < 1 || p.n_path < 2 || !p.d_path || p.T_agents < 1 || !p.d_cell || !p.d_pos0 || !p.d_yaw0 || !p.d_n ||
      !p.d_pos || !p.d_yaw || !p.d_v || !p.d_cov || !p.d_shape || !p.d_raw_dims || !p.d_type || !p.d_len)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn: bad arguments");
  const int routes = p.routes;
  if (routes < 0 || (routes > 0 && !m->d_lanelet_raster))
    return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn: routes = %d needs fo_scene_set_routes first", routes);
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  const int cells = p.win_nx * p.win_ny;
  int rc;
  if ((rc = ensure_cells(ctx, sc, (size_t)cells))) return rc;
  if ((rc = fo_reserve(ctx, &sc->d_cand, &sc->cap_cand, (size_t)cells))) return rc;
  if (at && sc->cand_flags_ready) {   // flagged during the compaction of the visibility stage
    sc->cand_flags_ready = false;
    if ((rc = compact(ctx, sc, sc->d_flags2, sc->d_blk2, cells, sc->d_cand, sc->d_ncand, s))) return rc;
  } else {
    SpawnFlagArgs sf;
    sf.on = 1; sf.cls = p.d_cls; sf.nx = p.win_nx; sf.ny = p.win_ny; sf.ix0 = p.win_ix0; sf.iy0 = p.win_iy0;
    sf.all_occluded = p.all_occluded ? 1 : 0;
    sf.rx0 = m->x0; sf.ry0 = m->y0; sf.cs = m->cs; sf.ex = p.ego_x; sf.ey = p.ego_y; sf.hx = p.head_x; sf.hy = p.head_y;
    sf.min_ahead = p.min_ahead; sf.max_dist = p.max_dist; sf.flag = sc->d_flags; sf.blk = sc->d_blk;
    hipLaunchKernelGGL(fo_spawn_flag_kernel, dim3((cells + 255) / 256), dim3(256), 0, s, sf);
    if ((rc = compact(ctx, sc, sc->d_flags, sc->d_blk, cells, sc->d_cand, sc->d_ncand, s))) return rc;
  }
  SpawnTypes st;
  for (int i = 0; i < 4; ++i) {
    st.type[i] = p.type4[i]; st.speed[i] = p.speed4[i]; st.raw_l[i] = p.raw_l4[i]; st.raw_w[i] = p.raw_w4[i];
    st.infl_l[i] = p.infl_l4[i]; st.infl_w[i] = p.infl_w4[i];
  }
  const int R = routes > 0 ? routes : 1;
  RouteView rv;
  if (routes > 0) { rv.RT = m->R; rv.first = m->d_route_first; rv.count = m->d_route_count; rv.xy = m->d_route_xy; rv.s = m->d_route_s; }
  PredOut po{p.d_pos, p.d_yaw, p.d_v, p.d_cov, p.d_shape, p.d_raw_dims, p.d_type, p.d_len};
  hipLaunchKernelGGL(fo_spawn_predict_kernel, dim3(p.max_agents * R), dim3(64), 0, s, p.max_agents, R, sc->d_cand, sc->d_ncand, m->x0,
                     m->y0, m->cs, p.n_path, p.d_path, m->d_lane_yaw, st, p.T_agents, p.dt, p.var0, p.var_factor, p.win_nx, p.win_ix0,
                     p.win_iy0, m->rnx, m->rny, routes > 0 ? m->d_lanelet_raster : nullptr, rv, p.d_cell, p.d_pos0, p.d_yaw0, p.d_n, po,
                     at ? 1 : 0, at ? *at : fo_agent_table_t());
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

int fo_scene_spawn(fo_ctx *ctx, const uint8_t *d_cls, int win_ix0, int win_iy0, int win_nx, int win_ny, double ego_x,
                   double ego_y, double head_x, double head_y, double min_ahead, double max_dist, int all_occluded,
                   int max_agents, int routes, const int32_t *type4, const double *speed4, const double *raw_l4, const double *raw_w4,
                   const double *infl_l4, const double *infl_w4, int n_path, const double *d_path, int T, double dt,
                   double var0, double var_factor, int32_t *d_cell, double *d_pos0, double *d_yaw0, int32_t *d_n,
                   double *d_pos, double *d_yaw, double *d_v, double *d_cov, double *d_shape, double *d_raw_dims,
                   int32_t *d_type, int32_t *d_len, void *stream) {
  // (the step's structure holds the four type slots by value: a missing table is refused here, after the state as ever)
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn: call fo_scene_set_map first");
  if (!type4 || !speed4 || !raw_l4 || !raw_w4 || !infl_l4 || !infl_w4) return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn: bad arguments");
  fo_step_t p{};
  p.d_cls = const_cast<uint8_t *>(d_cls);   // (read only by this stage)
  p.win_ix0 = win_ix0; p.win_iy0 = win_iy0; p.win_nx = win_nx; p.win_ny = win_ny;
  p.ego_x = ego_x; p.ego_y = ego_y; p.head_x = head_x; p.head_y = head_y; p.min_ahead = min_ahead; p.max_dist = max_dist;
  p.all_occluded = all_occluded; p.max_agents = max_agents; p.routes = routes;
  for (int i = 0; i < 4; ++i) {
    p.type4[i] = type4[i]; p.speed4[i] = speed4[i]; p.raw_l4[i] = raw_l4[i]; p.raw_w4[i] = raw_w4[i];
    p.infl_l4[i] = infl_l4[i]; p.infl_w4[i] = infl_w4[i];
  }
  p.n_path = n_path; p.d_path = d_path; p.T_agents = T; p.dt = dt; p.var0 = var0; p.var_factor = var_factor;
  p.d_cell = d_cell; p.d_pos0 = d_pos0; p.d_yaw0 = d_yaw0; p.d_n = d_n; p.d_pos = d_pos; p.d_yaw = d_yaw; p.d_v = d_v; p.d_cov = d_cov;
  p.d_shape = d_shape; p.d_raw_dims = d_raw_dims; p.d_type = d_type; p.d_len = d_len;
  return scene_spawn(ctx, p, stream, nullptr);
}

// ---- the spawn rule families (fo_spawn_rules.hpp; the decisions below: fo_rule_plan.hpp)
// the static map's side of a RuleView (raster, lane headings, lanelet polygons, topology); the caller adds the step's window of
// classes and the frame table
static RuleView rule_view_of(const StaticMap *m) {
  RuleView v{};
  v.x0 = m->x0; v.y0 = m->y0; v.cs = m->cs; v.lane_yaw = m->d_lane_yaw; v.rnx = m->rnx; v.rny = m->rny;
  v.P = m->P; v.poly_off = m->d_poly_off; v.poly_xy = m->d_poly_xy; v.poly_box = m->d_poly_box;
  v.left0 = m->d_left0; v.pred0 = m->d_pred0; v.adj_left = m->d_adj_left;
  v.n_inter = m->n_inter; v.inter_off = m->d_inter_off; v.inter_lanelet = m->d_inter_lanelet; v.inter_kind = m->d_inter_kind;
  return v;
}

// (label_nodes: an environment switch, set by the entry)
static RuleParams rule_params_of(const fo_spawn_rule_params_t &p) {
  RuleParams pr{};
  pr.ego_x = p.ego_x; pr.ego_y = p.ego_y; pr.ego_yaw = p.ego_yaw; pr.ego_s = p.ego_s; pr.ego_d = p.ego_d;
  pr.s_threshold = p.s_threshold; pr.ped_width = p.ped_width; pr.ped_length = p.ped_length;
  pr.intention = p.intention; pr.win_i0 = p.win_i0; pr.win_i1 = p.win_i1;
  pr.behind_static = p.behind_static; pr.behind_turn = p.behind_turn; pr.behind_dynamic = p.behind_dynamic;
  pr.max_static = p.max_static; pr.max_dynamic = p.max_dynamic;
  return pr;
}

int fo_scene_spawn_rules(fo_ctx *ctx, const uint8_t *d_cls, int win_ix0, int win_iy0, int win_nx, int win_ny, int n_path,
                         const double *d_path6, int O, const double *d_ocorn, const double *d_ocen, const double *d_oyaw,
                         const double *d_odims, const uint8_t *d_oflags, const uint8_t *d_obst_vis,
                         const fo_spawn_rule_params_t *params, int max_out, double *d_out, int32_t *d_n_out, void *stream) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn_rules: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  StaticMap *m = sc->map;
  if (!d_cls || !params || !d_out || !d_n_out || max_out < 1 || win_nx < 1 || win_ny < 1 || n_path < 2 || !d_path6 || O < 0 ||
      (O > 0 && (!d_ocorn || !d_ocen || !d_oyaw || !d_odims || !d_oflags || !d_obst_vis)))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: bad arguments (n_path=%d O=%d max_out=%d)", n_path, O, max_out);
  if (!m->d_poly_off) return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn_rules: the map holds no lanelet polygons");
  if (params->win_i0 < 0 || params->win_i1 > n_path || params->win_i1 < params->win_i0)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: reference window [%d, %d) outside the path", params->win_i0, params->win_i1);
  if (params->frame != 0 && params->frame != 1)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: frame = %d (0 the polyline frame, 1 the caller's frame)", params->frame);
  // table space the host can see (what only the device can -- a sampled line longer than RL_MAXSAMP cells / 8 -- comes back as
  // *d_n_out = -1): a rule that ran short would leave out a point the reference finds, unnoticed
  const int nw = params->win_i1 - params->win_i0;
  const bool dynamic_on = rule_dynamic_on(params->behind_dynamic, params->intention);
  if (rule_turn_window_over(params->behind_turn, params->intention, nw))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: the reference window holds %d path vertices, the turn rule %d "
                   "(thin the path out: the window is 40 m)", nw, RL_TURNW);
  if (rule_max_static_over(params->behind_static, params->max_static))
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: max_static = %d, the selection compares the pedestrians of at most %d obstacles", params->max_static, RL_MAXPED);
  if (dynamic_on) {
    if (rule_lanelets_over(m->P))
      return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: %d lanelets, the dynamic-obstacle rule holds flags for %d", m->P, RL_LAT * RL_LAT);
    if (rule_fifth_over(nw))
      return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: the reference window holds %d path vertices, the dynamic-obstacle rule "
                     "asks every fifth of at most %d", nw, 5 * RL_FIFTHV);
  }
  const int can = rule_capacity(params->behind_dynamic, params->max_dynamic, params->behind_static, params->max_static, params->behind_turn);
  if (max_out < can)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rules: max_out = %d cannot hold the %d spawn points max_dynamic = %d / "
                   "max_static = %d allow", max_out, can, params->max_dynamic, params->max_static);
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = fo_reserve(ctx, &sc->d_rule_rec, &sc->cap_rule_rec, (size_t)(O + 1) * RL_REC))) return rc;
  RuleView v = rule_view_of(m);
  v.cls = d_cls; v.ix0 = win_ix0; v.iy0 = win_iy0; v.nx = win_nx; v.ny = win_ny;
  v.path = d_path6; v.n_path = n_path; v.frame = params->frame;
  RuleParams pr = rule_params_of(*params);
  {  // (looked at on every call, like the other knobs: a test runs both labelling forms in one process)
    const char *e = fo_getenv(fo_env_any("FO_SCENE_"), "FO_SCENE_RULE_NODES");
    pr.label_nodes = e && e[0] == '1';
  }
  {  // lattice hand-off of the dynamic rule: [O][97 x 97] labels + a counter per obstacle (zero between launches)
    const size_t cap0 = sc->cap_rule_cnt;
    if ((rc = fo_reserve(ctx, &sc->d_rule_lab, &sc->cap_rule_lab, (size_t)(O > 0 ? O : 1) * RL_LAT * RL_LAT))) return rc;
    if ((rc = fo_reserve(ctx, &sc->d_rule_cnt, &sc->cap_rule_cnt, (size_t)(O > 0 ? O : 1)))) return rc;
    if (sc->cap_rule_cnt != cap0) FO_HIP_TRY(ctx, hipMemsetAsync(sc->d_rule_cnt, 0, sc->cap_rule_cnt * sizeof(int), s));
  }
  const int n_dyn = rule_helped(params->n_dynamic_plus1, O, dynamic_on);
  hipLaunchKernelGGL(fo_spawn_rules_kernel, dim3(rule_grid(O, n_dyn)), dim3(RL_THREADS), 0, s, v, pr, O, d_ocorn, d_ocen, d_oyaw,
                     d_odims, d_oflags, d_obst_vis, sc->d_rule_rec, sc->d_rule_lab, sc->d_rule_cnt, rule_told(params->n_dynamic_plus1) ? 0 : 1,
                     n_dyn);
  hipLaunchKernelGGL(fo_spawn_rules_select_kernel, dim3(1), dim3(64), 0, s, v, pr, O, d_ocorn, d_oflags, d_obst_vis,
                     sc->d_rule_rec, max_out, d_out, d_n_out);
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

// fo_scene_spawn_rule_agents; slot0 / agent0 / at (fo_step_run): the rule agents' slots follow the cell sampler's in the
// same arrays, and the kernel writes its slots' rows of the sweep's agent table
int fo_scene_rule_agents_(fo_ctx *ctx, int max_points, const double *d_points, const int32_t *d_n_points, int routes,
                          const fo_rule_agent_types_t *types, int n_path, const double *d_path, int T, double dt, double var0,
                          double var_factor, int slot0, int agent0, double *d_pos0, double *d_yaw0, double *d_pos, double *d_yaw,
                          double *d_v, double *d_cov, double *d_shape, double *d_raw_dims, int32_t *d_type, int32_t *d_len,
                          void *stream, const fo_agent_table_t *at) {
  if (!ctx || !ctx->scene) return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn_rule_agents: call fo_scene_set_map first");
  Scene *sc = (Scene *)ctx->scene;
  StaticMap *m = sc->map;
  if (max_points < 1 || !d_points || !d_n_points || !types || n_path < 2 || !d_path || T < 1 || !d_pos0 || !d_yaw0 || !d_pos ||
      !d_yaw || !d_v || !d_cov || !d_shape || !d_raw_dims || !d_type || !d_len || slot0 < 0 || agent0 < 0)
    return fo_fail(ctx, FO_E_ARG, "fo_scene_spawn_rule_agents: bad arguments (max_points=%d n_path=%d T=%d)", max_points, n_path, T);
  if (!m->d_poly_off) return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn_rule_agents: the map holds no lanelet polygons");
  if (routes < 0 || (routes > 0 && !m->d_route_first))
    return fo_fail(ctx, FO_E_STATE, "fo_scene_spawn_rule_agents: routes = %d needs fo_scene_set_routes first", routes);
  FO_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const RuleView v = rule_view_of(m);   // (no window of classes, no frame table: the kernel asks the lanelet polygons only)
  RuleAgentTypes ty;
  for (int i = 0; i < 3; ++i) {
    ty.speed[i] = types->speed[i]; ty.raw_l[i] = types->raw_l[i]; ty.raw_w[i] = types->raw_w[i];
    ty.infl_l[i] = types->infl_l[i]; ty.infl_w[i] = types->infl_w[i];
  }
  RouteView rv;
  if (routes > 0) { rv.RT = m->R; rv.first = m->d_route_first; rv.count = m->d_route_count; rv.xy = m->d_route_xy; rv.s = m->d_route_s; }
  const int R = routes > 0 ? routes : 1;
  PredOut po{d_pos, d_yaw, d_v, d_cov, d_shape, d_raw_dims, d_type, d_len};
  hipLaunchKernelGGL(fo_spawn_rule_predict_kernel, dim3(max_points * R), dim3(64), 0, (hipStream_t)stream, v, max_points, d_points,
                     d_n_points, R, ty, n_path, d_path, m->d_center_off, m->d_center_xy, rv, T, dt, var0, var_factor, slot0, agent0,
                     d_pos0, d_yaw0, po, at ? 1 : 0, at ? *at : fo_agent_table_t());
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

int fo_scene_spawn_rule_agents(fo_ctx *ctx, int max_points, const double *d_points, const int32_t *d_n_points, int routes,
                               const fo_rule_agent_types_t *types, int n_path, const double *d_path, int T, double dt,
                               double var0, double var_factor, double *d_pos0, double *d_yaw0, double *d_pos, double *d_yaw,
                               double *d_v, double *d_cov, double *d_shape, double *d_raw_dims, int32_t *d_type,
                               int32_t *d_len, void *stream) {
  return fo_scene_rule_agents_(ctx, max_points, d_points, d_n_points, routes, types, n_path, d_path, T, dt, var0, var_factor, 0, 0,
                               d_pos0, d_yaw0, d_pos, d_yaw, d_v, d_cov, d_shape, d_raw_dims, d_type, d_len, stream, nullptr);
}

// h_mirror as a device pointer if the kernels can fill it themselves (see FanArgs::hit_host), else null (fo_api.hip copies)
void *fo_step_direct_mirror_(fo_ctx *ctx, const fo_step_t *p) {
  if (!p->h_mirror || !p->d_mirror || p->O < 1 || !p->d_obst_vis) return nullptr;
  if (p->d_mirror != (const void *)p->d_hit_id || (const uint8_t *)p->d_obst_vis != (const uint8_t *)p->d_hit_id + sizeof(int32_t) * (size_t)p->n_rays ||
      p->mirror_bytes != (int64_t)(sizeof(int32_t) * (size_t)p->n_rays + (size_t)p->O))
    return nullptr;
  // (FO_STEP_MIRROR_COPY=1: the copy command instead, for A/B runs and the test that compares the two paths -- looked at on
  // every call like the other knobs, fo_ctx.hpp)
  const char *e = fo_getenv(fo_env_any("FO_STEP_"), "FO_STEP_MIRROR_COPY");
  if (e && e[0] == '1') return nullptr;
  // the device-side address of the pinned block, cached by (address, size): a block freed and registered again at the same
  // address with another size is another mapping
  if (ctx->mirror_host != p->h_mirror || ctx->mirror_bytes != p->mirror_bytes) {
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, p->h_mirror, 0) != hipSuccess) { (void)hipGetLastError(); d = nullptr; }
    ctx->mirror_host = p->h_mirror;
    ctx->mirror_bytes = p->mirror_bytes;
    ctx->mirror_dev = d;
  }
  return ctx->mirror_dev;
}

// the scene stages of a planning step in their fused form (fo_step_run, fo_api.hip): fan inside the ray kernel, candidate
// flags inside the first compaction, the sweep's agent table written by the prediction kernels
int fo_scene_step_(fo_ctx *ctx, const fo_step_t *p, const fo_agent_table_t *at, const fo_prep_args_t *prep, void *stream) {
  if (!ctx || !p) return FO_E_ARG;
  if (p->n_rays < 4 || !p->d_dirs || !(p->r > 0) || !(p->fov_deg > 0)) return fo_fail(ctx, FO_E_ARG, "fo_scene_fan: bad arguments");
  const bool cells = p->spawn_mode != FO_SPAWN_RULES, rules = p->spawn_mode != FO_SPAWN_CELLS;
  FanArgs fan;
  fan.on = 1; fan.full = p->fov_deg >= 359.9; fan.polygon = p->polygon_footprint; fan.yaw = p->ego_yaw;
  fan.fov = p->fov_deg * (3.14159265358979323846 / 180.0);
  fan.dirs = p->d_dirs; fan.rmax = p->d_rmax; fan.half = p->d_half;
  // the step's mirror, when it is exactly the pair (hit ids | visibility flags) the interface allocates back to back: stored
  // by the kernels themselves (fo_api.hip then only records the event behind the step)
  if (void *hm = fo_step_direct_mirror_(ctx, p)) {
    fan.hit_host = (int32_t *)hm;
    fan.vis_host = (uint8_t *)hm + sizeof(int32_t) * (size_t)p->n_rays;
  }
  SpawnFlagArgs sf;
  sf.all_occluded = p->all_occluded ? 1 : 0; sf.min_ahead = p->min_ahead; sf.max_dist = p->max_dist;
  int rc;
  if ((rc = scene_visibility(ctx, *p, stream, &fan, cells ? &sf : nullptr, prep))) return rc;
  if (cells && (rc = scene_spawn(ctx, *p, stream, at))) return rc;
  if (rules) {
    const int R = p->routes > 0 ? p->routes : 1, cell_agents = cells ? p->max_agents : 0;
    if ((rc = fo_scene_spawn_rules(ctx, p->d_cls, p->win_ix0, p->win_iy0, p->win_nx, p->win_ny, p->n_path6, p->d_path6, p->O, p->d_ocorn,
                                   p->d_ocen, p->d_oyaw, p->d_odims, p->d_oflags, p->d_obst_vis, &p->rule, p->max_rule_points,
                                   p->d_rule_points, p->d_n_rule_points, stream))) return rc;
    if ((rc = fo_scene_rule_agents_(ctx, p->max_rule_points, p->d_rule_points, p->d_n_rule_points, p->routes, &p->rule_types, p->n_path,
                                    p->d_path, p->T_agents, p->dt, p->var0, p->var_factor, cell_agents * R, cell_agents, p->d_pos0,
                                    p->d_yaw0, p->d_pos, p->d_yaw, p->d_v, p->d_cov, p->d_shape, p->d_raw_dims, p->d_type, p->d_len,
                                    stream, at))) return rc;
  }
  return FO_OK;
}

#if FO_PRED_TRACE
int fo_debug_pred_ticks(long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pred_ticks), sizeof(long long) * 16); }
int fo_debug_ray_ticks(long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ray_ticks), sizeof(long long) * 16); }
#endif

int fo_scene_candidate_count(fo_ctx *ctx, int32_t *h_n, void *stream) {
  if (!ctx || !ctx->scene || !h_n) return FO_E_ARG;
  Scene *sc = (Scene *)ctx->scene;
  FO_HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
  FO_HIP_TRY(ctx, hipMemcpy(h_n, sc->d_ncand, sizeof(int32_t), hipMemcpyDeviceToHost));
  return FO_OK;
}

}  // extern "C"
