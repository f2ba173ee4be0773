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
//   fo_hidden_brake_impact.hpp  fo_hr_brake_impact_kernel  the impact verdict: the same walk, keeping the speed the ego has left at
//                                            the hit; the worst harm over the classes folded likewise (fo_hidden_impact.hpp: the harm
//                                            rows, the choice and the fold as plain functions of values)
//   fo_hidden_brake_ladder_verdict.hpp  fo_hr_brake_ladder_verdict_kernel  the ladder verdict: the ladder-users walk over the first B
//                                            brake starts, reduced to the level the worst start needs and folded likewise
//                                            (fo_hidden_ladder_verdict.hpp: the reduction and the fold as plain functions of values)
//   fo_hidden_brake_harm_ladder.hpp  fo_hr_brake_harm_ladder_kernel  the harm ladder: the ladder verdict with "unclear" relaxed to "hit
//                                            at a harm above the limit", and the greatest harm each level leaves
//                                            (fo_hidden_harm_ladder.hpp: what is over and the curve as plain functions of values)
//   fo_hidden_brake_harm_ladder_lanes.hpp  fo_hr_brake_harm_ladder_lanes_kernel  the harm ladder by approach angle: every hit of a
//                                            lane-bound class priced in the walk's hit hook at the cosine the move table allows
// The host side of the hidden-traffic extensions -- the fo_scene_hidden_* entry points and their argument checks -- is a part too:
// fo_scene_hidden.hpp, behind the kernel parts.
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
#include "fo_hidden_brake_impact.hpp"
#include "fo_hidden_brake_impact_lanes.hpp"
#include "fo_hidden_brake_ladder_verdict.hpp"
#include "fo_hidden_brake_harm_ladder.hpp"
#include "fo_hidden_brake_harm_ladder_lanes.hpp"
#include "fo_scene_rays.hpp"
#include "fo_scene_grid.hpp"
#include "fo_future_visibility.hpp"
#include "fo_scene_compact.hpp"
#include "fo_spawn_predict.hpp"
#include "fo_occlusion_memory.hpp"
#include "fo_occlusion_memory_flow.hpp"
#include "fo_spawn_rules.hpp"
#include "fo_scene_hidden.hpp"

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
