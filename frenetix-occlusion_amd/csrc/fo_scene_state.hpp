// fo_scene_state.hpp -- what the scene stage keeps between calls: the static map of a scenario (StaticMap, shared by
// reference between contexts) and the per-step workspace of a context (Scene).  Each struct frees its device tables through
// ONE list (free_tables): a new table is added to the struct and to that list, nowhere else.  Part of the one translation
// unit fo_scene.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "fo_ctx.hpp"

namespace {

// groups of a map's device tables, by the call that uploads them (StaticMap::free_tables)
enum : unsigned {
  MAP_GEOMETRY = 1u,         // fo_scene_set_map
  MAP_EDGE_LINES = 2u,       // fo_scene_set_edge_lines
  MAP_LANELET_RASTER = 4u,   // fo_scene_set_routes; a new road raster (fo_scene_set_map) invalidates it
  MAP_ROUTES = 8u,           // fo_scene_set_routes
  MAP_TOPOLOGY = 16u,        // fo_scene_set_topology
  MAP_CENTERLINES = 32u,     // fo_scene_set_centerlines
  MAP_LANE_MOVES = 64u,      // fo_scene_set_lane_moves; a new road raster (fo_scene_set_map) invalidates it
  MAP_ALL = ~0u
};

// the static map of a scenario: uploaded once (fo_scene_set_map / _set_routes / _set_edge_lines), read-only afterwards,
// and shared by reference between the contexts of several egos on one GPU (fo_scene_share_map: BASELINE configs[4],
// "shared occlusion map in HBM")
struct StaticMap {
  std::atomic<int> refs{1};        // contexts reading this map (fo_scene_share_map / fo_destroy may run on other host threads)
  int P = 0, E = 0;
  double cs = 0.5, x0 = 0, y0 = 0;
  int rnx = 0, rny = 0;
  double *d_edges = nullptr;      // [E][4]
  int32_t *d_edge_line = nullptr; // [E] straight-line chain of each piece (optional)
  double *d_chunk_box = nullptr;  // [ceil(E/64)][4] xmin, ymin, xmax, ymax of 64 consecutive pieces
  double *d_sub_box = nullptr;    // [ceil(E/64)][4][4] the same for the four 16-piece quarters of each chunk
  uint8_t *d_raster = nullptr;    // [rny][rnx]
  double *d_lane_yaw = nullptr;   // [rny][rnx] or null
  // phantom vehicle routes (optional): routes r < R of lanelet p = vertices route_first[p*R+r] .. +route_count[p*R+r]
  int R = 0, n_lanelets = 0;
  int32_t *d_route_first = nullptr, *d_route_count = nullptr, *d_lanelet_raster = nullptr;
  double *d_route_xy = nullptr, *d_route_s = nullptr;
  // lanelet polygons as uploaded (exact point-in-lanelet tests of the spawn rule families, fo_spawn_rules.hpp)
  int32_t *d_poly_off = nullptr;  // [P + 1]
  double *d_poly_xy = nullptr;    // [V][2]
  double *d_poly_box = nullptr;   // [P][4] xmin, ymin, xmax, ymax
  // lanelet topology the rule families read (fo_scene_set_topology; optional)
  double *d_left0 = nullptr;      // [P][2] first vertex of the left bound
  int32_t *d_pred0 = nullptr, *d_adj_left = nullptr;   // [P] index of predecessors[0] / adj_left, -1 = none
  int n_inter = 0;
  int32_t *d_inter_off = nullptr, *d_inter_lanelet = nullptr;   // intersection i: entries [off[i], off[i+1]) of
  uint8_t *d_inter_kind = nullptr;                              // (lanelet index, kind: 0 incoming, 1 inner)
  // lanelet centre lines (fo_scene_set_centerlines; optional): vertices center_xy[center_off[p] .. center_off[p+1])
  int32_t *d_center_off = nullptr;
  double *d_center_xy = nullptr;
  // move bytes of the lane flow (fo_scene_set_lane_moves; optional): bit k = step k * 45 degrees may be taken out of the cell
  uint8_t *d_lane_moves = nullptr;   // [rny][rnx] or null

  // frees the tables of the groups in `which` and nulls their pointers: THE list of the map's device tables
  void free_tables(unsigned which = MAP_ALL) {
    const struct { unsigned group; void **p; } tables[] = {
        {MAP_GEOMETRY, (void **)&d_edges},          {MAP_GEOMETRY, (void **)&d_chunk_box},     {MAP_GEOMETRY, (void **)&d_sub_box},
        {MAP_GEOMETRY, (void **)&d_raster},         {MAP_GEOMETRY, (void **)&d_lane_yaw},      {MAP_GEOMETRY, (void **)&d_poly_off},
        {MAP_GEOMETRY, (void **)&d_poly_xy},        {MAP_GEOMETRY, (void **)&d_poly_box},      {MAP_EDGE_LINES, (void **)&d_edge_line},
        {MAP_LANELET_RASTER, (void **)&d_lanelet_raster}, {MAP_ROUTES, (void **)&d_route_first}, {MAP_ROUTES, (void **)&d_route_count},
        {MAP_ROUTES, (void **)&d_route_xy},         {MAP_ROUTES, (void **)&d_route_s},         {MAP_TOPOLOGY, (void **)&d_left0},
        {MAP_TOPOLOGY, (void **)&d_pred0},          {MAP_TOPOLOGY, (void **)&d_adj_left},      {MAP_TOPOLOGY, (void **)&d_inter_off},
        {MAP_TOPOLOGY, (void **)&d_inter_lanelet},  {MAP_TOPOLOGY, (void **)&d_inter_kind},    {MAP_CENTERLINES, (void **)&d_center_off},
        {MAP_CENTERLINES, (void **)&d_center_xy},   {MAP_LANE_MOVES, (void **)&d_lane_moves}};
    for (const auto &t : tables)
      if ((t.group & which) && *t.p) { (void)hipFree(*t.p); *t.p = nullptr; }
  }
};

void map_release(StaticMap *m) {
  if (!m || m->refs.fetch_sub(1) > 1) return;
  m->free_tables();
  delete m;
}

struct Scene {
  StaticMap *map = new StaticMap();
  // per-step workspace
  size_t cap_cand = 0, cap_vis32 = 0;
  int32_t *d_vis32 = nullptr;     // [O] probe results (zero between steps)
  uint8_t *d_flags = nullptr;     // [cells]
  int32_t *d_blk = nullptr;       // block counts / offsets
  size_t cap_cells = 0, cap_blk = 0;
  uint8_t *d_flags2 = nullptr;    // the same pair for the candidate flags a fused step writes during the first compaction
  int32_t *d_blk2 = nullptr;
  size_t cap_cells2 = 0, cap_blk2 = 0;
  bool cand_flags_ready = false;  // d_flags2 / d_blk2 hold this step's candidate flags (set by the fused visibility call)
  int32_t *d_cand = nullptr;      // candidate cell list
  int32_t *d_ncand = nullptr;
  int32_t *d_amb = nullptr;       // [cells] window indices of the cells the fan cannot decide
  int32_t *d_namb = nullptr;      // [1]; zeroed by the ray kernel of the step
  size_t cap_amb = 0;
  double *d_rule_rec = nullptr;   // [1 + O][24] per-workgroup records of the spawn rule families (fo_spawn_rules.hpp)
  size_t cap_rule_rec = 0;
  double shadow_length = 100.0;   // where an obstacle's shadow wedge ends (helper_functions.py:145-146); <= 0 or inf: nowhere
  double *d_ofar = nullptr;       // [O][3] per step: half-plane beyond the end of each obstacle's wedge
  size_t cap_ofar = 0;
  int *d_rule_lab = nullptr, *d_rule_cnt = nullptr;   // dynamic rule: [O][97 x 97] lattice labels, [O] arrival counters
  size_t cap_rule_lab = 0, cap_rule_cnt = 0;
  // occlusion memory (fo_scene_set_occlusion_memory): armed for the next visibility stage only, caller-owned buffers
  bool om_armed = false;
  bool om_road = false;   // the armed call asked for the road metric (fo_scene_set_occlusion_memory_road)
  fo_occlusion_memory_t om{};
  // its vehicle layer (fo_scene_set_occlusion_memory_vehicles): armed on top of an armed main memory, for the same stage only
  bool ov_armed = false;
  fo_occlusion_memory_t ov{};
  // hidden-traffic reach forecast (fo_scene_hidden_reach): row distances of the grown window, allocated by its first call
  uint8_t *d_hr_g = nullptr;
  size_t cap_hr_g = 0;
  uint16_t *d_hr_dist = nullptr;        // ... and the road metric's distance map, when the caller hands in no buffer for it
  size_t cap_hr_dist = 0;

  // THE list of the workspace's device buffers (the context goes away: fo_scene_destroy_)
  void free_tables() {
    void *ptrs[] = {d_vis32, d_flags, d_blk, d_flags2, d_blk2, d_cand, d_ncand, d_amb, d_namb, d_rule_rec, d_rule_lab, d_rule_cnt,
                    d_ofar, d_hr_g, d_hr_dist};
    for (void *p : ptrs)
      if (p) (void)hipFree(p);
  }
};

Scene *scene_of(fo_ctx *ctx) {
  if (!ctx->scene) ctx->scene = new Scene();
  return (Scene *)ctx->scene;
}

int ensure_cells(fo_ctx *ctx, Scene *sc, size_t cells) {
  int rc;
  if ((rc = fo_reserve(ctx, &sc->d_flags, &sc->cap_cells, cells))) return rc;
  const size_t nb = (cells + 255) / 256 + 1;
  if ((rc = fo_reserve(ctx, &sc->d_blk, &sc->cap_blk, nb))) return rc;
  if (!sc->d_ncand) FO_HIP_TRY(ctx, hipMalloc((void **)&sc->d_ncand, sizeof(int32_t)));
  if ((rc = fo_reserve(ctx, &sc->d_amb, &sc->cap_amb, cells))) return rc;
  if (!sc->d_namb) {
    FO_HIP_TRY(ctx, hipMalloc((void **)&sc->d_namb, sizeof(int32_t)));
    FO_HIP_TRY(ctx, hipMemset(sc->d_namb, 0, sizeof(int32_t)));
  }
  return FO_OK;
}

}  // namespace
