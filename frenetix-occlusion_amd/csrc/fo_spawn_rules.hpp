// fo_spawn_rules.hpp -- the reference's three spawn rule families on the per-step cell classes, on the device.
// Included by fo_scene.hip with the other parts of the scene stage (one translation unit: the kernels read the static map of
// fo_scene_state.hpp, the rule agents share the prediction slot of fo_spawn_predict.hpp), compiled with -ffp-contract=off like
// the rest of the scene stage.  This file: the rule kernel (which workgroup runs which family), the selection kernel, the rule
// agents' prediction kernel.  The parts it includes: what the rules ask of cells and lanelet polygons (fo_rule_cells.hpp), the
// frames (fo_rule_frame.hpp), the families (fo_rule_pedestrian.hpp, fo_rule_dynamic.hpp); the C entry points are in fo_scene.hip
// with the others, their decisions as plain functions of integers in fo_rule_plan.hpp.
//
// Replaces SpawnLocator.find_spawn_points' rule functions (ref: spawn_locator.py:80-139):
//   pedestrian behind a visible static obstacle   spawn_locator.py:323-476
//   pedestrian behind a turn                       spawn_locator.py:481-578
//   Car / Bicycle behind a visible dynamic obstacle  spawn_locator.py:145-317, rectangle fit :695-726
// The reference asks shapely for intersections of lines, buffers and polygons with the visible / occluded AREAS; here
// the same predicates are asked of the cell classes of fo_scene_visibility ("Rule families on cells"):
//   line.intersects(area)             -> a sample of the line (every cs/8) lies in a cell of that class
//   point.buffer(r).intersects(area)  -> the disc touches a cell square of that class
//   point.buffer(r).within(road)      -> every cell square the disc touches is road
//   area.buffer(b).exterior & line    -> samples where "disc of radius b touches the area" flips along the line
// The curvilinear frame is the polyline frame of the ego's reference path (utils/curvilinear.PolylineCS; the table
// [n][6] = x, y, s, segment length, unit tangent is built on the host once per reference path) or, with
// fo_spawn_rule_params_t::frame = 1, a table sampled from the caller's own frame object (x, y, s, polyline arc length, vertex normal:
// rl_cf_* of fo_rule_frame.hpp; the host builds it once per object, SpawnLocator._frame_setup).
// Checked against oracle/fo_spawn_rules_ref.py (an independent NumPy restatement of the same definitions).
//
// Launch shape: one workgroup for the turn rule + one per obstacle (static rule: a wave; dynamic rule: 1 024 threads and
// 100 KB of LDS for the 97 x 97 candidate lattice), then one small workgroup that applies what depends on the order of
// the obstacles (sorted by distance, the maxima of the YAML, 5 m between pedestrians) and writes the spawn points.
#pragma once
#include "fo_scene_state.hpp"
#include "fo_spawn_predict.hpp"
#include "fo_rule_plan.hpp"
#include "fo_rule_cells.hpp"
#include "fo_rule_frame.hpp"
#include "fo_rule_pedestrian.hpp"
#include "fo_rule_dynamic.hpp"

namespace {

// this wave's copy of the path table (a wave's LDS accesses are ordered)
__device__ __forceinline__ void rl_own_path(RuleView &v, double *dst) {
  if (v.n_path <= RL_PATHV) {
    for (int i = (threadIdx.x & 63); i < 6 * v.n_path; i += 64) dst[i] = v.path[i];
    v.path = dst;
  }
}

// blocks 1 .. O: an obstacle each (its record, the static rule, part 0 of the dynamic rule's lattice); blocks beyond: the
// other RL_PARTS - 1 parts of the dynamic rule's lattice -- of the c-th obstacle whose HOST-known flags allow the rule at
// all (present, dynamic role, no bicycle / pedestrian), c = (b - 1 - O) / (RL_PARTS - 1): the caller says how many there
// are (fo_spawn_rule_params_t::n_dynamic_plus1), and the launch dispatches helper workgroups -- sixteen waves and 144 KB of
// LDS each, a CU apiece -- for those only instead of for every obstacle (scenario 1: 23 workgroups instead of 113; whether
// such an obstacle is visible and the rule applies stays a decision of the device).  `all_obstacles`: the caller did not say.
__device__ __forceinline__ int rl_workgroup_obstacle(int O, const uint8_t *oflags, int all_obstacles, int &part) {
  const bool helper = (int)blockIdx.x > O;
  int o = (int)blockIdx.x - 1;
  part = helper ? 1 + ((int)blockIdx.x - 1 - O) % (RL_PARTS - 1) : 0;
  if (helper) {
    int want = ((int)blockIdx.x - 1 - O) / (RL_PARTS - 1);
    if (all_obstacles) o = want;
    else {
      o = -1;
      for (int i = 0; i < O; ++i)
        if ((oflags[i] & 13) == 5 && want-- == 0) { o = i; break; }
    }
  }
  return o;
}

// the obstacle's own workgroup without the dynamic rule: wave 0 keeps the record's head and the first cross line of the
// static rule, wave 1 the second (helper workgroups of an obstacle WITHOUT the dynamic rule have returned above; with it,
// every part clears the two validity words rec[2] / rec[5] in rl_dynamic_rule before its hand-off ticket -- the same value
// from sixteen writers, ordered before the last part's results by the fence in front of the ticket; the selection kernel
// is the next launch)
// samp (the lattice array), bytes: the two waves' sample tables; pathv, red: their copies of the path table
__device__ __forceinline__ void rl_obstacle_plain(RuleView &v, const RuleParams &pr, int o, int O, const double *ocorn, const double *ocen,
                                                  const uint8_t *oflags, const uint8_t *ovis, double *rec, bool vis, double *samp, double *red,
                                                  unsigned char *bytes, double *pathv) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave >= 2) return;
  for (int i = lane; i < RL_REC; i += 64)
    if ((i >= 8 && i < 14) == (wave == 1)) rec[i] = 0.0;
  if (wave == 0 && lane == 0) {
    const double dx = pr.ego_x - ocen[2 * o], dy = pr.ego_y - ocen[2 * o + 1];
    rec[0] = sqrt(dx * dx + dy * dy);
  }
  if (!vis) return;
  if (oflags[o] & 4) {                                       // a dynamic obstacle the rule does not apply to
    if (!(oflags[o] & 8) && wave == 0 && lane == 0) rec[1] = 2.0;   // (bicycles and pedestrians, :209-210: no role)
    return;
  }
  if (wave == 0 && lane == 0) rec[1] = 1.0;
  if (pr.behind_static) {
    rl_own_path(v, wave == 0 ? pathv : red);
    rl_static_rule(v, pr, o, O, ocorn, ocen, oflags, ovis, rec, samp + 2 * RL_MAXSAMP * wave, samp + 2 * RL_MAXSAMP * wave + RL_MAXSAMP,
                   bytes + RL_MAXSAMP * wave, wave);
  }
}

// flags of an obstacle at this step: bit0 present, bit1 occludes (not a bicycle), bit2 dynamic role, bit3 type bicycle or
// pedestrian (never triggers the dynamic rule, :209-210)
__global__ __launch_bounds__(RL_THREADS) void fo_spawn_rules_kernel(RuleView v, RuleParams pr, int O, const double *__restrict__ ocorn,
                                                             const double *__restrict__ ocen, const double *__restrict__ oyaw,
                                                             const double *__restrict__ odims, const uint8_t *__restrict__ oflags,
                                                             const uint8_t *__restrict__ ovis, double *__restrict__ recs,
                                                             int *__restrict__ g_lab, int *__restrict__ g_cnt, int all_obstacles, int n_helped) {
  // one LDS arena, carved per rule (the dynamic rule needs the two lattice arrays: 2 x 37.6 KB)
  __shared__ int lab[RL_LAT * RL_LAT];
  __shared__ int ired[RL_LAT * RL_LAT];
  __shared__ double red[3 * RL_THREADS];
  __shared__ unsigned char bytes[2048];
  __shared__ __align__(16) double polyv[2 * RL_PVERT];   // dynamic rule: the vertices of the candidate region's lanelet polygons (read as double2)
  // the reference path table into LDS: the projections and the arc-length searches of every rule are chains of dependent
  // reads of it (a binary search in HBM costs eight round trips of ~0.6 us; in LDS, of ~30 ns)
  __shared__ double pathv[6 * RL_PATHV];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // Only the dynamic rule needs the whole workgroup.  The others run on its first wave or two, which do not wait for the other
  // fourteen to be launched (sixteen waves of this size arrive over ~6 us): every wave that has nothing to do leaves at once,
  // the working waves copy the path table into LDS for themselves and meet no workgroup barrier.
  if (blockIdx.x == 0) {   // the turn rule's record
    if (wave > 0) return;
    double *rec = recs;
    for (int i = lane; i < RL_REC; i += 64) rec[i] = 0.0;
    if (pr.behind_turn && pr.intention != 0) {
      rl_own_path(v, pathv);
      static_assert(3 * RL_TURNW * sizeof(double) <= sizeof(lab), "the turn rule's three window arrays borrow the lattice array");
      double *lx = (double *)lab, *ly = lx + RL_TURNW, *cum = ly + RL_TURNW;
      rl_turn_rule(v, pr, rec, lx, ly, cum, bytes);
    }
    return;
  }
  const bool helper = (int)blockIdx.x > O;
  int part = 0;
  const int o = rl_workgroup_obstacle(O, oflags, all_obstacles, part);
  if (o < 0) return;      // (the caller counted more candidates than the flags hold: nothing to do)
  double *rec = recs + (size_t)(1 + o) * RL_REC;
  const bool vis = (oflags[o] & 1) && ovis[o];
  // (one call site for the dynamic rule, inlined: a call would put the kernel's RuleView on a stack in scratch memory -- and a
  // kernel with a private segment is dispatched noticeably later than one without, measured ~11 us here)
  bool dyn_rule = vis && (oflags[o] & 4) && !(oflags[o] & 8) && pr.behind_dynamic && (pr.intention == 0 || pr.intention == 1);
  if (dyn_rule && !helper && !all_obstacles) {
    // (a caller that counted fewer candidates than its flags hold: an obstacle beyond the count has no helper workgroups --
    // its lattice would never be handed over -- and is treated like a dynamic obstacle the rule does not apply to)
    int rank = 0;
    for (int i = 0; i < o; ++i) rank += (oflags[i] & 13) == 5;
    if (rank >= n_helped) dyn_rule = false;
  }
  if (helper && !dyn_rule) return;
  if (!dyn_rule) {
    rl_obstacle_plain(v, pr, o, O, ocorn, ocen, oflags, ovis, rec, vis, (double *)lab, red, bytes, pathv);
    return;
  }
  // the dynamic rule (straight ahead or left turn, :124-126): all sixteen waves, sixteen workgroups per obstacle
  if (v.n_path <= RL_PATHV) {
    for (int i = threadIdx.x; i < 6 * v.n_path; i += blockDim.x) pathv[i] = v.path[i];
    v.path = pathv;
  }
  if (!helper) {
    // (no fence behind the clear: the only other writer of the record is the rule's last part, which takes its ticket after this
    // workgroup has released its own -- rl_dynamic_rule fences before the ticket)
    if (threadIdx.x < RL_REC) rec[threadIdx.x] = 0.0;
  }
  __syncthreads();
  if (!helper && threadIdx.x == 0) {
    const double dx = pr.ego_x - ocen[2 * o], dy = pr.ego_y - ocen[2 * o + 1];
    rec[0] = sqrt(dx * dx + dy * dy);
    rec[1] = 2.0;
  }
  rl_dynamic_rule(v, pr, o, ocorn, ocen, oyaw, odims, rec, lab, red, ired, bytes, polyv, part, g_lab + (size_t)o * (RL_LAT * RL_LAT), g_cnt + o);
}

// what depends on the order of the obstacles: both lists sorted by distance (stable), the maxima of the YAML compared
// with '>' BEFORE appending (Q11), 5 m in s between pedestrians; output order = the reference's (dynamic, static, turn).
// out [max_out][8]: type code, x, y, yaw (NaN = none), s, d (NaN = none), source code, obstacle index (-1 = none)
__global__ void fo_spawn_rules_select_kernel(RuleView v, RuleParams pr, int O, const double *__restrict__ ocorn,
                                             const uint8_t *__restrict__ oflags, const uint8_t *__restrict__ ovis,
                                             const double *__restrict__ recs, int max_out, double *__restrict__ out,
                                             int32_t *__restrict__ n_out) {
  // (round 6, measured and dropped: the records and flags copied into LDS by the wave, the deciding thread reading them there
  // instead of in HBM -- the rules step does not move, same box, two passes: 0.0845 / 0.0831 against 0.0830 / 0.0850 ms)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  // a rule that ran out of table space left -1 in its validity word: the step's list would be short of a point the reference
  // finds, so there is NO list -- the count says -1, and a sweep over the step's agents delivers no verdict (fo_hip.h).  Only
  // a record the selection below CONSUMES can refuse the step: the turn record with the turn rule on, an obstacle the
  // distance-ordered loops visit before their maxima break.  The reference's list does not depend on the obstacles behind
  // the break, so neither does the refusal.
  bool over = false;
  int n = 0;
  auto put = [&](double type, double x, double y, double yaw, double s, double d, double src, double ob) {
    if (n < max_out) {
      double *q = out + 8 * (size_t)n;
      q[0] = type; q[1] = x; q[2] = y; q[3] = yaw; q[4] = s; q[5] = d; q[6] = src; q[7] = ob;
    }
    ++n;
  };
  // visit the obstacles of one role in ascending distance, ties in list order (a stable sort)
  auto next_by_distance = [&](double role, double last_d, int last_o) {
    int best = -1;
    double bd = INFINITY;
    for (int o = 0; o < O; ++o) {
      const double *r = recs + (size_t)(1 + o) * RL_REC;
      if (r[1] != role) continue;
      const bool after = r[0] > last_d || (r[0] == last_d && o > last_o);
      if (after && (r[0] < bd)) { bd = r[0]; best = o; }
    }
    return best;
  };
  if (pr.behind_dynamic && (pr.intention == 0 || pr.intention == 1)) {
    int n_dyn = 0, last_o = -1;
    double last_d = -1.0;
    for (;;) {
      const int o = next_by_distance(2.0, last_d, last_o);
      if (o < 0) break;
      const double *r = recs + (size_t)(1 + o) * RL_REC;
      last_d = r[0]; last_o = o;
      if (n_dyn > pr.max_dynamic) break;                                           // :212
      if (r[2] < 0.0) { over = true; continue; }
      if (r[2] != 0.0) { put(RL_TYPE_CAR, r[3], r[4], NAN, NAN, NAN, RL_SRC_DYNAMIC, o); ++n_dyn; }
      if (r[5] != 0.0) { put(RL_TYPE_BICYCLE, r[6], r[7], NAN, NAN, NAN, RL_SRC_DYNAMIC, o); ++n_dyn; }
    }
  }
  if (pr.behind_static) {
    double s_pos[RL_MAXPED];
    int n_st = 0, last_o = -1;
    double last_d = -1.0;
    for (;;) {
      const int o = next_by_distance(1.0, last_d, last_o);
      if (o < 0) break;
      const double *r = recs + (size_t)(1 + o) * RL_REC;
      last_d = r[0]; last_o = o;
      if (n_st > pr.max_static) break;                                             // :365
      if (r[2] < 0.0 || r[8] < 0.0) { over = true; continue; }                     // (both cross lines of a visited obstacle count)
      for (int li = 0; li < 2; ++li) {
        const double *q = r + 2 + 6 * li;
        if (q[0] == 0.0) continue;
        bool close = false;
        for (int i = 0; i < n_st && i < RL_MAXPED; ++i) close = close || fabs(s_pos[i] - q[3]) <= RL_MIN_DIST_PED;   // :453
        if (close) continue;
        put(RL_TYPE_PED, q[1], q[2], q[5], q[3], q[4], RL_SRC_STATIC, o);
        if (n_st < RL_MAXPED) s_pos[n_st] = q[3];
        ++n_st;
        break;                                                                     // one per obstacle
      }
    }
  }
  if (pr.behind_turn && pr.intention != 0) {
    const double *r = recs;
    if (r[0] < 0.0) over = true;
    else if (r[0] != 0.0) {
      bool ok = true;
      for (int o = 0; o < O && ok; ++o)                                            // :557: no visible obstacle within the 0.5 m disc
        if ((oflags[o] & 1) && ovis[o] && rl_seg_rect_distance(r[1], r[2], r[1], r[2], ocorn + 8 * (size_t)o) <= 0.5) ok = false;
      double ye, yp;
      if (ok && (!rl_lane_yaw_at(v, pr.ego_x, pr.ego_y, ye) || !rl_lane_yaw_at(v, r[1], r[2], yp))) ok = false;
      if (ok) {                                                                    // :561-572: the lanelet there must head elsewhere (>= 45 deg)
        double m = fmod(fabs(yp - ye), 6.283185307179586);
        if (m < 45.0 / 180.0 * 3.141592653589793) ok = false;
      }
      if (ok) put(RL_TYPE_PED, r[1], r[2], NAN, r[3], r[4], r[5], -1.0);
    }
  }
  *n_out = over ? -1 : n < max_out ? n : max_out;
}


// ---------------------------------------------------------------- rule points -> phantom agents, on the device
// Replaces the loop of FOInterface.evaluate_scenario over the spawn points (interface.py:186-198) with
// FOAgentManager.add_agent (agent.py:46-141) behind it: one wave per prediction slot (point i, route r).  Reads the records
// fo_spawn_rules_select_kernel wrote -- type, x, y, orientation (NaN = derive), s, d, source, obstacle -- in HBM.
struct RuleAgentTypes { double speed[3], raw_l[3], raw_w[3], infl_l[3], infl_w[3]; };   // 0 Car, 1 Bicycle, 2 Pedestrian

__global__ __launch_bounds__(64) void fo_spawn_rule_predict_kernel(
    RuleView v, int max_points, const double *__restrict__ points, const int32_t *__restrict__ n_points, int R, RuleAgentTypes ty,
    int n_path, const double *__restrict__ path, const int32_t *__restrict__ center_off, const double *__restrict__ center_xy,
    RouteView rv, int T, double dt, double var0, double factor, int slot0, int agent0, double *__restrict__ pos0,
    double *__restrict__ yaw0, PredOut o, int table_on, fo_agent_table_t at) {
  const int lane = threadIdx.x;
  const int i = blockIdx.x / R, r = blockIdx.x % R, slot = slot0 + blockIdx.x;
  const int n_raw = *n_points;
  const int n = min(max(n_raw, 0), max_points);
  const double vpow = pow(factor, (double)lane);   // (spawn_write_slot; here: under the first round trip)
  const bool on = i < n;
  const double *rec = points + 8 * (size_t)i;
  const int type = on ? (int)rec[0] : RL_TYPE_PED;
  const int ti = type == RL_TYPE_CAR ? 0 : type == RL_TYPE_BICYCLE ? 1 : 2;
  const double px = on ? rec[1] : 0.0, py = on ? rec[2] : 0.0;
  const int src = on ? (int)rec[6] : 0;
  double a0 = on ? rec[3] : 0.0;
  int ll = -1;
  if (on && ti == 2) {                                           // OAPPedestrianAgent._create_ped_trajectory (agent.py:451-481)
    if (a0 != a0) {
      const double *curve = path;
      int nc = n_path;
      if ((src == RL_SRC_LEFT || src == RL_SRC_RIGHT) && center_off) {       // mode 'lane_center' (interface.py:194)
        const int lc = rl_lanelet_of_wave(v, px, py);
        if (lc >= 0 && center_off[lc + 1] - center_off[lc] >= 2) { curve = center_xy + 2 * (size_t)center_off[lc]; nc = center_off[lc + 1] - center_off[lc]; }
      }
      a0 = heading_to_curve(lane, nc, curve, px, py);
    }
  } else if (on) {                                               // OAPVehicleAgent (agent.py:283-312): the lanelet under the point
    ll = rv.RT > 0 ? rl_lanelet_of_wave(v, px, py) : -1;
    if (ll >= 0 && rv.count[(size_t)ll * rv.RT] >= 2) {          // heading of the record: first segment of route 0
      const double *q = rv.xy + 2 * (size_t)rv.first[(size_t)ll * rv.RT];
      a0 = atan2(q[3] - q[1], q[2] - q[0]);
    } else {
      ll = -1;
      a0 = heading_to_curve(lane, n_path, path, px, py);
    }
  }
  if (r == 0 && lane == 0) { pos0[2 * (agent0 + i)] = px; pos0[2 * (agent0 + i) + 1] = py; yaw0[agent0 + i] = a0; }
  spawn_write_slot(lane, slot, r, on, px, py, a0, type, ty.speed[ti], ty.raw_l[ti], ty.raw_w[ti], ty.infl_l[ti], ty.infl_w[ti], ll, rv, T,
                   dt, var0, factor, o, table_on, at, vpow, -1.0);
  // A refused list (the selection kernel's -1) adds no rule agents -- and must not read as "nothing hidden there": the first
  // rule slot's length says so to whoever takes the arrays (fo_prep_agents_kernel raises the status word for it, the host
  // views read it as 0 live samples), and where this kernel writes the sweep's table itself it raises the word here.
  // fo_reduce_kernel turns the word into NaN costs and safe = 0 (fo_hip.h, fo_sweep_check).  After spawn_write_slot: the
  // same lane's later store to the same word.
  if (n_raw < 0 && blockIdx.x == 0 && lane == 0) {
    o.len[slot] = FO_LEN_REFUSED;
    if (table_on) atomicMax(at.status + 2, at.gen);
  }
}

}  // namespace
