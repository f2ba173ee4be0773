// fo_rule_plan.hpp -- the host decisions of fo_scene_spawn_rules as functions of plain integers: the table space the rule
// families hold (the entry refuses what exceeds it; it keeps the texts and the order), the spawn points they can emit, the
// obstacles whose dynamic rule gets helper workgroups, and the launch grid.  Host-only integer arithmetic, no HIP header: the
// device headers take the constants below from here (the kernels answer the same limits with -1 in a validity word), and a host
// compiler builds it alone (tests/test_rule_plan_cpu.py, next to an independent Python restatement and SpawnLocator's own copies).
#pragma once

namespace {

constexpr int RL_LAT = 97;                         // nodes per side of the 0.25 m candidate lattice (2 x 12 m + 1)
constexpr int RL_TURNW = 1536;                      // vertices of the reference window the turn rule holds (40 m of path; fo_scene_spawn_rules refuses more)
constexpr int RL_FIFTHV = 512;                     // every-fifth-vertex queries of the window (dynamic rule outside an intersection)
constexpr int RL_MAXSAMP = 1024;                   // samples of a rule polyline (cs/8 steps; 40 m at cs = 0.5 -> 641)
constexpr int RL_REC = 24;                         // doubles per per-workgroup record
constexpr int RL_PARTS = 16;                       // workgroups that share a dynamic obstacle's candidate lattice
constexpr int RL_THREADS = 1024;                   // the dynamic rule's lattice work spreads over sixteen waves (the other rules use one)
constexpr int RL_MAXPED = 16;                      // obstacles whose pedestrians the selection compares (5 m apart in s)

// which families a call runs: the turn rule needs a turning intention, the dynamic rule straight ahead or a left turn (:124-126)
inline bool rule_turn_on(int behind_turn, int intention) { return behind_turn && intention != 0; }
inline bool rule_dynamic_on(int behind_dynamic, int intention) { return behind_dynamic && (intention == 0 || intention == 1); }

// table space the host can see (nw = vertices of the reference window, P = lanelets of the map)
inline bool rule_turn_window_over(int behind_turn, int intention, int nw) { return rule_turn_on(behind_turn, intention) && nw > RL_TURNW; }
inline bool rule_max_static_over(int behind_static, int max_static) { return behind_static && max_static > RL_MAXPED - 1; }
inline bool rule_lanelets_over(int P) { return P > RL_LAT * RL_LAT; }               // (the flag array is the lattice's companion)
inline int rule_fifth_vertices(int nw) { return (nw + 4) / 5; }
inline bool rule_fifth_over(int nw) { return rule_fifth_vertices(nw) > RL_FIFTHV; }

// the select kernel compares the maxima BEFORE appending and a dynamic obstacle can yield two points (Q11): what the three
// families can emit.  A smaller buffer would silently lose the last points in the reference's order (the turn rule's
// pedestrian first) -- phantoms the sweep then never sees.
inline int rule_capacity(int behind_dynamic, int max_dynamic, int behind_static, int max_static, int behind_turn) {
  return (behind_dynamic ? (max_dynamic > 0 ? max_dynamic : 0) + 2 : 0) + (behind_static ? (max_static > 0 ? max_static : 0) + 1 : 0) +
         (behind_turn ? 1 : 0);
}

// helper workgroups of the dynamic rule for the obstacles that MAY take it (n_dynamic_plus1 - 1 of them by the caller's flags;
// 0 = not told: every obstacle) -- none when the rule is off or the ego turns right
inline bool rule_told(int n_dynamic_plus1) { return n_dynamic_plus1 > 0; }
inline int rule_helped(int n_dynamic_plus1, int O, bool dynamic_on) {
  if (!dynamic_on) return 0;
  return rule_told(n_dynamic_plus1) ? (n_dynamic_plus1 - 1 < O ? n_dynamic_plus1 - 1 : O) : O;
}
// the turn rule's workgroup, one per obstacle, and the other RL_PARTS - 1 parts of every helped obstacle's lattice
inline int rule_grid(int O, int n_dyn) { return 1 + O + n_dyn * (RL_PARTS - 1); }

}  // namespace
