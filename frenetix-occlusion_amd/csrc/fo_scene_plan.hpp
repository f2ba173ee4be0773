// fo_scene_plan.hpp -- the host decisions of the scene stage as functions of plain integers: which form of a kernel a call
// takes, and the reaches the hidden-traffic extensions derive from a squared radius.  Host-only integer arithmetic, no HIP
// header: fo_scene.hip includes it first, the device headers take the constants below from here, and a host compiler builds it
// alone (tests/test_scene_plan_cpu.py, next to the Python restatement tests/scene_forms.expected_form).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

constexpr int SCENE_CHUNK = 64;            // boundary pieces per chunk box (a lane each)
constexpr int RAY_WAVES = 5;               // waves of a ray / probe / settle workgroup ...
constexpr int COMPACT_BLOCK = 256;         // window cells per block count of the compaction
constexpr int COMPACT_ONE_LAUNCH = 2048;   // block counts the one-launch compaction sums per block
constexpr int FV_THREADS = 256;            // threads per pose of the future visibility
constexpr int HRR_HALO = 16;               // ring staged around a tile of the road distance = steps a band can hold
constexpr int HRR_BAND = 12 * HRR_HALO;    // B: distance units per band launch (12 per axis step)
constexpr int HW_LANES = 8;                // lanes per trajectory of the witness kernel: one per lattice direction
constexpr int HW_PER_BLOCK = 32;           // ... and trajectories per workgroup of 256 threads
constexpr int HB_THREADS = 256;            // threads per workgroup of the brake kernel
constexpr int OMR_SMALL_N = 16;            // largest halo of the road occlusion memory's small form
constexpr int OMF_SMALL_N = 16;            // ... and of its vehicle layer's (a lane per staged column: 32 + 2 n <= 64)

// ... or one: the boundary soup is a single group of chunk boxes (<= 64 chunks = 4 096 pieces: only the first wave of five would
// have pieces to scan) and the obstacle sides fit a wave; forced: FO_SCENE_FIVE_WAVES is set
inline int ray_waves(int E, int O, bool forced) {
  return (E + SCENE_CHUNK - 1) / SCENE_CHUNK <= 64 && 4 * O <= 64 && !forced ? 1 : RAY_WAVES;
}

// scan + scatter instead of the one-launch compaction: more than 2 048 blocks of 256 cells -- a window of 725 x 725 cells or
// more, which at the 0.5 m cell is any sensor radius above 120.5 m (SensorModel._window_for: ceil(3 r / cs) + 1 cells per side)
inline bool compact_two_launches(int cells) { return (cells + COMPACT_BLOCK - 1) / COMPACT_BLOCK > COMPACT_ONE_LAUNCH; }

// rays a thread of the future visibility walks (tid, tid + 256, ...)
inline int fv_rays_per_thread(int n_rays) { return (n_rays + FV_THREADS - 1) / FV_THREADS; }

// floor(sqrt(v)), v >= 0: the float guess corrected both ways
inline int64_t isqrt(int64_t v) {
  int64_t l = (int64_t)std::sqrt((double)v);
  while (l * l > v) --l;
  while ((l + 1) * (l + 1) <= v) ++l;
  return l;
}

// a hidden road user's reach of r2 (cells squared): h cells of halo; L distance units along the road (12 per axis step, 17 per
// diagonal one, 13 per cell); a path of cost <= L has at most L / 12 steps
inline int reach_cells(int r2) { return (int)isqrt(r2); }
inline int road_reach(int r2) { return (int)isqrt((int64_t)169 * r2); }
inline int road_steps(int L) { return L / 12; }
// workgroups of the witness kernel over M trajectories, and the shortest row that holds every walk within L
inline int witness_blocks(int M) { return (int)(((int64_t)M + HW_PER_BLOCK - 1) / HW_PER_BLOCK); }
inline int witness_min_cap(int r2) { return road_steps(road_reach(r2)); }
// the brake kernel: a lane per brake start b, G = the power of two >= min(T, 64) lanes per trajectory (b = lane, lane + G, ..),
// HB_THREADS / G trajectories per workgroup, whose six rows of T float64 (x, y, cos, sin, arc, v) are staged in LDS
inline int brake_group(int T) { int G = 1; while (G < T && G < 64) G <<= 1; return G; }
inline int brake_per_block(int T) { return HB_THREADS / brake_group(T); }
inline int brake_blocks(int M, int T) { const int p = brake_per_block(T); return (int)(((int64_t)M + p - 1) / p); }
inline size_t brake_lds_bytes(int T) { return (size_t)brake_per_block(T) * 6 * (size_t)T * sizeof(double); }
// the brake kernel by classes: the same lanes and grid; per trajectory its qmin row (T int32) joins the six rows in LDS, and the
// workgroup keeps the threshold table thr [C][T] int32 behind them (at T = 254, C * T = 896 at most: 56 416 bytes).  The per-class
// state lives in registers, indexed at compile time: the kernel's class count is the power of two >= C
inline int brake_classes_width(int C) { return C <= 1 ? 1 : C <= 2 ? 2 : C <= 4 ? 4 : 8; }
inline int brake_classes_blocks(int M, int T) { return brake_blocks(M, T); }
inline size_t brake_classes_lds_bytes(int T, int C) {
  return (size_t)brake_per_block(T) * (size_t)T * (6 * sizeof(double) + sizeof(int32_t)) + (size_t)C * (size_t)T * sizeof(int32_t);
}
// the brake kernel by road users: the same lanes and grid again; per trajectory one qmin row per map (K maps, one per forecast) joins
// the six rows, the table follows: brake_per_block(T) * T * (48 + 4 K) + 4 C T bytes.  brake_users_lds_bound: no call needs more --
// T = 254 (4 trajectories per workgroup), 3 maps and a full table of 896 entries, 64 544 bytes, under the 64 KB of a workgroup.
// The kernel's class count is 4 or 8 (a single class is fo_scene_hidden_brake_classes' case), its map count is K itself
constexpr int BRAKE_USERS_MAX_MAPS = 3;    // FO_HIDDEN_BRAKE_MAX_MAPS
constexpr int BRAKE_USERS_MAX_TABLE = 896; // FO_HIDDEN_BRAKE_MAX_TABLE
inline int brake_users_width(int C) { return C <= 4 ? 4 : 8; }
inline int brake_users_blocks(int M, int T) { return brake_blocks(M, T); }
inline size_t brake_users_lds_bytes(int T, int K, int C) {
  return (size_t)brake_per_block(T) * (size_t)T * (6 * sizeof(double) + (size_t)K * sizeof(int32_t)) + (size_t)C * (size_t)T * sizeof(int32_t);
}
inline size_t brake_users_lds_bound() {
  return (size_t)brake_per_block(254) * 254 * (6 * sizeof(double) + BRAKE_USERS_MAX_MAPS * sizeof(int32_t)) + BRAKE_USERS_MAX_TABLE * sizeof(int32_t);
}
// the brake ladder: a lane per (m, b, k), k fastest, padded to Kp = the power of two >= K (brake_ladder_width); G lanes per
// trajectory = the power of two >= min(B * Kp, HB_THREADS) -- then doubled while the six rows of the workgroup's HB_THREADS / G
// trajectories (48 T bytes each) exceed BRAKE_LADDER_ROWS_BYTES: the lanes' rule alone would stage 256 trajectories with B * K = 1,
// 3 MB at T = 254.  Half of the 64 KB a workgroup may take: a CU then holds four such workgroups, not two.  Behind the rows
// stands one int32 per lane of the workgroup, through which the waves of a trajectory (G > 64) meet for commit
constexpr int BRAKE_LADDER_MAX_LEVELS = 64;       // FO_HIDDEN_BRAKE_MAX_LEVELS
constexpr int BRAKE_LADDER_ROWS_BYTES = 32768;
inline int brake_ladder_width(int K) { int Kp = 1; while (Kp < K && Kp < BRAKE_LADDER_MAX_LEVELS) Kp <<= 1; return Kp; }
inline int brake_ladder_group(int T, int K, int B) {
  int G = brake_ladder_width(K);
  while (G < HB_THREADS && (int64_t)G < (int64_t)B * brake_ladder_width(K)) G <<= 1;
  while (G < HB_THREADS && (size_t)(HB_THREADS / G) * 6 * (size_t)T * sizeof(double) > (size_t)BRAKE_LADDER_ROWS_BYTES) G <<= 1;
  return G;
}
inline int brake_ladder_per_block(int T, int K, int B) { return HB_THREADS / brake_ladder_group(T, K, B); }
inline int brake_ladder_blocks(int M, int T, int K, int B) {
  const int p = brake_ladder_per_block(T, K, B);
  return (int)(((int64_t)M + p - 1) / p);
}
inline size_t brake_ladder_lds_bytes(int T, int K, int B) {
  return (size_t)brake_ladder_per_block(T, K, B) * 6 * (size_t)T * sizeof(double) + HB_THREADS * sizeof(int32_t);
}
// the brake ladder by road users: the ladder's lanes -- a lane per (m, b, l), l fastest, padded to Lp = brake_ladder_width(L); G
// lanes per trajectory = the power of two >= min(B * Lp, HB_THREADS), then doubled while the rows of the workgroup's HB_THREADS / G
// trajectories exceed BRAKE_LADDER_ROWS_BYTES -- with the users kernel's rows: per trajectory the six float64 rows and one int32 qmin
// row per map, T * (48 + 4 K) bytes.  Behind them the table (4 C T bytes) and the commit exchange, one int32 per class and lane of
// the workgroup.  brake_ladder_users_lds_bound: no call needs more -- the rows stay within BRAKE_LADDER_ROWS_BYTES wherever a
// workgroup holds two trajectories or more, a single one takes at most 254 * 60 bytes; the table is part of the argument
// (4 C T + 8 L <= BRAKE_LADDER_USERS_MAX_ARG_BYTES); the exchange is at most 8 classes wide: 44 544 bytes, under the 64 KB of a
// workgroup
constexpr int BRAKE_LADDER_USERS_MAX_ARG_BYTES = 3584;   // FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES
constexpr int BRAKE_LADDER_USERS_MAX_CLASSES = 8;        // FO_HIDDEN_BRAKE_MAX_CLASSES
inline int brake_ladder_users_width(int L) { return brake_ladder_width(L); }
inline int brake_ladder_users_group(int T, int K, int L, int B) {
  const int Lp = brake_ladder_users_width(L);
  const size_t per_traj = (size_t)T * (6 * sizeof(double) + (size_t)K * sizeof(int32_t));
  int G = Lp;
  while (G < HB_THREADS && (int64_t)G < (int64_t)B * Lp) G <<= 1;
  while (G < HB_THREADS && (size_t)(HB_THREADS / G) * per_traj > (size_t)BRAKE_LADDER_ROWS_BYTES) G <<= 1;
  return G;
}
inline int brake_ladder_users_per_block(int T, int K, int L, int B) { return HB_THREADS / brake_ladder_users_group(T, K, L, B); }
inline int brake_ladder_users_blocks(int M, int T, int K, int L, int B) {
  const int p = brake_ladder_users_per_block(T, K, L, B);
  return (int)(((int64_t)M + p - 1) / p);
}
inline size_t brake_ladder_users_lds_bytes(int T, int K, int C, int L, int B) {
  return (size_t)brake_ladder_users_per_block(T, K, L, B) * (size_t)T * (6 * sizeof(double) + (size_t)K * sizeof(int32_t)) +
         (size_t)C * (size_t)T * sizeof(int32_t) + (size_t)C * HB_THREADS * sizeof(int32_t);
}
inline size_t brake_ladder_users_lds_bound() {
  const size_t one = (size_t)254 * (6 * sizeof(double) + BRAKE_USERS_MAX_MAPS * sizeof(int32_t));
  return (one > (size_t)BRAKE_LADDER_ROWS_BYTES ? one : (size_t)BRAKE_LADDER_ROWS_BYTES) + BRAKE_LADDER_USERS_MAX_ARG_BYTES +
         (size_t)BRAKE_LADDER_USERS_MAX_CLASSES * HB_THREADS * sizeof(int32_t);
}
// the pose preparation of the fail-safe verdict: a lane per trajectory (its arc is a serial sum), 64 trajectories per workgroup
constexpr int POSES_THREADS = 64;
inline int poses_blocks(int M) { return (int)(((int64_t)M + POSES_THREADS - 1) / POSES_THREADS); }
// the fail-safe verdict: the users kernel's lanes over the first B brake starts only -- a lane per (m, b), b < B (b = lane,
// lane + G, ..), G = the power of two >= min(B, 64) lanes per trajectory, all in one wave.  A workgroup serves HB_THREADS / G
// trajectories, or fewer where their rows (the users kernel's: T * (48 + 4 K) bytes each) would exceed BRAKE_LADDER_ROWS_BYTES: the
// lanes' rule alone would stage 256 trajectories at B = 1, 3.9 MB at T = 254, K = 3.  The lanes beyond per_block * G take part in
// the staging and then have no trajectory.  Behind the rows stands the table (4 C T bytes).  brake_verdict_lds_bound: no call needs
// more -- a single trajectory takes at most 254 * 60 bytes, under the rows' bound
inline int brake_verdict_group(int B) { int G = 1; while (G < B && G < 64) G <<= 1; return G; }
inline int brake_verdict_per_block(int T, int K, int B) {
  const size_t per_traj = (size_t)T * (6 * sizeof(double) + (size_t)K * sizeof(int32_t));
  const int by_lanes = HB_THREADS / brake_verdict_group(B);
  const int by_rows = (int)((size_t)BRAKE_LADDER_ROWS_BYTES / per_traj);
  const int p = by_lanes < by_rows ? by_lanes : by_rows;
  return p < 1 ? 1 : p;
}
inline int brake_verdict_blocks(int M, int T, int K, int B) {
  const int p = brake_verdict_per_block(T, K, B);
  return (int)(((int64_t)M + p - 1) / p);
}
inline size_t brake_verdict_lds_bytes(int T, int K, int C, int B) {
  return (size_t)brake_verdict_per_block(T, K, B) * (size_t)T * (6 * sizeof(double) + (size_t)K * sizeof(int32_t)) +
         (size_t)C * (size_t)T * sizeof(int32_t);
}
inline size_t brake_verdict_lds_bound() { return (size_t)BRAKE_LADDER_ROWS_BYTES + BRAKE_USERS_MAX_TABLE * sizeof(int32_t); }
// the ladder verdict: the lanes of the brake ladder by road users over the first B brake starts -- a lane per (m, b, l), l fastest,
// padded to Lp = brake_ladder_width(L); G = the power of two >= min(B * Lp, HB_THREADS) lanes per trajectory (min(256, Lp *
// pow2ceil(B))), ceil(B * Lp / G) rounds over b.  A workgroup serves HB_THREADS / G trajectories, or fewer where their rows (T * (48
// + 4 K) bytes each) would exceed BRAKE_LADDER_ROWS_BYTES, as in the fail-safe verdict: at small B * Lp the lanes' rule alone would
// stage far more rows than LDS holds; the lanes beyond per_block * G take part in the staging and then have no trajectory.  Behind
// the rows stand the table (4 C T bytes) and the exchange through which the waves of a trajectory (G > 64) meet: one key and one
// rank per class for each of the workgroup's HB_THREADS / 64 waves.  brake_ladder_verdict_lds_bound: no call needs more -- a single
// trajectory takes at most 254 * 60 bytes, under the rows' bound; the table is part of the argument
constexpr int BRAKE_LADDER_VERDICT_WAVES = HB_THREADS / 64;
inline int brake_ladder_verdict_group(int L, int B) {
  const int Lp = brake_ladder_users_width(L);
  int G = Lp;
  while (G < HB_THREADS && (int64_t)G < (int64_t)B * Lp) G <<= 1;
  return G;
}
inline int brake_ladder_verdict_per_block(int T, int K, int L, int B) {
  const size_t per_traj = (size_t)T * (6 * sizeof(double) + (size_t)K * sizeof(int32_t));
  const int by_lanes = HB_THREADS / brake_ladder_verdict_group(L, B);
  const int by_rows = (int)((size_t)BRAKE_LADDER_ROWS_BYTES / per_traj);
  const int p = by_lanes < by_rows ? by_lanes : by_rows;
  return p < 1 ? 1 : p;
}
inline int brake_ladder_verdict_blocks(int M, int T, int K, int L, int B) {
  const int p = brake_ladder_verdict_per_block(T, K, L, B);
  return (int)(((int64_t)M + p - 1) / p);
}
inline size_t brake_ladder_verdict_lds_bytes(int T, int K, int C, int L, int B) {
  return (size_t)brake_ladder_verdict_per_block(T, K, L, B) * (size_t)T * (6 * sizeof(double) + (size_t)K * sizeof(int32_t)) +
         (size_t)C * (size_t)T * sizeof(int32_t) + (size_t)(C + 1) * BRAKE_LADDER_VERDICT_WAVES * sizeof(int32_t);
}
inline size_t brake_ladder_verdict_lds_bound() {
  return (size_t)BRAKE_LADDER_ROWS_BYTES + BRAKE_LADDER_USERS_MAX_ARG_BYTES +
         (size_t)(BRAKE_LADDER_USERS_MAX_CLASSES + 1) * BRAKE_LADDER_VERDICT_WAVES * sizeof(int32_t);
}
// the harm ladder: the ladder verdict's lanes, grid and LDS; where a trajectory has more than a wave (G > 64) the curve's exchange
// stands behind the ladder verdict's, aligned to 8 bytes: one float64 harm and one int32 class per lane of the workgroup.
// brake_harm_ladder_lds_bound: no call needs more -- 39 568 bytes, under the 64 KB of a workgroup
constexpr int BRAKE_HARM_LADDER_EXCHANGE_BYTES = HB_THREADS * (int)(sizeof(double) + sizeof(int32_t));
inline size_t brake_harm_ladder_lds_bytes(int T, int K, int C, int L, int B) {
  const size_t base = (brake_ladder_verdict_lds_bytes(T, K, C, L, B) + 7) / 8 * 8;
  return base + (brake_ladder_verdict_group(L, B) > 64 ? (size_t)BRAKE_HARM_LADDER_EXCHANGE_BYTES : 0);
}
inline size_t brake_harm_ladder_lds_bound() {
  return (brake_ladder_verdict_lds_bound() + 7) / 8 * 8 + (size_t)BRAKE_HARM_LADDER_EXCHANGE_BYTES;
}
// the harm ladder by approach angle: the harm ladder's lanes, grid and LDS; behind its last byte (a multiple of 8) stands the harm of
// the "met" case, one float64 per class and trajectory of the workgroup ([per_block][C]), formed once behind first[c] and read in
// every round.  brake_harm_ladder_lanes_lds_bound: no call needs more -- a workgroup holds at most HB_THREADS trajectories of 8
// classes, 16 384 bytes on top of the harm ladder's bound: 55 952 bytes, under the 64 KB of a workgroup
inline size_t brake_harm_ladder_lanes_lds_bytes(int T, int K, int C, int L, int B) {
  return brake_harm_ladder_lds_bytes(T, K, C, L, B) + (size_t)brake_ladder_verdict_per_block(T, K, L, B) * (size_t)C * sizeof(double);
}
inline size_t brake_harm_ladder_lanes_lds_bound() {
  return brake_harm_ladder_lds_bound() + (size_t)HB_THREADS * BRAKE_LADDER_USERS_MAX_CLASSES * sizeof(double);
}
// band launches of the road distance up to L (one also when the reach is 0: the sources)
inline int reach_bands(int L) { return L > 0 ? (L + HRR_BAND - 1) / HRR_BAND : 1; }
// the road occlusion memory's form by its halo n = road_steps(L)
inline bool omr_small(int n) { return n <= OMR_SMALL_N; }
// the vehicle layer's form (fo_occlusion_memory_flow_kernel) by the same halo
inline bool omf_small(int n) { return n <= OMF_SMALL_N; }

}  // namespace
