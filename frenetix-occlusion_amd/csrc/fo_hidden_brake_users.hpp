// fo_hidden_brake_users.hpp -- hidden-traffic brake clearance for mixed road users in one walk (fo_scene_hidden_brake_users;
// DESIGN.md §5.10 "Brake clearance by road users").  An EXTENSION, not part of the reference.  Included by fo_scene.hip after
// fo_hidden_brake_classes.hpp (same translation unit, same flags: -ffp-contract=off).
//
// The home of what the four users-family kernels (this one and fo_hidden_brake_{verdict,ladder_users,ladder_verdict}.hpp) share,
// each piece stated once: the staging of rows, qmin rows and table (hbu_stage), the class masks (hbu_masks), first[c] (hbu_first)
// and the walk of one manoeuvre (hbu_walk), on top of fo_hidden_brake.hpp's pieces.  Each kernel keeps its lane layout, its
// reductions and its outputs.
//
// Inputs are the key maps and qmin of K clearance calls over the same trajectories and window (one per forecast: a metric and a flow
// each), a threshold table thr [C][T] and map_of [C], the map each class of hidden road user is held against.  The pose arithmetic of
// a manoeuvre depends on neither: the manoeuvre of (m, b) is walked once, and under each braking pose ONE traversal of the footprint
// keeps one minimum key per map.  The definition stands in include/fo_hip.h.
//   fo_hr_brake_users_kernel<NC, NK>  the lanes of fo_hr_brake_classes_kernel: a lane per brake start (m, b), G = brake_group(T)
//                        lanes per trajectory, the six rows in LDS; next to them the K qmin rows of each trajectory
//                        ([K][per_block][T]) and the threshold table (brake_users_lds_bytes).  NC = brake_users_width(C) >= C and
//                        NK = K are compile-time: the per-class state is indexed by fully unrolled loops alone, the per-map minima
//                        are three named values (HbuKeys), and all of it stays in registers; map_of[c] is a run-time value, so
//                        every class is tested on every map and its own map's answer is picked by class masks (hbu_hits): no value
//                        is ever selected or indexed by it.  Instantiations: NC in {4, 8} x NK in {1, 2, 3}.
// The key maps are read through the caches and never written by these kernels, so two of them may be the same buffer: the scan's
// `__restrict__` on map 0 says nothing about memory that nobody modifies.  Next to fo_hidden_brake.hpp's bounds, for all four
// kernels: a class index into the table is bounded by c < C, and a map is read only at a window index that was tested against the
// window: no content of the keys, qmin, thr or map_of can make a lane read out of range (a map_of outside [0, K), which the entry
// refuses, would select map 0).  Every byte of every output is written.
#pragma once
#include "fo_hidden_brake_classes.hpp"

namespace {

struct HrBrakeUsersArgs {
  int M, T, G, C;                       // G lanes per trajectory (power of two, <= 64), C classes
  const double *x, *y, *heading;        // [M][T], [M][T], [M][T][2]
  const int32_t *len;                   // [M] or null
  double hl, hw, wb;
  double rx0, ry0, cs;
  const uint8_t *raster;
  int rnx, rny;
  int ix0, iy0, nx, ny;                 // the window
  // named members, no arrays of pointers: with key[3] and qmin[3] the register allocator kept a 16-byte spill slot (and the 4-byte
  // scavenging slot that follows any stack object) in the frame of the NK >= 2 instantiations -- never accessed, but a private segment
  const int32_t *key0, *key1, *key2;    // [ny][nx] each; those beyond K are null and never read
  const int32_t *qmin0, *qmin1, *qmin2; // [M][T] each
  uint32_t map_of;                      // map_of[c] in [0, K) in bits 2 c, 2 c + 1 (hbu_map_of); classes beyond C have 0
  const double *v, *arc;                // [M][T]
  double a_brake, dt;
  int32_t *brake_first;                 // [C][M][T]
  int32_t *stop;                        // [M][T]
  int32_t *commit, *first;              // [C][M]
};
static_assert(sizeof(HrBrakeUsersArgs) + sizeof(HbThr) <= 4096, "the arguments, map_of and the table fit the kernel-argument segment");
static_assert(FO_HIDDEN_BRAKE_MAX_MAPS == 3 && FO_HIDDEN_BRAKE_MAX_CLASSES == 8, "brake_users_width and the instantiations serve 8 classes on 3 maps");
static_assert(BRAKE_USERS_MAX_MAPS == FO_HIDDEN_BRAKE_MAX_MAPS && BRAKE_USERS_MAX_TABLE == FO_HIDDEN_BRAKE_MAX_TABLE,
              "brake_users_lds_bound speaks of the header's limits");

// The minimum key per map: three named values, no array.  Maps beyond NK are never touched: `if constexpr` removes their code.
struct HbuKeys { int q0, q1, q2; };
__host__ __device__ __forceinline__ int hbu_map_of(uint32_t packed, int c) { return (int)(packed >> (2 * c) & 3u); }
// bit c: class c -- of those in `live` -- has min key <= thr[c][i] on ITS map.  Every class is tested against every map and the
// answer of its own map is picked by the class masks cm1, cm2 (bit c: class c is on map 1 / map 2; neither: map 0): compares and bit
// operations alone, nothing is selected by the run-time value map_of[c] (a value selected by it, `mo == 1 ? q1 : ...`, goes to
// scratch at NK = 3: the compiler makes a load at a run-time offset of the chain of selects).
template <int NC, int NK>
__device__ __forceinline__ unsigned hbu_hits(const HbuKeys &q, const int32_t *TH, int T, int i, unsigned live, unsigned cm1, unsigned cm2) {
  unsigned h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (live >> c & 1u) {               // (uniform: classes beyond C read no threshold)
      const int t = TH[c * T + i];
      h0 |= (unsigned)(q.q0 <= t) << c;
      if constexpr (NK > 1) h1 |= (unsigned)(q.q1 <= t) << c;
      if constexpr (NK > 2) h2 |= (unsigned)(q.q2 <= t) << c;
    }
  unsigned h = h0 & ~(cm1 | cm2);
  if constexpr (NK > 1) h |= h1 & cm1;
  if constexpr (NK > 2) h |= h2 & cm2;
  return h;
}

// The rows, the NK qmin rows ([NK][per_block][T] at QM) and the table ([C][T] at TH) of a workgroup; table(t) is entry t of the
// caller's table (thr.v[t], or pk.w[2 L + t] behind the levels).  A callable, not a pointer: the table is part of a by-value kernel
// argument, and a pointer into such an argument is how a kernel acquires a stack copy of it -- a private segment.  The caller's
// __syncthreads() follows.
template <int NK, class Args, class F>
__device__ __forceinline__ void hbu_stage(const Args &a, double *rows, int32_t *QM, int32_t *TH, long long m0, int per_block, F &&table) {
  const size_t plane = (size_t)per_block * a.T;
  hb_stage_rows(a, rows, m0, per_block, [&](int t, size_t i) {
    QM[t] = a.qmin0[i];
    if constexpr (NK > 1) QM[plane + t] = a.qmin1[i];
    if constexpr (NK > 2) QM[2 * plane + t] = a.qmin2[i];
  });
  for (int t = threadIdx.x; t < a.C * a.T; t += HB_THREADS) TH[t] = table(t);    // (the table fits its argument: the host's refusal)
}

// every: bit c, class c is there (c < C) -- in the walk: it has no first hit yet; cm1, cm2: bit c, class c is held against map 1 / 2
struct HbuMasks { unsigned every, cm1, cm2; };
template <int NC>
__device__ __forceinline__ HbuMasks hbu_masks(uint32_t map_of, int nc) {
  unsigned cm1 = 0, cm2 = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int mo = hbu_map_of(map_of, c);
    if (c < nc && mo == 1) cm1 |= 1u << c;
    if (c < nc && mo == 2) cm2 |= 1u << c;
  }
  return HbuMasks{(1u << nc) - 1u, cm1, cm2};
}

// first[c] = min { k < Lm : qmin_map_of[c][m][k] <= thr[c][k] }, -1 if there is none.  `width` consecutive lanes of one wave (a
// power of two) split the samples, this lane from `start` on; Q: the trajectory's qmin row of map 0, map k2 at Q[k2 * plane + k].
template <int NC, int NK>
__device__ __forceinline__ void hbu_first(const int32_t *Q, size_t plane, const int32_t *TH, int T, int Lm, int start, int width,
                                          const HbuMasks &mk, int (&fm)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) fm[c] = 0x7fffffff;
  for (int k = start; k < Lm; k += width) {
    HbuKeys q{Q[k], 0, 0};
    if constexpr (NK > 1) q.q1 = Q[plane + k];
    if constexpr (NK > 2) q.q2 = Q[2 * plane + k];
    const unsigned h = hbu_hits<NC, NK>(q, TH, T, k, mk.every, mk.cm1, mk.cm2);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (h >> c & 1u) fm[c] = fm[c] < k ? fm[c] : k;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hb_shfl_min(fm[c], 1, width);
    if (fm[c] == 0x7fffffff) fm[c] = -1;
  }
}

// The walk of the manoeuvre that brakes from sample b < Lm at speed vb with a_brake (st: its stop sample): bf[c] becomes the first
// sample at which class c is hit, -1 if none.  X: the trajectory's six rows (row r from X + r T).  The scan runs over map 0; for
// every cell that passes the float64 point-in-rectangle test its callback forms the window index from (gx, gy) and reads maps 1
// and 2 only while they have an open class; outside the window the value it was handed (0 on raster road, NONE elsewhere) holds
// for every map.  Class c tests the minimum of map_of[c]; the walk ends when every class has its first hit, or at the standing
// pose, where one scan settles every open class (the rows of the table do not decrease).
// hit(i, p, h): called at a MOVING pose (i < st) with the sample, the pose and the mask h != 0 of the classes first hit at it, before
// they leave `open` (fo_hidden_brake_impact_lanes.hpp prices them there); hits of a standing ego are not handed over.  The default
// does nothing and leaves no code.
struct HbuNoHit { __device__ __forceinline__ void operator()(int, const HbPose &, unsigned) const {} };
template <int NC, int NK, class Args, class H = HbuNoHit>
__device__ __forceinline__ void hbu_walk(const Args &a, const double *X, const int32_t *TH, int Lm, int b, double vb, double a_brake, int st,
                                         const HbuMasks &mk, const HrBox &sb, int (&bf)[NC], H &&hit = H()) {
  const int T = a.T, last = Lm - 1;
  const double *Y = X + T, *C = Y + T, *S = C + T, *ARC = S + T;
  const double arc_end = ARC[last];
  const unsigned cm1 = mk.cm1, cm2 = mk.cm2;
#pragma unroll
  for (int c = 0; c < NC; ++c) bf[c] = -1;
  double s = ARC[b];
  int j = 0;
  unsigned open = mk.every;
  for (int i = b + 1; i < Lm; ++i) {
    const HbPose p = hb_pose_step(X, Y, C, S, ARC, Lm, last, arc_end, vb, a_brake, a.dt, i, b, s, j);
    const bool open1 = (open & cm1) != 0, open2 = (open & cm2) != 0;   // maps 1, 2 still have an open class (map 0 is the scan's own)
    HbuKeys q{HC_NONE, HC_NONE, HC_NONE};
    fo_hr_scan_pose_rows(a, p.x, p.y, p.c, p.s, a.key0, HC_NONE, sb.lox, sb.loy, sb.hix, sb.hiy, 0, 1, [&](int kv, int gx, int gy) {
      q.q0 = q.q0 < kv ? q.q0 : kv;
      if constexpr (NK > 1) {
        const int wx = gx - a.ix0, wy = gy - a.iy0;
        const bool in = wx >= 0 && wx < a.nx && wy >= 0 && wy < a.ny;
        if (open1) {
          const int vk = in ? a.key1[wy * a.nx + wx] : kv;      // outside the window: 0 or NONE, the same for every map
          q.q1 = q.q1 < vk ? q.q1 : vk;
        }
        if constexpr (NK > 2) {
          if (open2) {
            const int vk = in ? a.key2[wy * a.nx + wx] : kv;
            q.q2 = q.q2 < vk ? q.q2 : vk;
          }
        }
      }
    });
    if (i >= st) {                      // the ego stands: this pose is the manoeuvre's last one, hit_c(i') for i' >= i iff q <= thr[c][i']
      for (int at = i; at <= last && open; ++at) {       // the same minima against the samples that remain
        const unsigned h = hbu_hits<NC, NK>(q, TH, T, at, open, cm1, cm2);
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (h >> c & 1u) bf[c] = at;
        open &= ~h;
      }
      break;
    }
    const unsigned h = hbu_hits<NC, NK>(q, TH, T, i, open, cm1, cm2);
    if (h) hit(i, p, h);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (h >> c & 1u) bf[c] = i;
    open &= ~h;
    if (!open) break;
  }
}

// dynamic LDS: brake_users_lds_bytes(T, K, C)
template <int NC, int NK>
__global__ __launch_bounds__(HB_THREADS) void fo_hr_brake_users_kernel(const HrBrakeUsersArgs a, const HbThr thr) {
  extern __shared__ double hbu_rows[];  // per trajectory of the workgroup x, y, cos, sin, arc, v (T float64 each); then qmin per map, then thr
  const int G = a.G, T = a.T, nc = a.C, per_block = HB_THREADS / G;
  const int sub = threadIdx.x / G, kl = threadIdx.x & (G - 1);
  const long long m0 = (long long)blockIdx.x * per_block, m = m0 + sub;
  const bool live = m < a.M;
  int32_t *QM = (int32_t *)(hbu_rows + (size_t)per_block * 6 * T);   // [NK][per_block][T]
  int32_t *TH = QM + (size_t)NK * per_block * T;                     // [C][T]
  hbu_stage<NK>(a, hbu_rows, QM, TH, m0, per_block, [&](int t) { return thr.v[t]; });
  __syncthreads();
  const double *X = hbu_rows + (size_t)sub * 6 * T, *V = X + 5 * T;
  const int Lm = live ? hb_length(a, m) : 0;
  const HbuMasks mk = hbu_masks<NC>(a.map_of, nc);
  int fm[NC];                           // the lanes of the trajectory split its samples
  hbu_first<NC, NK>(QM + (size_t)sub * T, (size_t)per_block * T, TH, T, Lm, kl, G, mk, fm);
  const HrBox sb = fo_hr_scan_box(a);
  int commit[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) commit[c] = 0x7fffffff;
  for (int b = kl; b < T; b += G) {
    int bf[NC], st = -1;
#pragma unroll
    for (int c = 0; c < NC; ++c) bf[c] = -1;
    if (b < Lm) {                       // (Lm = 0 on lanes without a trajectory)
      const double vb = V[b];
      st = hb_stop_sample(vb, a.a_brake, a.dt, b, Lm);
      hbu_walk<NC, NK>(a, X, TH, Lm, b, vb, a.a_brake, st, mk, sb, bf);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (hb_unclear(fm[c], b, bf[c], st)) commit[c] = commit[c] < b ? commit[c] : b;
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) a.brake_first[((size_t)c * a.M + (size_t)m) * T + b] = bf[c];
      a.stop[(size_t)m * T + b] = st;
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hb_shfl_min(commit[c], 1, G);       // lanes of a trajectory are G consecutive lanes of one wave
    if (live && kl == 0 && c < nc) {
      a.commit[(size_t)c * a.M + (size_t)m] = commit[c] == 0x7fffffff ? -1 : commit[c];
      a.first[(size_t)c * a.M + (size_t)m] = fm[c];
    }
  }
}

// The launch of a users-family kernel for K maps: k1, k2, k3 are its instantiations NK = 1, 2, 3 at one class width
template <class A, class P>
void hbu_launch_maps(int K, void (*k1)(A, P), void (*k2)(A, P), void (*k3)(A, P), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                     const A &a, const P &p) {
  void (*const kernel)(A, P) = K == 1 ? k1 : (K == 2 ? k2 : k3);
  hipLaunchKernelGGL(kernel, grid, block, lds, s, a, p);
}

template <int NC>
void hbu_launch(int K, dim3 grid, dim3 block, size_t lds, hipStream_t s, const HrBrakeUsersArgs &a, const HbThr &thr) {
  hbu_launch_maps(K, fo_hr_brake_users_kernel<NC, 1>, fo_hr_brake_users_kernel<NC, 2>, fo_hr_brake_users_kernel<NC, 3>,
                  grid, block, lds, s, a, thr);
}

}  // namespace
