// fo_future_visibility.hpp -- fo_future_visibility_kernel (an extension: what a candidate trajectory will come to see), its
// argument struct and the choice of its <RPT, SECTOR, FS> form (launch_future_visibility).  Part of the one translation
// unit fo_scene.hip.
#pragma once
#include "fo_scene_rays.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ future visibility
// An extension, NOT part of the reference: how much of the currently occluded area a candidate trajectory
// will come to see.  A workgroup per pose (trajectory m, every t_stride-th sample k): (1) the 64-piece chunks whose box
// lies within r of the pose are listed in LDS; (2) a thread per ray of the fan walks that list -- per-ray box culling,
// and a wave whose rays all miss a chunk skips it -- keeping the first hit against the map and the pose's occluder
// slice; (3) shoelace area of the polygon of hit points; (4) the cells of the current occluded set are tested against the
// fan (chord rule of the cell-grid kernel) and counted.  Ranges never leave LDS.
// fo_scene_future_visibility is the form <RPT, false, false> with one slice and a world-aligned full fan.  The extended
// entry adds: per-pose occluder slices; a fan rotated per pose by a given heading (float64, no contraction: this file is
// built with -ffp-contract=off), open when SECTOR (open shoelace sum, fan_sector(full = 0) lookup); and with FS a
// workgroup per TRAJECTORY that walks its poses in order and keeps a "seen" bit per occluded-list entry in LDS, so that
// it can count the cells a pose sees for the first time.  Bit j of thread t's word w stands for list entry
// t + 256 (32 w + j): every bit belongs to the thread that tests that entry, so the set needs no atomics.
// (FV_THREADS = 256 threads per pose: fo_scene_plan.hpp; a thread walks RPT rays (tid, tid + 256, ...): RPT = ceil(n_rays / 256))
constexpr int FV_MAX_RPT = 3;     // <= 768 rays: the 720-ray fan of BASELINE configs[2] (0.5 deg) fits (round 6; 256 before)
constexpr int FV_BATCH = 48;      // 16-piece quarters staged in LDS at a time (24 KB)
constexpr int FV_SEEN_CELLS = 32 * FV_THREADS;   // list entries per word row of the seen set (one 1 KB row)
static_assert(FO_FUTURE_VISIBILITY_MAX_CELLS % FV_SEEN_CELLS == 0, "seen-set capacity: whole word rows");
struct FvArgs {
  int T, t_stride, K, n_rays;
  const double *x, *y, *dirs, *heading;   // heading [M][K][2] or null (world-aligned)
  double r;
  int E;
  const double *edges, *sub_box;
  int O, n_slices;                        // slice s: ocorn + 8 O s, oflags + O s; pose k reads min(k, n_slices - 1)
  const double *ocorn;
  const uint8_t *oflags;
  const int32_t *occ_idx, *n_occ_ptr;
  double rx0, ry0, cs;
  int ix0, iy0, nx;
  int32_t *revealed;
  double *area;
  int32_t *revealed_new, *revealed_any;   // FS only (either may be null)
};
template <int RPT, bool SECTOR, bool FS>
__global__ __launch_bounds__(FV_THREADS) void fo_future_visibility_kernel(const FvArgs a) {
  __shared__ double s_dir[2 * FV_THREADS * RPT];
  __shared__ double s_rng[FV_THREADS * RPT];
  __shared__ double s_seg[FV_BATCH][64];    // 16 pieces x (ax, ay, bx, by) per staged quarter
  __shared__ float s_box[FV_BATCH][4];      // their boxes relative to the pose (float, grown by 1 mm)
  __shared__ int s_ch[FV_BATCH];
  __shared__ int s_nob;
  __shared__ double s_ob[64][8];            // corner rows of the obstacles within reach (64 at a time)
  __shared__ double s_red[FV_THREADS / 64];
  __shared__ int s_cnt[FV_THREADS / 64];
  __shared__ int s_new[FV_THREADS / 64];
  extern __shared__ uint32_t s_seen[];      // FS: [rows][FV_THREADS], rows = ceil(n_occ / FV_SEEN_CELLS)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_rays = a.n_rays, E = a.E, K = a.K;
  const double r = a.r;
  const int m = FS ? (int)blockIdx.x : (int)blockIdx.x / K;
  const int k_begin = FS ? 0 : (int)blockIdx.x % K, k_end = FS ? K : k_begin + 1;
  const int n_occ = *a.n_occ_ptr;
  if (FS)
    for (int w = tid; w < (n_occ + FV_SEEN_CELLS - 1) / FV_SEEN_CELLS * FV_THREADS; w += FV_THREADS) s_seen[w] = 0u;
  int n_any = 0;
  for (int k = k_begin; k < k_end; ++k) {
  const size_t pose = (size_t)m * K + k;
  const int sl = k < a.n_slices ? k : a.n_slices - 1;
  const double *__restrict__ ocorn = a.ocorn + 8 * (size_t)a.O * sl;
  const uint8_t *__restrict__ oflags = a.oflags + (size_t)a.O * sl;
  const double px = a.x[(size_t)m * a.T + (size_t)k * a.t_stride], py = a.y[(size_t)m * a.T + (size_t)k * a.t_stride];
  if (FS) __syncthreads();   // the previous pose is done with s_dir / s_rng / s_red / s_cnt
  if (a.heading) {
    const double hc = a.heading[2 * pose], hs = a.heading[2 * pose + 1];
    for (int i = tid; i < n_rays; i += FV_THREADS) {
      const double ux = a.dirs[2 * i], uy = a.dirs[2 * i + 1];
      s_dir[2 * i] = hc * ux - hs * uy;
      s_dir[2 * i + 1] = hs * ux + hc * uy;
    }
  } else {
    for (int i = tid; i < n_rays; i += FV_THREADS) { s_dir[2 * i] = a.dirs[2 * i]; s_dir[2 * i + 1] = a.dirs[2 * i + 1]; }
  }
  __syncthreads();
  // ray u of this thread: index tid + 256 u
  bool ray[RPT];
  double dx[RPT], dy[RPT], best[RPT];
#pragma unroll
  for (int u = 0; u < RPT; ++u) {
    const int i = tid + u * FV_THREADS;
    ray[u] = i < n_rays;
    dx[u] = ray[u] ? s_dir[2 * i] : 1.0;
    dy[u] = ray[u] ? s_dir[2 * i + 1] : 0.0;
    best[u] = INFINITY;
  }
  // (1) + (2): the 16-piece quarters whose box lies within r of the pose are listed FV_BATCH at a time, staged in LDS
  // by the whole workgroup (one exposed round trip per batch), and every ray walks the staged list: box culling per
  // ray, 16 segment tests per surviving quarter, all operands LDS broadcasts
  const int nq = (E + 15) >> 4;
  const double rr = r + 1e-7;
  const size_t n_dbl = 4 * (size_t)E;
  auto in_reach = [&](int c) {
    const double *b = a.sub_box + 4 * (size_t)c;
    const double ddx = fmax(fmax(b[0] - px, px - b[2]), 0.0), ddy = fmax(fmax(b[1] - py, py - b[3]), 0.0);
    return ddx * ddx + ddy * ddy <= rr * rr;   // an empty box (inf, -inf) is never in reach
  };
  // rank of every quarter in reach (thread-major order): per-thread count, then an exclusive prefix over the workgroup
  int mine = 0;
  for (int c = tid; c < nq; c += FV_THREADS) mine += in_reach(c) ? 1 : 0;
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) s_cnt[wave] = incl;
  __syncthreads();
  int offset = incl - mine, n_total = 0;
  for (int w = 0; w < FV_THREADS / 64; ++w) {
    if (w < wave) offset += s_cnt[w];
    n_total += s_cnt[w];
  }
  __syncthreads();
  for (int b0 = 0; b0 < n_total; b0 += FV_BATCH) {
    int rk = offset;
    for (int c = tid; c < nq; c += FV_THREADS)
      if (in_reach(c)) {
        if (rk >= b0 && rk < b0 + FV_BATCH) s_ch[rk - b0] = c;
        ++rk;
      }
    __syncthreads();
    const int nch = n_total - b0 < FV_BATCH ? n_total - b0 : FV_BATCH;
    // stage: four quarters per pass (thread -> quarter tid / 64, double tid % 64), loads back to back
    for (int base = 0; base < nch; base += 4) {
      const int slot = base + (tid >> 6);
      if (slot < nch) {
        const size_t g = 64 * (size_t)s_ch[slot] + (tid & 63);
        s_seg[slot][tid & 63] = g < n_dbl ? a.edges[g] : 0.0;
        if ((tid & 63) < 4) {  // box relative to the pose, in float, grown by 1 mm (>> float rounding at map scale)
          const int u = tid & 63;
          const double v = a.sub_box[4 * (size_t)s_ch[slot] + u] - ((u & 1) ? py : px);
          s_box[slot][u] = (float)v + (u < 2 ? -1e-3f : 1e-3f);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RPT; ++u)
    if (ray[u]) {
      // the ray segment [0, r d] against the staged boxes, all in pose-relative float: bounding boxes, then "all four
      // corners on one side of the ray's line" (1 mm margins; culling is conservative, it never changes a result)
      const float fdx = (float)dx[u], fdy = (float)dy[u], fr = (float)r * 1.000001f;
      const float ex_ = fr * fdx, ey_ = fr * fdy;
      const float sx0 = fminf(0.0f, ex_) - 1e-3f, sx1 = fmaxf(0.0f, ex_) + 1e-3f;
      const float sy0 = fminf(0.0f, ey_) - 1e-3f, sy1 = fmaxf(0.0f, ey_) + 1e-3f;
      for (int q = 0; q < nch; ++q) {
        const float bx0 = s_box[q][0], by0 = s_box[q][1], bx1 = s_box[q][2], by1 = s_box[q][3];
        if (bx0 > sx1 || bx1 < sx0 || by0 > sy1 || by1 < sy0) continue;
        const float c00 = fdx * by0 - fdy * bx0, c10 = fdx * by0 - fdy * bx1;
        const float c01 = fdx * by1 - fdy * bx0, c11 = fdx * by1 - fdy * bx1;
        const float mm = 2e-3f;
        if ((c00 > mm && c10 > mm && c01 > mm && c11 > mm) || (c00 < -mm && c10 < -mm && c01 < -mm && c11 < -mm)) continue;
        const int e_first = s_ch[q] << 4;
        const int cnt = E - e_first < 16 ? E - e_first : 16;
        const double *buf = s_seg[q];
        for (int e = 0; e < cnt; ++e) {
          const double t = ray_segment(px, py, dx[u], dy[u], buf[4 * e], buf[4 * e + 1], buf[4 * e + 2], buf[4 * e + 3]);
          best[u] = t < best[u] ? t : best[u];
        }
      }
    }
    __syncthreads();
  }
  // obstacles within reach: corner rows staged in LDS (64 at a time)
  for (int base = 0; base < a.O; base += 64) {
    __syncthreads();
    if (tid == 0) s_nob = 0;
    __syncthreads();
    const int o = base + tid;
    if (tid < 64 && o < a.O && (oflags[o] & 1) && (oflags[o] & 2)) {
      const double *c = ocorn + 8 * (size_t)o;
      const double mx = 0.5 * (c[0] + c[4]), my = 0.5 * (c[1] + c[5]);
      const double hd2 = (c[0] - mx) * (c[0] - mx) + (c[1] - my) * (c[1] - my);
      const double d2c = (px - mx) * (px - mx) + (py - my) * (py - my);
      // nearer than r + half diagonal ((r + hd)^2 <= r^2 + r (1 + hd2) + hd2; a pure early-out)
      if (d2c <= r * r + r * (1.0 + hd2) + hd2 + 1e-6) {
        const int slot = atomicAdd(&s_nob, 1);
#pragma unroll
        for (int u = 0; u < 8; ++u) s_ob[slot][u] = c[u];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RPT; ++u)
    if (ray[u]) {
      for (int q = 0; q < s_nob; ++q) {
        const double *c = s_ob[q];
        {  // per-ray early-out: the obstacle's circumscribed circle misses the ray segment (margin as for the boxes)
          const double mx = 0.5 * (c[0] + c[4]) - px, my = 0.5 * (c[1] + c[5]) - py;
          const double hd2 = (c[0] - px - mx) * (c[0] - px - mx) + (c[1] - py - my) * (c[1] - py - my);
          const double cr = dx[u] * my - dy[u] * mx, al = dx[u] * mx + dy[u] * my;      // offset from the line, position along it
          const double lim = hd2 + 1e-6 * (1.0 + hd2);
          if (cr * cr > lim || (al < 0.0 && al * al > lim) || (al > r && (al - r) * (al - r) > lim)) continue;
        }
#pragma unroll
        for (int sd = 0; sd < 4; ++sd) {
          const int s2 = (sd + 1) & 3;
          const double t = ray_segment(px, py, dx[u], dy[u], c[2 * sd], c[2 * sd + 1], c[2 * s2], c[2 * s2 + 1]);
          best[u] = t < best[u] ? t : best[u];
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < RPT; ++u) {
    if (!(best[u] <= r)) best[u] = r;
    if (ray[u]) s_rng[tid + u * FV_THREADS] = best[u];
  }
  __syncthreads();
  // (3) shoelace area of the polygon of hit points (an open fan: pose + hit points, the two edges at the pose add
  // nothing): per-thread terms (its rays in ascending order), fixed-order tree sum
  double term = 0.0;
#pragma unroll
  for (int u = 0; u < RPT; ++u)
    if (ray[u] && !(SECTOR && tid + u * FV_THREADS == n_rays - 1)) {
      const int i = tid + u * FV_THREADS, j = (i + 1 == n_rays) ? 0 : i + 1;
      const double hix = s_rng[i] * s_dir[2 * i], hiy = s_rng[i] * s_dir[2 * i + 1];
      const double hjx = s_rng[j] * s_dir[2 * j], hjy = s_rng[j] * s_dir[2 * j + 1];
      term += hix * hjy - hjx * hiy;
    }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) term += __shfl_xor(term, off);
  if (lane == 0) s_red[wave] = term;
  // (4) occluded cells inside the fan
  const double r2 = r * r;
  int cnt = 0, nw = 0;
  auto inside_fan = [&](int idx) -> int {
    const int wx = a.ix0 + idx % a.nx, wy = a.iy0 + idx / a.nx;
    const double cx = a.rx0 + ((double)wx + 0.5) * a.cs, cy = a.ry0 + ((double)wy + 0.5) * a.cs;
    const double qx = cx - px, qy = cy - py;
    if (qx * qx + qy * qy > r2) return 0;
    if (qx == 0.0 && qy == 0.0) return 1;
    const int i = SECTOR ? fan_sector(n_rays, s_dir, 0, qx, qy) : fan_sector_uniform(n_rays, s_dir, qx, qy);
    if (i < 0) return 0;
    const int j = (i + 1 == n_rays) ? 0 : i + 1;
    const double hix = s_rng[i] * s_dir[2 * i], hiy = s_rng[i] * s_dir[2 * i + 1];
    const double hjx = s_rng[j] * s_dir[2 * j], hjy = s_rng[j] * s_dir[2 * j + 1];
    return ((hjx - hix) * (qy - hiy) - (hjy - hiy) * (qx - hix) >= 0.0) ? 1 : 0;
  };
  if (FS) {
    // entry ci = tid + 256 (32 w + b): bit b of this thread's word w; seen by an earlier pose = set
    for (int w = 0; w * FV_SEEN_CELLS + tid < n_occ; ++w) {
      uint32_t bits = s_seen[w * FV_THREADS + tid];
      const uint32_t before = bits;
      for (int b = 0; b < 32; ++b) {
        const int ci = tid + (32 * w + b) * FV_THREADS;
        if (ci >= n_occ) break;
        if (inside_fan(a.occ_idx[ci])) { ++cnt; bits |= 1u << b; }
      }
      nw += __popc(bits & ~before);
      s_seen[w * FV_THREADS + tid] = bits;
    }
  } else {
    // four cell indices per thread in flight (the list is read once per pose; the loads are what the loop waits for)
    int ci = tid;
    for (; ci + 3 * FV_THREADS < n_occ; ci += 4 * FV_THREADS) {
      const int i0 = a.occ_idx[ci], i1 = a.occ_idx[ci + FV_THREADS], i2 = a.occ_idx[ci + 2 * FV_THREADS],
                i3 = a.occ_idx[ci + 3 * FV_THREADS];
      cnt += inside_fan(i0) + inside_fan(i1) + inside_fan(i2) + inside_fan(i3);
    }
    for (; ci < n_occ; ci += FV_THREADS) cnt += inside_fan(a.occ_idx[ci]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) s_cnt[wave] = cnt;
  if (FS) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nw += __shfl_xor(nw, off);
    if (lane == 0) s_new[wave] = nw;
  }
  __syncthreads();
  if (tid == 0) {
    double a2 = 0.0;
    int total = 0, fresh = 0;
    for (int w = 0; w < FV_THREADS / 64; ++w) {
      a2 += s_red[w];
      total += s_cnt[w];
      if (FS) fresh += s_new[w];
    }
    a.area[pose] = 0.5 * a2;
    a.revealed[pose] = total;
    if (FS) {
      if (a.revealed_new) a.revealed_new[pose] = fresh;
      n_any += fresh;
    }
  }
  }
  if (FS && tid == 0 && a.revealed_any) a.revealed_any[m] = n_any;
}

// launch of fo_future_visibility_kernel: RPT by the ray count, the open-fan and first-seen forms by the caller
int launch_future_visibility(fo_ctx *ctx, const FvArgs &a, int M, bool sector, bool fs, size_t seen_bytes, void *stream) {
  const int rpt = fv_rays_per_thread(a.n_rays);
  const dim3 grid((unsigned)(fs ? (size_t)M : (size_t)M * a.K)), block(FV_THREADS);
  const size_t lds = fs ? seen_bytes : 0;
  hipStream_t st = (hipStream_t)stream;
#define FO_LAUNCH_FV(RPT_, SEC_, FS_) hipLaunchKernelGGL((fo_future_visibility_kernel<RPT_, SEC_, FS_>), grid, block, lds, st, a)
#define FO_LAUNCH_FV_RPT(SEC_, FS_)                                                      \
  do {                                                                                   \
    if (rpt == 1) FO_LAUNCH_FV(1, SEC_, FS_); else if (rpt == 2) FO_LAUNCH_FV(2, SEC_, FS_); else FO_LAUNCH_FV(3, SEC_, FS_); \
  } while (0)
  if (sector) { if (fs) FO_LAUNCH_FV_RPT(true, true); else FO_LAUNCH_FV_RPT(true, false); }
  else { if (fs) FO_LAUNCH_FV_RPT(false, true); else FO_LAUNCH_FV_RPT(false, false); }
#undef FO_LAUNCH_FV_RPT
#undef FO_LAUNCH_FV
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

}  // namespace
