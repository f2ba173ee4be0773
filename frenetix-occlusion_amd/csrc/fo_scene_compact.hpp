// fo_scene_compact.hpp -- flags -> ascending index list: fo_flag_compact_kernel (one launch), fo_flag_scan_kernel +
// fo_flag_scatter_kernel (very large windows), the phantom sampler's candidate flags (fo_spawn_flag_kernel, or inside the
// compaction) and the choice between the one- and the two-launch form (compact).  Part of the one translation unit
// fo_scene.hip.
#pragma once
#include "fo_scene_plan.hpp"
#include "fo_scene_state.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ compaction
// flags[n] (+ per-256 block counts from the producing kernel) -> ascending index list + count; two launches, no
// atomics (deterministic order)
__global__ __launch_bounds__(1024) void fo_flag_scan_kernel(int32_t *__restrict__ blk, int nb,
                                                            int32_t *__restrict__ total) {
  __shared__ int sh[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? blk[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int add = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < nb) blk[i] = carry + sh[threadIdx.x] - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry += sh[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void fo_flag_scatter_kernel(const uint8_t *__restrict__ flags, int n,
                                                              const int32_t *__restrict__ blk,
                                                              int32_t *__restrict__ out) {
  __shared__ int wsum[4];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool f = idx < n && flags[idx];
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int off = blk[blockIdx.x];
  for (int k = 0; k < w; ++k) off += wsum[k];
  if (f) out[off + before] = idx;
}

// candidate cells of the phantom sampler: occluded, on the front towards the visible area (or anywhere when
// all_occluded), ahead of the ego and within max_dist -- flags + per-block counts for the compaction that follows
struct SpawnFlagArgs {
  int on = 0;
  const uint8_t *cls = nullptr;
  int nx = 0, ny = 0, ix0 = 0, iy0 = 0, all_occluded = 0;
  double rx0 = 0, ry0 = 0, cs = 0, ex = 0, ey = 0, hx = 0, hy = 0, min_ahead = 0, max_dist = 0;
  uint8_t *flag = nullptr;
  int32_t *blk = nullptr;
};
// (whole 256-thread block; wsum: four ints of LDS)
__device__ __forceinline__ void spawn_flag_block(const SpawnFlagArgs &a, int *wsum) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool in = idx < a.nx * a.ny;
  const int ix = in ? idx % a.nx : 0, iy = in ? idx / a.nx : 0;
  const uint8_t *__restrict__ cls = a.cls;
  uint8_t f = 0;
  if (in && (cls[idx] & 4)) {
    int front = a.all_occluded;
    if (ix > 0 && (cls[idx - 1] & 2)) front = 1;
    if (ix + 1 < a.nx && (cls[idx + 1] & 2)) front = 1;
    if (iy > 0 && (cls[idx - a.nx] & 2)) front = 1;
    if (iy + 1 < a.ny && (cls[idx + a.nx] & 2)) front = 1;
    if (front) {
      const double px = a.rx0 + ((double)(a.ix0 + ix) + 0.5) * a.cs, py = a.ry0 + ((double)(a.iy0 + iy) + 0.5) * a.cs;
      const double rx = px - a.ex, ry = py - a.ey;
      if (!(rx * a.hx + ry * a.hy < a.min_ahead) && !(rx * rx + ry * ry > a.max_dist * a.max_dist)) f = 1;
    }
  }
  if (in) a.flag[idx] = f;
  const unsigned long long b = __ballot(f != 0);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) a.blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One-launch variant for the usual window sizes (a few hundred blocks): every block sums the counts of the blocks
// before it itself (a few hundred L2-resident ints) instead of waiting for a separate scan launch; same output.
// sf.on (fo_step_run): the same launch also flags the phantom sampler's candidate cells for the compaction after this
// one -- into buffers of their own, this compaction's flags and counts are still being read by other blocks.
__global__ __launch_bounds__(256) void fo_flag_compact_kernel(const uint8_t *__restrict__ flags, int n,
                                                              const int32_t *__restrict__ cnt,
                                                              int32_t *__restrict__ out, int32_t *__restrict__ total,
                                                              SpawnFlagArgs sf) {
  __shared__ int wsum[4], psum[4];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool f = idx < n && flags[idx];
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  int part = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += 256) part += cnt[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) { wsum[w] = __popcll(b); psum[w] = part; }
  __syncthreads();
  int off = psum[0] + psum[1] + psum[2] + psum[3];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = off + wsum[0] + wsum[1] + wsum[2] + wsum[3];
  for (int k = 0; k < w; ++k) off += wsum[k];
  if (f) out[off + before] = idx;
  if (sf.on) {
    __syncthreads();   // (wsum is used again)
    spawn_flag_block(sf, wsum);
  }
}

// ------------------------------------------------------------------------------------------------ spawn sampling
__global__ __launch_bounds__(256) void fo_spawn_flag_kernel(SpawnFlagArgs a) {
  __shared__ int wsum[4];
  spawn_flag_block(a, wsum);
}

// flags -> ascending indices (out) + count (d_total)
// (sf: candidate flags of the phantom sampler in the same launch, fo_step_run; *sf_done says whether that happened)
// Up to 2048 blocks of 256 cells: the one-launch kernel.  Beyond that -- a window of 725 x 725 cells or more, which at the 0.5 m
// cell is any sensor radius above 120.5 m (SensorModel._window_for: ceil(3 r / cs) + 1 cells per side) -- the scan + scatter
// pair, and the caller flags the sampler's candidates in a launch of its own.  tests/test_scene_forms_gpu.py runs both sides.
int compact(fo_ctx *ctx, Scene *sc, const uint8_t *flags, const int32_t *blk, int n, int32_t *out, int32_t *d_total,
            hipStream_t s, const SpawnFlagArgs *sf = nullptr, bool *sf_done = nullptr) {
  const int nb = (n + 255) / 256;  // block counts were written by the kernel that produced the flags
  if (sf_done) *sf_done = false;
  if (!compact_two_launches(n)) {
    SpawnFlagArgs a;
    if (sf) { a = *sf; if (sf_done) *sf_done = true; }
    hipLaunchKernelGGL(fo_flag_compact_kernel, dim3(nb), dim3(256), 0, s, flags, n, blk, out, d_total, a);
  } else {
    hipLaunchKernelGGL(fo_flag_scan_kernel, dim3(1), dim3(1024), 0, s, const_cast<int32_t *>(blk), nb, d_total);
    hipLaunchKernelGGL(fo_flag_scatter_kernel, dim3(nb), dim3(256), 0, s, flags, n, blk, out);
  }
  FO_HIP_TRY(ctx, hipGetLastError());
  return FO_OK;
}

}  // namespace
