// fo_scene_grid.hpp -- the cell half of the scene stage's chain: fo_raster_kernel (the one-off road raster), fo_grid_kernel
// (class bits per window cell), fo_settle_kernel (the cells the fan cannot decide, the obstacles' 5 mm skins) and the choice
// of its <SKIP, NW> form (launch_settle).  Part of the one translation unit fo_scene.hip.
#pragma once
#include "fo_scene_rays.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ road raster
__global__ void fo_raster_kernel(int P, const int32_t *__restrict__ poly_off, const double *__restrict__ poly_xy,
                                 const double *__restrict__ pbox, double x0, double y0, double cs, int nx, int ny,
                                 uint8_t *__restrict__ mask) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nx * ny) return;
  const int ix = idx % nx, iy = idx / nx;
  const double px = x0 + ((double)ix + 0.5) * cs, py = y0 + ((double)iy + 0.5) * cs;
  int inside_any = 0;
  for (int p = 0; p < P && !inside_any; ++p) {
    const double *bb = pbox + 4 * (size_t)p;  // xmin, ymin, xmax, ymax: pure early-out, cannot change the result
    if (px < bb[0] || px > bb[2] || py < bb[1] || py > bb[3]) continue;
    const int b = poly_off[p], e = poly_off[p + 1];
    int c = 0;
    for (int i = b, j = e - 1; i < e; j = i++) {
      const double xi = poly_xy[2 * i], yi = poly_xy[2 * i + 1], xj = poly_xy[2 * j], yj = poly_xy[2 * j + 1];
      if ((yi > py) != (yj > py)) {
        const double xc = xi + (py - yi) * (xj - xi) / (yj - yi);
        if (px < xc) c ^= 1;
      }
    }
    inside_any = c;
  }
  mask[idx] = (uint8_t)inside_any;
}

// The reference's 1.5 r half disc is the 100-point fan of _calc_relevant_sector (sensor_model.py:85-87,201-209).  A
// centre in the thin rim between that polygon and the circle (d2 above 0.9994 ro2; the polygon's inscribed radius
// squared is 0.99975 ro2) is tested against the chord of its sector; half = its 100 unit directions or null.
__device__ __forceinline__ int in_half_fan(const double *__restrict__ half, double r, double rx, double ry, double d2,
                                           double ro2) {
  if (!half || !(d2 > 0.9994 * ro2)) return 1;
  const int k = fan_search(100, half, 0, 99, rx, ry);
  if (k < 0) return 1;
  const double R = 1.5 * r;
  const double ax = R * half[2 * k], ay = R * half[2 * k + 1];
  const double bx = R * half[2 * k + 2], by = R * half[2 * k + 3];
  return ((bx - ax) * (ry - ay) - (by - ay) * (rx - ax)) >= 0.0;
}

// sensor_model.py:183: the obstacle rectangle grown by 5 mm (mitred corners) is taken out of the visible area.  Inside
// iff the signed distance to each side is <= 5 mm: cross(e, q - a) against 0.005 |e|, either ring orientation;
// present, non-bicycle obstacles only.
__device__ __forceinline__ int in_obstacle_skin(int O, const double *__restrict__ ocorn,
                                                const uint8_t *__restrict__ oflags, double px, double py) {
  for (int o = 0; o < O; ++o) {
    if (!(oflags[o] & 1) || !(oflags[o] & 2)) continue;
    const double *c = ocorn + 8 * (size_t)o;
    {  // pure early-out: farther from the rectangle's centre than its grown half diagonal (hd + 0.005 sqrt 2)
      const double mx = 0.5 * (c[0] + c[4]), my = 0.5 * (c[1] + c[5]);
      const double hd2 = (c[0] - mx) * (c[0] - mx) + (c[1] - my) * (c[1] - my);
      const double d2c = (px - mx) * (px - mx) + (py - my) * (py - my);
      if (d2c > hd2 + 0.0071 * (1.0 + hd2) + 1e-4) continue;
    }
    const double area2 = (c[2] - c[0]) * (c[5] - c[1]) - (c[3] - c[1]) * (c[4] - c[0]);
    const double sg = area2 >= 0.0 ? 1.0 : -1.0;
    int inside = 1;
    for (int sd = 0; sd < 4 && inside; ++sd) {
      const int s2 = (sd + 1) & 3;
      const double ex = c[2 * s2] - c[2 * sd], ey = c[2 * s2 + 1] - c[2 * sd + 1];
      const double cr = ex * (py - c[2 * sd + 1]) - ey * (px - c[2 * sd]);
      if (-(sg * cr) > 0.005 * sqrt(ex * ex + ey * ey)) inside = 0;
    }
    if (inside) return 1;
  }
  return 0;
}

// Where an obstacle's shadow ENDS in the reference (helper_functions.py:139-176): the occlusion polygon is the quad
// [c1, c2, c2 + L u(c2 - ego), c1 + L u(c1 - ego)], L = 100 m, with (c1, c2) the corner pair that subtends the largest angle
// at the ego (_identify_projection_points: all 4 x 4 ordered pairs, arccos of the clipped dot product of the unit vectors,
// strictly greater wins, first in loop order).  Beyond the chord between the two end points the obstacle hides nothing.
// out[3] = (a, b, c): a point lies beyond that chord iff a x + b y + c > 0 (the ego on the other side); a = b = 0, c = -1
// when there is no such chord (length <= 0 or infinite: shadows without end, or a degenerate view).
// Sixteen consecutive lanes per obstacle (q = lane & 15 = the ordered corner pair i = q >> 2, j = q & 3): one arccos per lane
// instead of a chain of sixteen; the largest angle with the smallest q among equals = the reference's "strictly greater, first
// in loop order".  Every lane of the group must call; lane q == 0 writes.
__device__ inline void wedge_far_halfplane(int q, double ex, double ey, const double *__restrict__ c, double length, double *out) {
  const bool on = length > 0.0 && length < INFINITY;
  const int i = q >> 2, j = q & 3;
  double ang;
  {
    const double r1x = c[2 * i] - ex, r1y = c[2 * i + 1] - ey, r2x = c[2 * j] - ex, r2y = c[2 * j + 1] - ey;
    const double n1 = sqrt(r1x * r1x + r1y * r1y), n2 = sqrt(r2x * r2x + r2y * r2y);
    const double u1x = r1x / n1, u1y = r1y / n1, u2x = r2x / n2, u2y = r2y / n2;
    ang = acos(fmin(fmax(u1x * u2x + u1y * u2y, -1.0), 1.0));
  }
  // (an angle that is not > 0 -- zero or NaN -- never replaces the initial "none": key -1)
  double best = ang > 0.0 ? ang : -1.0;
  int bq = ang > 0.0 ? q : 16;
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const double b2 = __shfl_xor(best, off, 16);
    const int q2 = __shfl_xor(bq, off, 16);
    if (b2 > best || (b2 == best && q2 < bq)) { best = b2; bq = q2; }
  }
  if (q != 0) return;
  out[0] = 0.0; out[1] = 0.0; out[2] = -1.0;
  if (!on || bq >= 16) return;
  const int i1 = bq >> 2, i2 = bq & 3;
  const double r1x = c[2 * i1] - ex, r1y = c[2 * i1 + 1] - ey, r2x = c[2 * i2] - ex, r2y = c[2 * i2 + 1] - ey;
  const double n1 = sqrt(r1x * r1x + r1y * r1y), n2 = sqrt(r2x * r2x + r2y * r2y);
  const double c4x = c[2 * i1] + r1x / n1 * length, c4y = c[2 * i1 + 1] + r1y / n1 * length;   // c1 + L u(c1 - ego)
  const double c3x = c[2 * i2] + r2x / n2 * length, c3y = c[2 * i2 + 1] + r2y / n2 * length;   // c2 + L u(c2 - ego)
  double a = -(c4y - c3y), b = c4x - c3x;
  double cc = -(a * c3x + b * c3y);
  const double ge = a * ex + b * ey + cc;
  if (ge == 0.0 || ge != ge) return;
  if (ge > 0.0) { a = -a; b = -b; cc = -cc; }
  out[0] = a; out[1] = b; out[2] = cc;
}

// ------------------------------------------------------------------------------------------------ cell grid
__global__ void fo_grid_kernel(const uint8_t *__restrict__ raster, int rnx, int rny, double rx0, double ry0, double cs,
                               int ix0, int iy0, int nx, int ny, double ex, double ey, double hx, double hy, double r,
                               int full, int n_rays, const double *__restrict__ dirs,
                               const double *__restrict__ range, uint8_t *__restrict__ cls,
                               uint8_t *__restrict__ occ_flag, int32_t *__restrict__ blk, int O,
                               int32_t *__restrict__ vis32, uint8_t *__restrict__ vis, int exact, int E,
                               const int32_t *__restrict__ hit_id, const double *__restrict__ rmax,
                               int32_t *__restrict__ amb, int32_t *__restrict__ n_amb,
                               const double *__restrict__ half, const int32_t *__restrict__ edge_line,
                               const double *__restrict__ ocorn, const uint8_t *__restrict__ oflags, double shadow_length,
                               double *__restrict__ ofar, int n_obst, uint8_t *__restrict__ vis_host) {
  __shared__ int wsum[4];
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  // where the obstacles' shadows end (read by the settle kernel, the next launch): sixteen lanes per obstacle
  if (ofar && ocorn && (idx >> 4) < n_obst) {   // (uniform over each group of sixteen lanes: blocks are multiples of 16)
    const int o = idx >> 4;
    if ((oflags[o] & 1) && (oflags[o] & 2)) wedge_far_halfplane(idx & 15, ex, ey, ocorn + 8 * (size_t)o, shadow_length, ofar + 3 * (size_t)o);
    else if ((idx & 15) == 0) { ofar[3 * o] = 0.0; ofar[3 * o + 1] = 0.0; ofar[3 * o + 2] = -1.0; }
  }
  if (vis && idx < O) {  // obstacle-visibility flags of the probe workgroups (previous launch); self-cleaning
    vis[idx] = vis32[idx] ? 1 : 0;
    if (vis_host) vis_host[idx] = vis32[idx] ? 1 : 0;
    vis32[idx] = 0;
  }
  const bool in = idx < nx * ny;
  uint8_t c = 0;
  bool pending = false;
  int visible = 0;
  double px = 0.0, py = 0.0, rx = 0.0, ry = 0.0, d2 = 0.0;
  const double r2 = r * r, ro2 = (1.5 * r) * (1.5 * r);
  if (in) {
    const int ix = idx % nx, iy = idx / nx;
    const int wx = ix0 + ix, wy = iy0 + iy;
    if (wx >= 0 && wx < rnx && wy >= 0 && wy < rny && raster[(size_t)wy * rnx + wx]) c |= 1;
    px = rx0 + ((double)wx + 0.5) * cs;
    py = ry0 + ((double)wy + 0.5) * cs;
    rx = px - ex;
    ry = py - ey;
    d2 = rx * rx + ry * ry;
    if ((c & 1) && d2 <= r2) {
      // (the zero vector never confirms a proposal and falls through to fan_sector's -1)
      const int i = full ? fan_sector_uniform(n_rays, dirs, rx, ry) : fan_sector(n_rays, dirs, full, rx, ry);
      if (rx == 0.0 && ry == 0.0) {
        visible = 1;
      } else if (i >= 0) {
        const int j = (i + 1 == n_rays) ? 0 : i + 1;
        const double hix = range[i] * dirs[2 * i], hiy = range[i] * dirs[2 * i + 1];
        const double hjx = range[j] * dirs[2 * j], hjy = range[j] * dirs[2 * j + 1];
        const double cr = (hjx - hix) * (ry - hiy) - (hjy - hiy) * (rx - hix);
        visible = cr >= 0.0;
        if (exact) {
          // the two enclosing rays stop at different occluders (or at an obstacle) and the centre is not nearer than
          // the shorter of them by more than a cell: the fan cannot decide (at grazing incidence the centre's own
          // ray may reach well past both); inside the footprint chord the settle kernel does
          int idi = hit_id[i], idj = hit_id[j];
          if (edge_line && idi >= 0 && idi < E && idj >= 0 && idj < E) {  // same straight chain = one occluder
            idi = edge_line[idi];
            idj = edge_line[idj];
          }
          if (idi != idj || idi >= E) {
            const double lo = range[i] < range[j] ? range[i] : range[j];
            double lom = lo - cs;
            if (lom < 0.0) lom = 0.0;
            if (d2 >= lom * lom) {
              const double fi = rmax ? rmax[i] : r, fj = rmax ? rmax[j] : r;
              const double fix = fi * dirs[2 * i], fiy = fi * dirs[2 * i + 1];
              const double fjx = fj * dirs[2 * j], fjy = fj * dirs[2 * j + 1];
              const double cf = (fjx - fix) * (ry - fiy) - (fjy - fiy) * (rx - fix);
              visible = 0;
              pending = cf >= 0.0;
            }
          }
        }
      }
    }
  }
  if (in) {
    if (visible) c |= 2;
    if ((c & 1) && !visible && !pending && d2 <= ro2 && (rx * hx + ry * hy) >= 0.0 &&
        in_half_fan(half, r, rx, ry, d2, ro2))
      c |= 4;
    cls[idx] = c;
    occ_flag[idx] = (c & 4) ? 1 : 0;
  }
  if (exact) {  // append the undecided cells (wave-aggregated; order is irrelevant, each cell is settled on its own)
    const unsigned long long pb = __ballot(pending);
    if (pb) {
      const int lane = threadIdx.x & 63;
      int base = 0;
      if (lane == 0) base = atomicAdd(n_amb, __popcll(pb));
      base = __shfl(base, 0);
      if (pending) amb[base + __popcll(pb & ((1ull << lane) - 1ull))] = idx;
    }
  }
  // block count of the occluded cells (first stage of the compaction, saves a launch)
  const unsigned long long b = __ballot(in && (c & 4));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ------------------------------------------------------------------------------------------------ settle
// The cells the fan could not decide, settled by the reference's own rule at the cell centre: the shadow quads
// [v1, v2, v2 + 100 (v2 - ego), v1 + 100 (v1 - ego)] (helper_functions.py:79-96) and the obstacle occlusion polygons
// (:133-141) contain a point iff an occluding piece crosses the open segment ego -> point.  A workgroup per cell
// (grid-stride over the list), its threads share the soup like a ray workgroup; "t < 1" along the unnormalised
// direction is decided on tn and denom, no division.  Thread 0 writes the class and keeps the per-block counts of
// the occluded-cell compaction in step.
constexpr int SETTLE_BLOCKS = 1024;  // grid of the settle kernel (grid-stride over the undecided cells)
template <bool SKIP, int NW>
__global__ __launch_bounds__(64 * NW) void fo_settle_kernel(
    int E, const double *__restrict__ edges, const double *__restrict__ chunk_box, const uint8_t *__restrict__ eskip,
    int O, const double *__restrict__ ocorn, const uint8_t *__restrict__ oflags, double rx0, double ry0, double cs, int ix0, int iy0, int nx, double ex,
    double ey, double hx, double hy, double r, const double *__restrict__ half, const int32_t *__restrict__ amb,
    const int32_t *__restrict__ n_amb, uint8_t *__restrict__ cls, uint8_t *__restrict__ occ_flag,
    int32_t *__restrict__ blk, int ny, const double *__restrict__ ofar) {
  if ((int)blockIdx.x >= SETTLE_BLOCKS) {
    // Workgroups past the cell part: one per obstacle.  sensor_model.py:183 takes the obstacle grown by 5 mm out of
    // the visible area, so a centre the grid kernel found visible inside that skin loses the bit here (the undecided
    // cells get the same test below).  The bit is cleared with a 32-bit atomic on the word holding the class byte, so
    // two obstacles with overlapping skins cannot both count the cell.
    const int o = blockIdx.x - SETTLE_BLOCKS;
    if (!((oflags[o] & 1) && (oflags[o] & 2))) return;
    const double *q = ocorn + 8 * (size_t)o;
    const double xa = fmin(fmin(q[0], q[2]), fmin(q[4], q[6])) - 0.0072, xb = fmax(fmax(q[0], q[2]), fmax(q[4], q[6])) + 0.0072;
    const double ya = fmin(fmin(q[1], q[3]), fmin(q[5], q[7])) - 0.0072, yb = fmax(fmax(q[1], q[3]), fmax(q[5], q[7])) + 0.0072;
    int ixa = (int)floor((xa - rx0) / cs - 0.5) - ix0 - 1, ixb = (int)ceil((xb - rx0) / cs - 0.5) - ix0 + 1;
    int iya = (int)floor((ya - ry0) / cs - 0.5) - iy0 - 1, iyb = (int)ceil((yb - ry0) / cs - 0.5) - iy0 + 1;
    ixa = ixa < 0 ? 0 : ixa; iya = iya < 0 ? 0 : iya;
    ixb = ixb > nx - 1 ? nx - 1 : ixb; iyb = iyb > ny - 1 ? ny - 1 : iyb;
    if (ixb < ixa || iyb < iya) return;
    const int w = ixb - ixa + 1, h = iyb - iya + 1;
    unsigned int *words = (unsigned int *)cls;
    for (int t = threadIdx.x; t < w * h; t += 64 * NW) {
      const int ix = ixa + t % w, iy = iya + t / w;
      const int idx = iy * nx + ix;
      const int sh = 8 * (idx & 3);
      if (!((words[idx >> 2] >> sh) & 2u)) continue;
      const double px = rx0 + ((double)(ix0 + ix) + 0.5) * cs, py = ry0 + ((double)(iy0 + iy) + 0.5) * cs;
      if (!in_obstacle_skin(1, q, oflags + o, px, py)) continue;
      const unsigned int old = atomicAnd(&words[idx >> 2], ~(2u << sh));
      if (!((old >> sh) & 2u)) continue;  // another obstacle's workgroup took it first
      const double rx = px - ex, ry = py - ey;
      const double d2 = rx * rx + ry * ry, ro2 = (1.5 * r) * (1.5 * r);
      if (d2 <= ro2 && (rx * hx + ry * hy) >= 0.0 && in_half_fan(half, r, rx, ry, d2, ro2)) {
        atomicOr(&words[idx >> 2], 4u << sh);
        occ_flag[idx] = 1;
        atomicAdd(&blk[idx >> 8], 1);
      }
    }
    return;
  }
  const int n = *n_amb;
  for (int k = blockIdx.x; k < n; k += SETTLE_BLOCKS) {
    const int idx = amb[k];
    const int ix = idx % nx, iy = idx / nx;
    const int wx = ix0 + ix, wy = iy0 + iy;
    const double px = rx0 + ((double)wx + 0.5) * cs, py = ry0 + ((double)wy + 0.5) * cs;
    const double rx = px - ex, ry = py - ey;
    int hit = 0;
    constexpr int stride = 64 * NW;
    auto crosses = [&](double ax, double ay, double bx, double by) -> int {
      const double sx = bx - ax, sy = by - ay;
      const double denom = rx * sy - ry * sx;
      if (denom == 0.0) return 0;
      const double wx_ = ax - ex, wy_ = ay - ey;
      const double tn = wx_ * sy - wy_ * sx;
      const double un = wx_ * ry - wy_ * rx;
      return denom > 0.0 ? (tn >= 0.0 && un >= 0.0 && un <= denom && tn < denom)
                         : (tn <= 0.0 && un <= 0.0 && un >= denom && tn > denom);
    };
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nc = (E + 63) >> 6;
    for (int cb = wave * 64; cb < nc; cb += NW * 64) {  // culled like the ray scan (segment ego -> centre)
      const int cc = cb + lane;
      unsigned long long live = __ballot(cc < nc && !chunk_culled(chunk_box + 4 * (size_t)(cc < nc ? cc : 0), ex, ey, rx, ry, 1.0));
      while (live) {
        const int c = cb + __builtin_ctzll(live);
        live &= live - 1;
        const int gi = (c << 6) + lane;
        if (gi >= E) continue;
        if (SKIP && eskip[gi]) continue;
        const double *p = edges + 4 * (size_t)gi;
        hit |= crosses(p[0], p[1], p[2], p[3]);
      }
    }
    // a centre within 5 mm of an obstacle is not visible either (sensor_model.py:183): an obstacle per thread
    for (int o = threadIdx.x; o < O; o += stride) hit |= in_obstacle_skin(1, ocorn + 8 * (size_t)o, oflags + o, px, py);
    for (int gi = threadIdx.x; gi < 4 * O; gi += stride) {
      const int o = gi >> 2, sd = gi & 3, s2 = (sd + 1) & 3;
      if (!((oflags[o] & 1) && (oflags[o] & 2))) continue;
      const double *c = ocorn + 8 * (size_t)o;
      // the obstacle hides the centre unless the centre lies beyond the end of its shadow wedge (wedge_far_halfplane)
      if (ofar && ofar[3 * o] * px + ofar[3 * o + 1] * py + ofar[3 * o + 2] > 0.0) continue;
      hit |= crosses(c[2 * sd], c[2 * sd + 1], c[2 * s2], c[2 * s2 + 1]);
    }
    int blocked = __syncthreads_or(hit);
    if (threadIdx.x == 0) {
      uint8_t c = 1;
      if (!blocked) c |= 2;
      const double d2 = rx * rx + ry * ry;
      const double ro2 = (1.5 * r) * (1.5 * r);
      if (blocked && d2 <= ro2 && (rx * hx + ry * hy) >= 0.0 && in_half_fan(half, r, rx, ry, d2, ro2)) c |= 4;
      cls[idx] = c;
      if (c & 4) {
        occ_flag[idx] = 1;
        atomicAdd(&blk[idx >> 8], 1);
      }
    }
  }
}

// the form of fo_rays_kernel the step took (launch_rays); far: the half-planes the grid kernel wrote, or null
void launch_settle(const StaticMap *m, const Scene *sc, const fo_step_t &p, int nw, const double *far, hipStream_t s) {
  const dim3 grid(SETTLE_BLOCKS + p.O), block(64 * nw);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, m->E, m->d_edges, m->d_chunk_box, p.d_edge_skip, p.O, p.d_ocorn, p.d_oflags, m->x0, m->y0,
                       m->cs, p.win_ix0, p.win_iy0, p.win_nx, p.ego_x, p.ego_y, p.head_x, p.head_y, p.r, p.d_half, sc->d_amb, sc->d_namb,
                       p.d_cls, sc->d_flags, sc->d_blk, p.win_ny, far);
  };
  if (p.d_edge_skip) { if (nw == 1) go(fo_settle_kernel<true, 1>); else go(fo_settle_kernel<true, RAY_WAVES>); }
  else { if (nw == 1) go(fo_settle_kernel<false, 1>); else go(fo_settle_kernel<false, RAY_WAVES>); }
}

}  // namespace
