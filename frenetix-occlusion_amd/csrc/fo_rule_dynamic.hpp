// fo_rule_dynamic.hpp -- Car / Bicycle behind a visible dynamic obstacle (spawn_locator.py:145-317, rectangle fit :695-726): the
// whole workgroup, sixteen workgroups per obstacle up to the hand-off of the candidate lattice.  Six phases, member functions of
// RlDyn in the order they run; rl_dynamic_rule at the end of the file is the sequence.
// LDS: the kernel lends the rule its arrays; who owns which in which phase (a barrier lies between any two owners):
//   lab   [97 x 97] int   phase 1 BORROWS words [0, 2 048) as the hit list of its lanelet queries; from phase 3: the lattice (a
//                         member node's own index, INT_MAX elsewhere; phase 4 stamps the largest part with its label)
//   ired  [97 x 97] int   phases 1-2: flags per lanelet [P]; phase 4: the run tables [3][RL_MAXRUN] | the part sizes per label;
//                         from phase 5: the polygon slot that held each node (member_idx's hint)
//   red   [3 072] double  [0, 64): per-wave partial sums (phases 5, 6); [0, 2 048): phase 4's node form, a pair per thread.  The
//                         tail from red + 64, as int: edge_band's list `el` (phases 3, 6), in between phase 5's hit list
//   fitok [2 048] bytes   [0, 1 536): phase 6, a fit's clipped points; [1 536, 2 048): phases 2-5, `relflag` (P <= 512)
//   polyv [2 RL_PVERT] double   from phase 2: the candidate polygons' vertices (while they fit: `plds`)
#pragma once
#include "fo_rule_frame.hpp"

namespace {

constexpr int RL_MAXRUN = 3072;   // row runs of the lattice the runs form of phase 4 holds (three tables in `ired`: 9 409 ints)
constexpr int RL_FITROWS = 25;    // lattice rows of the wider fit (the Car's 2.5 m at 0.1 m)

// the rule's own scalars and small tables in LDS, declared once (rl_dynamic_rule); the digit: the phase that writes it.  8-byte
// members first and an even count of ints per line group: no padding
struct RlDynShared {
  unsigned long long rowbits[RL_LAT][2], bestA;   // 4: member nodes of a lattice row; 6: smallest enclosing rectangle (bits of a double)
  double obsd[2], oc[8], pbox[32];         // 1: the obstacle's (s, d), its corners; 2: bounding boxes of the candidate polygons
  double c[2], yaw, fit[4];                // 5: centroid of the largest part, lane heading there; 6: area, cx, cy, jaccard of a fit
  int pol[8], npol, go;                    // 1: candidate polygons (lanelets); go on? (also phase 5's verdict)
  int ego_ll, inter, inter_first;          // 1: the ego's lanelet, the intersection it is in
  int nin, in[16], vll[RL_FIFTHV];         // 1: lanelets that hold the obstacle's centre; lanelet under every fifth window vertex
  int curv_ok, nhit;                       // 1: the obstacle projects onto the path; rl_which_lanelets' count (zero between queries)
  int pb0[8], plen[8], poff[9], plds;      // 2: first vertex and length in the map; offsets in polyv; they all fit polyv
  int ecnt, ticket;                        // 3: edge_band's count (zero between bands); the hand-off ticket
  int rowoff[RL_LAT + 1], nrun;            // 4: runs in front of each row; runs in all
  int changed, best, bestn;                // 4: a round changed a label | the root run; the largest part's label and size
  int relc, front, yawok;                  // 5: centroid on a relevant lanelet, region in front of the obstacle, a heading
  int fitany, nv, np2;                     // 6: a fit clipped something in; its part is a proper polygon; hull candidates
  int a0[RL_FITROWS], a1[RL_FITROWS], hull_r[64], hull_c[64];   // 6: first / last clipped point per row; the candidates (row, column)
};

// the per-obstacle values the phases share (registers), the kernel's LDS arrays, and the phases
struct RlDyn {
  static constexpr double h = 0.25, fh = 0.1;   // steps of the candidate lattice and of the fits' lattice
  static constexpr int NL = RL_LAT * RL_LAT;
  const RuleView &v;
  const RuleParams &pr;
  RlDynShared &sh;
  int *lab, *ired;
  double *red;
  unsigned char *fitok;
  double *polyv;
  int *g_lab;                                   // the obstacle's lattice in HBM: node | polygon slot << 16, or INT_MAX
  double cx, cy, olen, owid;                    // the obstacle's centre and size
  int *el;                                      // edge_band's list
  bool el_on = false;                           // member_idx asks the listed edges instead of walking the polygons
  double oc_c = 0.0, oc_s = 0.0, fc = 0.0, fs = 0.0;   // cos, sin of the obstacle's heading | of the lane heading at the centroid
  bool wedge = false;                           // the obstacle comes towards the ego: the region is its own shadow
  int npol = 0, best = -1;                      // candidate polygons; label of the largest part
  bool plds = false, rel_fits = false;          // the polygons' vertices are in polyv; relflag holds the relevance flags
  unsigned char *relflag = nullptr;

  // ---------------------------------------------------------------- phase 1: relevant lanelets, go / no-go
  // Writes ired[0, P), sh.oc ... vll; borrows lab[0, 2 048).  False (uniform): out of table space, or the ego is on no lanelet.
  // relevant lanelets (:171-202): the other incomings / inner lanelets of the intersection the ego is in, else the
  // oncoming neighbours (adj_left) of the lanelets under every fifth vertex of the reference window.  Flags per lanelet
  // in ired[0, P): bit0 relevant, bit1 inner, bit2 holds the obstacle's centre.  Every "which lanelet holds this point" below is asked of all lanelets at
  // once, a thread per (point, lanelet) -- the first lanelet in list order by atomicMin -- instead of one thread walking
  // the polygon table in HBM
  __device__ __forceinline__ bool lanelet_flags(const double *oc, double *rec, int part) {
    const int tid = threadIdx.x, nth = blockDim.x;
    // out of table space (-1 in the Car slot's validity word; every part of the obstacle decides the same and leaves before the
    // hand-off): more lanelets than the flag array holds (refused by the host entry already), or more fifth vertices of the window
    if (v.P > RL_LAT * RL_LAT || (pr.win_i1 - pr.win_i0 + 4) / 5 > RL_FIFTHV) {
      if (part == 0 && tid == 0) { rec[2] = -1.0; rec[5] = 0.0; }
      return false;
    }
    for (int p = tid; p < v.P; p += nth) ired[p] = 0;
    if (tid == 0) {
      rec[2] = 0.0; rec[5] = 0.0;
      sh.go = 0; sh.npol = 0; sh.inter = -1; sh.inter_first = 0x7fffffff; sh.ego_ll = 0x7fffffff; sh.nin = 0; sh.relc = 0; sh.curv_ok = 0; sh.nhit = 0;
    }
    if (tid == 0) sh.ecnt = 0;   // (edge_band's count, far below)
    if (tid >= 64 && tid < 72) sh.oc[tid - 64] = oc[tid - 64];   // (the obstacle's corners for the shadow test: LDS instead of a load from HBM's caches per edge and point)
    if (tid < RL_FIFTHV) sh.vll[tid] = 0x7fffffff;
    __syncthreads();
    // (measured and dropped, round 6: the lanelets under every fifth vertex of the reference window -- needed when the ego turns
    // out to be in no intersection, two barriers further down -- asked in this same pass: +4 us in front of the lattice where
    // there IS an intersection, the usual case of the rule)
    // the lanelets under the ego (the first in list order) and under the obstacle's centre (all of them; also flagged: more than
    // sixteen are re-collected in list order below); the hit list borrows the lattice array, which is idle until the hand-off
    rl_which_lanelets(v, 2, [&](int q, double &x, double &y) { x = q == 0 ? pr.ego_x : cx; y = q == 0 ? pr.ego_y : cy; },
                      [](int, int) { return true; },
                      [&](int q, int p) {
                        if (q == 0) { atomicMin(&sh.ego_ll, p); return; }
                        atomicOr(&ired[p], 4);
                        const int k = atomicAdd(&sh.nin, 1);
                        if (k < 16) sh.in[k] = p;
                      }, lab, 2048, &sh.nhit);
    if (tid < 64) {   // the obstacle's curvilinear position (wave 0)
      double ob_s, ob_d;
      const bool okc = rl_to_curv_wave(v, cx, cy, ob_s, ob_d);
      if (tid == 0) { sh.curv_ok = okc ? 1 : 0; sh.obsd[0] = ob_s; sh.obsd[1] = ob_d; sh.nhit = 0; }
    }
    __syncthreads();
    if (sh.ego_ll == 0x7fffffff) return false;
    // the first intersection (list order) that lists the ego's lanelet: a thread per table entry and an atomicMin on the
    // intersection's index (one thread walking the table was a chain of dependent loads)
    {
      const int n_ent = v.n_inter > 0 ? v.inter_off[v.n_inter] : 0;
      for (int e = tid; e < n_ent; e += nth)
        if (v.inter_lanelet[e] == sh.ego_ll) {
          int it = 0;
          while (it + 1 < v.n_inter && v.inter_off[it + 1] <= e) ++it;
          atomicMin(&sh.inter_first, it);
        }
    }
    __syncthreads();
    if (tid == 0) sh.inter = sh.inter_first == 0x7fffffff ? -1 : sh.inter_first;
    __syncthreads();
    if (sh.inter >= 0) {
      for (int e = v.inter_off[sh.inter] + tid; e < v.inter_off[sh.inter + 1]; e += nth) {
        const int p = v.inter_lanelet[e];
        atomicOr(&ired[p], (p != sh.ego_ll ? 1 : 0) | (v.inter_kind[e] == 1 ? 2 : 0));
      }
    } else if (v.adj_left) {
      const int nv = (pr.win_i1 - pr.win_i0 + 4) / 5;   // every fifth vertex of the reference window (40 m: a dozen; <= RL_FIFTHV, above)
      rl_which_lanelets(v, nv, [&](int q, double &x, double &y) { const double *w_ = v.path + 6 * (size_t)(pr.win_i0 + 5 * q); x = w_[0]; y = w_[1]; },
                        [](int, int) { return true; }, [&](int q, int p) { atomicMin(&sh.vll[q], p); }, lab, 2048, &sh.nhit);
      if (tid < nv) {
        const int ll = sh.vll[tid];
        if (ll != 0x7fffffff && v.adj_left[ll] >= 0) atomicOr(&ired[v.adj_left[ll]], 1);
      }
    }
    __syncthreads();
    return true;
  }
  // thread 0 decides.  Reads ired[0, P) and phase 1's scalars; writes sh.pol / npol / go and, short of table space, rec[2]
  __device__ __forceinline__ bool decide(double *rec) {
    const int tid = threadIdx.x, nth = blockDim.x;
    if (tid == 0) {
      sh.nhit = 0;   // (the next lanelet query -- the centroid's -- finds its list empty)
      do {
        if (sqrt((pr.ego_x - cx) * (pr.ego_x - cx) + (pr.ego_y - cy) * (pr.ego_y - cy)) > RL_MAX_DIST_OBST) break;   // :215
        // the obstacle's lanelets (all that hold its centre) in list order.  Up to sixteen arrived through the atomic counter
        // in any order and are sorted; MORE than sixteen (a centre on a pile of overlapping lanelets) would leave a subset that
        // depends on the arrival order -- and the sixteen workgroups of an obstacle must take identical decisions before their
        // hand-off ticket below -- so the first sixteen in list order are collected from the flags instead
        // (and more than sixteen is more than the rule holds: the step's list is refused, below)
        int n_ob = min(sh.nin, 16);
        bool short_of_space = sh.nin > 16;
        if (sh.nin > 16) {
          n_ob = 0;
          for (int p = 0; p < v.P && n_ob < 16; ++p)
            if (ired[p] & 4) sh.in[n_ob++] = p;
        }
        for (int i = 1; i < n_ob; ++i) {   // (a point lies on a handful of lanelets: insertion sort)
          const int key = sh.in[i];
          int j = i - 1;
          while (j >= 0 && sh.in[j] > key) { sh.in[j + 1] = sh.in[j]; --j; }
          sh.in[j + 1] = key;
        }
        int first_rel = -1;
        bool any_rel = false, all_inner = true;
        for (int i = 0; i < n_ob; ++i) {
          const int p = sh.in[i];
          if (ired[p] & 1) {
            any_rel = true;
            if (first_rel < 0) first_rel = p;
            if (sh.npol < 7) sh.pol[sh.npol++] = p; else short_of_space = true;
          }
          if (!(ired[p] & 2)) all_inner = false;
        }
        // more relevant lanelets under the obstacle's centre than candidate polygons are held (seven + the predecessor): out of
        // table space, -1 in the Car slot's validity word (the selection kernel refuses the step's list).  Every part of the
        // obstacle decides the same and writes the same -- whichever clears the word last at its own start writes it again here.
        if (short_of_space) { rec[2] = -1.0; break; }
        if (!any_rel) break;                                                        // :222
        if (!sh.curv_ok) break;
        if (sh.obsd[0] < pr.ego_s + 3.0 || fabs(sh.obsd[1]) > 15.0) break;            // :234
        if (sh.inter >= 0 && n_ob > 0 && all_inner && v.pred0 && v.pred0[first_rel] >= 0 && sh.npol < 8) sh.pol[sh.npol++] = v.pred0[first_rel];   // :249-252
        sh.go = 1;
      } while (false);
    }
    __syncthreads();
    return sh.go != 0;
  }

  // ---------------------------------------------------------------- phase 2: the candidate polygons staged
  // Reads sh.pol, ired[0, P); writes sh.pb0 ... plds, polyv and relflag = fitok[1 536, 2 048).
  // where the candidate polygons' vertices go in LDS (member_idx below); too many vertices: read from HBM as before.  (Round 6:
  // a thread per polygon asks for its offsets, then ONE flat copy of all vertices -- thread 0 used to walk the offset table,
  // sixteen loads one after the other, and the copy ran polygon by polygon behind a load of its own each)
  __device__ __forceinline__ void stage_polygons(double oy) {
    const int tid = threadIdx.x, nth = blockDim.x;
    npol = sh.npol;
    if (tid < npol) {
      const int p = sh.pol[tid], b0 = v.poly_off[p];
      sh.pb0[tid] = b0;
      sh.plen[tid] = v.poly_off[p + 1] - b0;
    }
    if (tid < 4 * npol) sh.pbox[tid] = v.poly_box[4 * (size_t)sh.pol[tid >> 2] + (tid & 3)];
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int i = 0; i < npol; ++i) { sh.poff[i] = tot; tot += sh.plen[i]; }
      sh.poff[npol] = tot;
      sh.plds = tot <= RL_PVERT;
    }
    __syncthreads();
    plds = sh.plds != 0;
    if (plds) {
      const int n2 = 2 * sh.poff[npol];
      for (int k = tid; k < n2; k += nth) {
        int i = 0;
        while (i + 1 < npol && k >= 2 * sh.poff[i + 1]) ++i;
        polyv[k] = v.poly_xy[2 * (size_t)sh.pb0[i] + (k - 2 * sh.poff[i])];
      }
    }
    // (the relevance flags move to the end of `lab`'s companion array later; keep a compact copy for the centroid test)
    relflag = fitok + 1536;   // [P] bit0: relevant -- only consulted for the few lanelets holding the centroid
    rel_fits = v.P <= 512;
    if (rel_fits)
      for (int p = tid; p < v.P; p += nth) relflag[p] = (unsigned char)(ired[p] & 1);
    __syncthreads();
    // membership of a point in the candidate region's defining sets (:254-277)
    const double diff = fmod(fabs(oy - pr.ego_yaw), 6.283185307179586);
    wedge = 3.141592653589793 - RL_TOL_SAME_DIR <= diff && diff <= 3.141592653589793 + RL_TOL_SAME_DIR;
    oc_c = cos(oy);
    oc_s = sin(oy);
  }
  // Reads sh.oc, pbox, poff, pol, polyv and, with el_on, el[0, sh.ecnt).
  // (the tests are a conjunction: cheapest first -- distance, the obstacle grown by 1 m, shadow / occluded class -- and
  // the lanelet polygons, the dear ones, last)
  // returns 0 (not a member) or 1 + the slot of a candidate polygon that holds the point; `hint`: the slot asked first
  __device__ __forceinline__ int member_idx(double x, double y, int hint) const {
    const double rx = x - cx, ry = y - cy;
    // sqrt(d2) <= 12 exactly when d2 <= 144: the midpoint between 12 and the next double squares to 144 + 2.1e-14, below the
    // double that follows 144 (144 + 2.8e-14) -- no square root needed
    static_assert(RL_BUFFER_SIDE == 12.0, "the squared form of the distance test is derived for 12 m");
    if (!(rx * rx + ry * ry <= 144.0)) return 0;
    const double lx_ = oc_c * rx + oc_s * ry, ly_ = -oc_s * rx + oc_c * ry;
    const double ex_ = fmax(fabs(lx_) - olen / 2.0, 0.0), ey_ = fmax(fabs(ly_) - owid / 2.0, 0.0);
    // minus the obstacle grown by 1 m: sqrt(e2) > 1 exactly when e2 > 1 + 2^-52 (sqrt(1 + 2^-52) = 1 + 2^-53 - ... rounds to 1)
    if (!(ex_ * ex_ + ey_ * ey_ > 1.0000000000000002)) return 0;
    if (wedge) {   // the obstacle's own shadow: the sight line ego -> point crosses the rectangle (:264)
      bool hit = false;
      const double dx = x - pr.ego_x, dy = y - pr.ego_y;
      for (int i = 0; i < 4 && !hit; ++i) {
        const int j = (i + 1) & 3;
        const double ex = sh.oc[2 * j] - sh.oc[2 * i], ey = sh.oc[2 * j + 1] - sh.oc[2 * i + 1];
        const double den = dx * ey - dy * ex, wx = sh.oc[2 * i] - pr.ego_x, wy = sh.oc[2 * i + 1] - pr.ego_y;
        if (fabs(den) > 1e-14) {
          // t = tn / den and u = un / den in [0, 1] without the divisions: a correctly rounded quotient is <= 1 exactly
          // when |tn| <= |den| and >= 0 exactly when the signs agree (or tn = 0)
          const double tn = wx * ey - wy * ex, un = wx * dy - wy * dx;
          hit = den > 0.0 ? (tn >= 0.0 && tn <= den && un >= 0.0 && un <= den) : (tn <= 0.0 && tn >= den && un <= 0.0 && un >= den);
        }
      }
      if (!hit) return 0;
    } else if (!(rl_class_at(v, x, y) & 4)) {   // the global occluded area (:272)
      return 0;
    }
    // possible_polygon (:255): the union of the candidate lanelet polygons -- any order of asking gives the same answer;
    // the polygon that held the nearest lattice node goes first (it holds most points around that node as well)
    if (el_on) {
      // ONE pass over the edges listed for the band the point lies in (edge_band below: only those can straddle its y), all
      // polygons at once: a crossing flips the bit of the edge's polygon -- the crossing number is a parity, the order of the
      // edges does not matter, each edge is tested by the arithmetic of the ring walk -- and a polygon with an odd count
      // holds the point if its bounding box does (rl_in_polygon asks the box first; kept, so that the answer is the ring
      // walk's in every rounding case).  The walk polygon by polygon was a chain of four dependent LDS round trips per
      // polygon, and a wave walks every polygon one of its lanes needs: 1.3 of the 2.2 us a wave spent per point.
      const double2 *pv2 = (const double2 *)polyv;
      const int n = sh.ecnt;
      int par = 0;
      for (int h0 = 0; h0 < n; h0 += 4) {
        int en[4];
        double2 pi[4], pj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) en[u] = el[h0 + u < n ? h0 + u : n - 1];
#pragma unroll
        for (int u = 0; u < 4; ++u) { pi[u] = pv2[en[u] & 1023]; pj[u] = pv2[(en[u] >> 10) & 1023]; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (h0 + u < n && (pi[u].y > y) != (pj[u].y > y) && rl_left_of_crossing(x, y, pi[u].x, pi[u].y, pj[u].x, pj[u].y)) par ^= 1 << (en[u] >> 20);
      }
      for (int i = 0; par != 0 && i < npol; ++i)
        if ((par >> i) & 1) {
          const double *bb = sh.pbox + 4 * i;
          if (!(x < bb[0] || x > bb[2] || y < bb[1] || y > bb[3])) return i + 1;
        }
      return 0;
    }
    for (int q = 0; q < npol; ++q) {
      const int i = q == 0 ? hint : (q <= hint ? q - 1 : q);
      if (!plds) {
        if (rl_in_polygon(v, sh.pol[i], x, y)) return i + 1;
        continue;
      }
      const double *bb = sh.pbox + 4 * i;            // rl_in_polygon on the copy in LDS (the same arithmetic)
      if (x < bb[0] || x > bb[2] || y < bb[1] || y > bb[3]) continue;
      const double2 *pv2 = (const double2 *)polyv;
      if (rl_crossing_parity(sh.poff[i], sh.poff[i + 1], x, y, [&](int k) { return pv2[k]; }) != 0) return i + 1;
    }
    return 0;
  }
  // edge_band(ylo, yhi): the edges of the candidate polygons that some y in [ylo, yhi] can straddle (min(yi, yj) <= yhi and
  // max(yi, yj) > ylo: a straddled edge has min <= y < max) -- round 6.  A lanelet polygon has 50-100 vertices; a band of lattice
  // rows or a fit's rectangle is crossed by a handful of its edges.  An entry: the edge's vertex | its predecessor in the ring
  // << 10 | the polygon's slot << 20 (RL_PVERT = 1024 vertices in LDS).  The list borrows the tail of `red` (the lanelet
  // queries' hit list, idle here) and holds every edge if it must.  The count is zero on entry (cleared behind a barrier
  // after its last reader); ends with a barrier.
  static_assert(RL_PVERT <= 1024, "edge_band packs two vertex indices of ten bits");
  __device__ __forceinline__ void edge_band(double ylo, double yhi) const {
    const int tid = threadIdx.x, nth = blockDim.x;
    const double2 *pv2 = (const double2 *)polyv;
    const int tot = sh.poff[npol];
    for (int k = tid; k < tot; k += nth) {
      int i = 0;
      while (i + 1 < npol && k >= sh.poff[i + 1]) ++i;
      const int kj = k == sh.poff[i] ? sh.poff[i + 1] - 1 : k - 1;
      const double yi = pv2[k].y, yj = pv2[kj].y;
      if (fmin(yi, yj) <= yhi && fmax(yi, yj) > ylo) el[atomicAdd(&sh.ecnt, 1)] = k | (kj << 10) | (i << 20);
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------- phase 3: membership lattice over the sixteen parts, hand-off
  // Writes this part's slice of g_lab, borrows `el`; true for the workgroup with the last ticket, which fills `lab` and goes on.
  // RL_PARTS workgroups (on as many CUs) share the lattice: each decides its slice of the nodes -- membership is arithmetic,
  // ~300 float64 operations per node, and one CU's four SIMDs are the limit -- and writes it to the obstacle's lattice in
  // HBM; the workgroup that finishes LAST (a counter per obstacle) loads the whole lattice and goes on alone, the others
  // are done.  (Every workgroup took the same decisions up to here: they read the same inputs.)
  __device__ __forceinline__ bool lattice(int part, int *g_cnt) {
    const int tid = threadIdx.x, nth = blockDim.x;
    const int chunk = (NL + RL_PARTS - 1) / RL_PARTS, i1 = min((part + 1) * chunk, NL);
    if (plds && part * chunk < i1) {   // the rows of this workgroup's slice (the nodes' y by the expression of the loop below: monotone in the row)
      edge_band(cy + (-RL_BUFFER_SIDE + (double)((part * chunk) / RL_LAT) * h), cy + (-RL_BUFFER_SIDE + (double)((i1 - 1) / RL_LAT) * h));
      el_on = true;
    }
    for (int i = part * chunk + tid; i < i1; i += nth) {
      const int ix = i % RL_LAT, iy = i / RL_LAT;
      const int mi = member_idx(cx + (-RL_BUFFER_SIDE + (double)ix * h), cy + (-RL_BUFFER_SIDE + (double)iy * h), 0);
      g_lab[i] = mi ? (i | ((mi - 1) << 16)) : 0x7fffffff;      // (+ which polygon held the node: the fits' hint)
    }
    el_on = false;
    // Hand-off with ONE release and ONE acquire per workgroup (round 6).  The fences are whole-cache operations -- the release
    // writes the XCD's L2 back, the acquire invalidates the CU's L1 and the L2's non-local lines -- and sixteen waves issuing
    // them one after the other cost 5 us on the releasing and 3 us on the acquiring side (stamps of the trace build;
    // tools/microbench/grid_barrier.hip: the same finding for a grid barrier).  The workgroup barrier in front orders every
    // wave's stores before thread 0's release (its cumulativity carries them to agent scope), the one behind holds the
    // other waves' loads back until thread 0's acquire has been executed for the CU they share.
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      sh.ticket = atomicAdd(g_cnt, 1);
    }
    __syncthreads();
    if (sh.ticket != RL_PARTS - 1) return false;
    if (tid == 0) {
      *g_cnt = 0;   // for the next planning step (launches on a stream are ordered)
      __threadfence();
    }
    if (tid == 64) sh.ecnt = 0;   // (edge_band's count: every reader is past the barriers above)
    __syncthreads();
    const volatile int *gl = g_lab;
    for (int i = tid; i < NL; i += nth) { const int w = gl[i]; lab[i] = w == 0x7fffffff ? w : (w & 0xffff); }
    __syncthreads();
    return true;
  }

  // ---------------------------------------------------------------- phase 4: the largest connected part (runs form | node form)
  // Both forms read `lab`, own `ired` and leave sh.best / bestn, the part's nodes in `lab` stamped with sh.best.
  // connected parts (4-neighbourhood, scipy.ndimage.label's default), their sizes and the largest one (first maximum in label
  // order, :279-281).  Round 6: on the RUNS of the lattice rows (maximal stretches of member nodes in a row: a few per row, a
  // couple of hundred in all) instead of on its 9 409 nodes -- the sixteen waves cut the rows into runs with two ballots per
  // row, ONE wave then labels the runs by the same label equivalence as before (a run's label = its index, runs are numbered
  // row-major, so the smallest index of a part is the run that holds the part's smallest linear node index = scipy's numbering
  // order; runs of neighbouring rows touch where their column intervals overlap), adds up the run lengths per root and picks
  // the largest part; the nodes of that part are then stamped with its label.  A wave's LDS traffic is ordered: its rounds need
  // no workgroup barrier, where the node form paid three barriers of sixteen waves per round and two more passes over the
  // lattice for the sizes (7.8 + 8.5 us -> see DESIGN section 5).  More runs than the arrays hold: the node form below.
  // row_runs: the rows cut into runs -> sh.rowbits, rowoff, nrun.  True: the run tables hold them
  __device__ __forceinline__ bool row_runs() const {
    const int tid = threadIdx.x, nth = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63, nw = nth >> 6;
    for (int r = wave; r < RL_LAT; r += nw) {
      const unsigned long long b0 = __ballot(lab[r * RL_LAT + lane] != 0x7fffffff);
      const unsigned long long b1 = __ballot(lane < RL_LAT - 64 && lab[r * RL_LAT + 64 + (lane < RL_LAT - 64 ? lane : 0)] != 0x7fffffff);
      if (lane == 0) {
        const unsigned long long s0 = b0 & ~(b0 << 1), s1 = b1 & ~((b1 << 1) | (b0 >> 63));
        sh.rowbits[r][0] = b0; sh.rowbits[r][1] = b1;
        sh.rowoff[r + 1] = __popcll(s0) + __popcll(s1);
      }
    }
    if (tid == 0) sh.rowoff[0] = 0;
    __syncthreads();
    if (tid < 64) {   // inclusive prefix of the row counts (97 rows: two per lane)
      const int r0 = 2 * tid + 1, r1 = 2 * tid + 2;
      const int c0 = r0 <= RL_LAT ? sh.rowoff[r0] : 0, c1 = r1 <= RL_LAT ? sh.rowoff[r1] : 0;
      int incl = c0 + c1;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if (tid >= off) incl += t; }
      if (r0 <= RL_LAT) sh.rowoff[r0] = incl - c1;
      if (r1 <= RL_LAT) sh.rowoff[r1] = incl;
      if (tid == 63) sh.nrun = incl;
    }
    __syncthreads();
    return sh.nrun <= RL_MAXRUN;   // (uniform)
  }
  __device__ __forceinline__ void label_runs_wave0() const {
    const int tid = threadIdx.x, lane = tid & 63, NR = sh.nrun;
    int *const run_rec = ired, *const run_lab = ired + RL_MAXRUN, *const run_size = ired + 2 * RL_MAXRUN;
    for (int round = 0; round < 4096; ++round) {
      bool ch = false;
      for (int i = lane; i < NR; i += 64) {
        const int rec_ = run_rec[i], r = rec_ >> 16, c0 = (rec_ >> 8) & 255, c1 = rec_ & 255;
        const int l = run_lab[i];
        int m = l;
        if (r > 0)
          for (int j = sh.rowoff[r - 1]; j < sh.rowoff[r]; ++j) {
            const int q = run_rec[j];
            if (((q >> 8) & 255) <= c1 && (q & 255) >= c0) m = min(m, run_lab[j]);
          }
        if (r + 1 < RL_LAT)
          for (int j = sh.rowoff[r + 1]; j < sh.rowoff[r + 2]; ++j) {
            const int q = run_rec[j];
            if (((q >> 8) & 255) <= c1 && (q & 255) >= c0) m = min(m, run_lab[j]);
          }
        if (m < l) { atomicMin(&run_lab[l], m); ch = true; }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (int i = lane; i < NR; i += 64) {
        int r0 = run_lab[i];
        while (true) {
          const int q = run_lab[r0];
          if (q == r0) break;
          r0 = q;
        }
        run_lab[i] = r0;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (!__ballot(ch)) break;
    }
    for (int i = lane; i < NR; i += 64) {
      const int rec_ = run_rec[i];
      atomicAdd(&run_size[run_lab[i]], (rec_ & 255) - ((rec_ >> 8) & 255) + 1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // the largest part, the smallest label among equals: (size, -index) as one 64-bit key
    unsigned long long key = 0ull;
    for (int i = lane; i < NR; i += 64)
      if (run_lab[i] == i) {
        const unsigned long long k_ = ((unsigned long long)(unsigned)run_size[i] << 32) | (unsigned)(0x7fffffff - i);
        key = k_ > key ? k_ : key;
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o_ = __shfl_xor(key, off);
      key = o_ > key ? o_ : key;
    }
    if (tid == 0) {
      if (key >> 32) {
        const int bi = 0x7fffffff - (int)(unsigned)(key & 0xffffffffull), rec_ = run_rec[bi];
        sh.bestn = (int)(key >> 32);
        sh.best = (rec_ >> 16) * RL_LAT + ((rec_ >> 8) & 255);   // the part's smallest linear node index = its label
        sh.changed = bi;                                          // (the root run, for the stamping below)
      } else { sh.bestn = 0; sh.best = -1; sh.changed = -1; }
    }
  }
  __device__ __forceinline__ void label_by_runs() const {
    const int tid = threadIdx.x, nth = blockDim.x, NR = sh.nrun;
    int *const run_rec = ired, *const run_lab = ired + RL_MAXRUN, *const run_size = ired + 2 * RL_MAXRUN;
    {
      const int wave = tid >> 6, lane = tid & 63, nw = nth >> 6;
      for (int r = wave; r < RL_LAT; r += nw) {   // the runs of row r: a lane per start column
        const unsigned long long b0 = sh.rowbits[r][0], b1 = sh.rowbits[r][1];
        const unsigned long long s0 = b0 & ~(b0 << 1), s1 = b1 & ~((b1 << 1) | (b0 >> 63));
        const int base = sh.rowoff[r];
        if ((s0 >> lane) & 1ull) {
          const unsigned long long z = ~(b0 >> lane);          // first column past the run, relative to `lane`
          int len = z ? __builtin_ctzll(z) : 64;
          if (lane + len == 64) len += b1 == ~0ull ? 64 : __builtin_ctzll(~b1);   // (the run goes on in the second word)
          const int idx = base + __popcll(s0 & ((1ull << lane) - 1ull));
          run_rec[idx] = (r << 16) | (lane << 8) | (lane + len - 1);
          run_lab[idx] = idx;
          run_size[idx] = 0;
        }
        if ((s1 >> lane) & 1ull) {
          const int len = __builtin_ctzll(~(b1 >> lane));
          const int idx = base + __popcll(s0) + __popcll(s1 & ((1ull << lane) - 1ull));
          run_rec[idx] = (r << 16) | ((64 + lane) << 8) | (64 + lane + len - 1);
          run_lab[idx] = idx;
          run_size[idx] = 0;
        }
      }
    }
    __syncthreads();
    if (tid < 64) label_runs_wave0();   // wave 0 alone: label equivalence on the runs, sizes, the largest part
    __syncthreads();
    {   // stamp the nodes of the largest part (every other member node keeps its own index, which is not the part's label)
      const int root = sh.changed, bl = sh.best;
      for (int i = tid; i < NR; i += nth)
        if (run_lab[i] == root) {
          const int rec_ = run_rec[i], r = rec_ >> 16;
          for (int c = (rec_ >> 8) & 255; c <= (rec_ & 255); ++c) lab[r * RL_LAT + c] = bl;
        }
    }
    __syncthreads();
  }
  // the node form (FO_SCENE_RULE_NODES=1, or more runs than the tables hold); borrows red[0, 2 048) for its partial maxima
  // connected parts (4-neighbourhood, scipy.ndimage.label's default) by label equivalence (Hawick et al.): every member node
  // starts as its own root (label = linear index); a round links the root of every node whose neighbourhood holds a smaller
  // label to that label (atomicMin), then flattens every node to its root by pointer jumping; labels only ever decrease
  // and stay inside their part, so every part ends up carrying its smallest linear index (= scipy's numbering order) after
  // a handful of rounds, whatever its shape -- and every thread of the workgroup works in every round
  __device__ __forceinline__ void label_by_nodes() const {
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int round = 0; round < 256; ++round) {
      if (tid == 0) sh.changed = 0;
      __syncthreads();
      bool ch = false;
      for (int i = tid; i < NL; i += nth) {
        const int l = lab[i];
        if (l == 0x7fffffff) continue;
        const int ix = i % RL_LAT, iy = i / RL_LAT;
        int m = l;
        if (ix > 0) m = min(m, lab[i - 1]);
        if (ix + 1 < RL_LAT) m = min(m, lab[i + 1]);
        if (iy > 0) m = min(m, lab[i - RL_LAT]);
        if (iy + 1 < RL_LAT) m = min(m, lab[i + RL_LAT]);
        if (m < l) { atomicMin(&lab[l], m); ch = true; }
      }
      if (ch) sh.changed = 1;
      __syncthreads();
      for (int i = tid; i < NL; i += nth) {
        int r = lab[i];
        if (r == 0x7fffffff) continue;
        while (true) {
          const int q = lab[r];
          if (q == r) break;
          r = q;
        }
        lab[i] = r;
      }
      __syncthreads();
      if (!sh.changed) break;
      __syncthreads();
    }
    // the largest part (first maximum in label order, :279-281): sizes by the roots' labels.  A thread counts a contiguous
    // stretch of nodes and adds a run of equal labels with one atomic (neighbours in a row mostly share their part)
    if (tid == 0) { sh.best = -1; sh.bestn = 0; }
    for (int i = tid; i < NL; i += nth) ired[i] = 0;
    __syncthreads();
    {
      const int per = (NL + nth - 1) / nth, i0 = tid * per, i1 = min(i0 + per, NL);
      int run_l = 0x7fffffff, run_n = 0;
      for (int i = i0; i < i1; ++i) {
        const int l = lab[i];
        if (l == run_l) { ++run_n; continue; }
        if (run_n > 0 && run_l != 0x7fffffff) atomicAdd(&ired[run_l], run_n);
        run_l = l; run_n = 1;
      }
      if (run_n > 0 && run_l != 0x7fffffff) atomicAdd(&ired[run_l], run_n);
    }
    __syncthreads();
    {   // first maximum in label order: per-thread (count, smallest label), then thread 0 over the partials
      int bn = 0, bi = -1;
      for (int i = tid; i < NL; i += nth)
        if (ired[i] > bn || (ired[i] == bn && bn > 0 && i < bi)) { bn = ired[i]; bi = i; }
      red[2 * tid] = (double)bn; red[2 * tid + 1] = (double)bi;
      __syncthreads();
      // (two levels: 32 threads fold nth / 32 partials each, thread 0 folds those -- the order is fixed, the rule associative)
      const int grp = nth / 32;
      if (tid < 32) {
        int gn = 0, gl = -1;
        for (int i = tid * grp; i < (tid + 1) * grp; ++i) {
          const int n_ = (int)red[2 * i], l_ = (int)red[2 * i + 1];
          if (n_ > gn || (n_ == gn && n_ > 0 && l_ < gl)) { gn = n_; gl = l_; }
        }
        red[2 * tid * grp] = (double)gn; red[2 * tid * grp + 1] = (double)gl;
      }
      __syncthreads();
      if (tid == 0)
        for (int t = 0; t < 32; ++t) {
          const int n_ = (int)red[2 * t * grp], l_ = (int)red[2 * t * grp + 1];
          if (n_ > sh.bestn || (n_ == sh.bestn && n_ > 0 && l_ < sh.best)) { sh.bestn = n_; sh.best = l_; }
        }
      __syncthreads();
    }
  }

  // ---------------------------------------------------------------- phase 5: the centroid and the three checks
  // Reads lab, g_lab; writes sh.c; takes `ired` over for the hints; red[0, 32): the waves' partial sums
  __device__ __forceinline__ void centroid() const {
    const int tid = threadIdx.x, nth = blockDim.x;
    // (the polygon slot that held each lattice node -- the hint of member_idx, for the fits -- is asked for here, under the
    // centroid's arithmetic, and parked in `ired`, which is free from here on)
    int hint_w[(RL_LAT * RL_LAT + RL_THREADS - 1) / RL_THREADS];
    {
      const volatile int *gl = g_lab;
#pragma unroll
      for (int u = 0; u < (RL_LAT * RL_LAT + RL_THREADS - 1) / RL_THREADS; ++u) {
        const int i = tid + u * RL_THREADS;
        hint_w[u] = i < NL ? gl[i] : 0x7fffffff;
      }
    }
    // centroid of the part (mean of its nodes; fixed summation order: per-thread partials, then thread 0)
    double ax = 0.0, ay = 0.0;
    for (int i = tid; i < NL; i += nth)
      if (lab[i] == best) { ax += cx + (-RL_BUFFER_SIDE + (double)(i % RL_LAT) * h); ay += cy + (-RL_BUFFER_SIDE + (double)(i / RL_LAT) * h); }
    // fixed summation order: per thread, a butterfly over the wave (every lane ends with the same total), the waves in order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { ax += __shfl_xor(ax, off); ay += __shfl_xor(ay, off); }
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = ax; red[2 * (tid >> 6) + 1] = ay; }
#pragma unroll
    for (int u = 0; u < (RL_LAT * RL_LAT + RL_THREADS - 1) / RL_THREADS; ++u) {
      const int i = tid + u * RL_THREADS;
      if (i < NL) ired[i] = hint_w[u] == 0x7fffffff ? 0 : (hint_w[u] >> 16);
    }
    __syncthreads();
    if (tid == 0) {
      double sx_ = 0.0, sy_ = 0.0;
      for (int w = 0; w < nth / 64; ++w) { sx_ += red[2 * w]; sy_ += red[2 * w + 1]; }
      sh.c[0] = sx_ / (double)sh.bestn; sh.c[1] = sy_ / (double)sh.bestn;
    }
    __syncthreads();
  }
  __device__ __forceinline__ bool in_region(double x, double y) const {   // (reads lab and the hints in ired)
    const int ix = (int)rint((x - (cx - RL_BUFFER_SIDE)) / h), iy = (int)rint((y - (cy - RL_BUFFER_SIDE)) / h);
    if (ix < 0 || ix >= RL_LAT || iy < 0 || iy >= RL_LAT) return false;
    const int l_ = lab[iy * RL_LAT + ix], hn_ = ired[iy * RL_LAT + ix];
    return l_ == best && member_idx(x, y, hn_) != 0;
  }
  // Reads sh.c, relflag; writes sh.front, yawok, yaw, relc and the verdict sh.go; borrows the tail of `red` as its hit list.
  // three conditions, independent of each other (:287-300): the centroid on a relevant lanelet -- every lanelet asked at once
  // --, no region in front of the obstacle, a lane heading at the centroid.  Round 6: the last two are taken by the LAST thread
  // of the workgroup (another wave) while the others ask the lanelets, instead of by thread 0 behind them (a membership test
  // and a raster look-up by one thread: ~3 us of the chain)
  __device__ __forceinline__ bool checks() const {
    const int tid = threadIdx.x, nth = blockDim.x;
    if (tid == nth - 1) {
      sh.front = in_region(cx + 4.0 * oc_c, cy + 4.0 * oc_s) ? 1 : 0;                  // the region in front of the obstacle (:297)
      double yw = 0.0;
      sh.yawok = rl_lane_yaw_at(v, sh.c[0], sh.c[1], yw) ? 1 : 0;
      sh.yaw = yw;
    }
    if (rel_fits) {   // the centroid must lie on a relevant lanelet (:287-291): every relevant lanelet asked at once
      // (sh.nhit: zero since the set-up's last query -- the hand-off and four barriers lie between; the list borrows the tail of `red`)
      rl_which_lanelets(v, 1, [&](int, double &x, double &y) { x = sh.c[0]; y = sh.c[1]; }, [&](int, int p) { return (relflag[p] & 1) != 0; },
                        [&](int, int) { sh.relc = 1; }, (int *)(red + 64), 2048, &sh.nhit);
    } else {
      __syncthreads();
    }
    if (tid == 0) {
      sh.go = 0;
      do {
        // the centroid must lie on a relevant lanelet (:287-291)
        bool rel_c = rel_fits && sh.relc;
        for (int p = 0; !rel_fits && p < v.P && !rel_c; ++p)
          if (rl_in_polygon(v, p, sh.c[0], sh.c[1])) {
            if (sh.inter >= 0) {
              if (p != sh.ego_ll)
                for (int e = v.inter_off[sh.inter]; e < v.inter_off[sh.inter + 1]; ++e)
                  if (v.inter_lanelet[e] == p) rel_c = true;
            } else {
              for (int i = pr.win_i0; i < pr.win_i1 && !rel_c; i += 5) {
                const double *q = v.path + 6 * (size_t)i;
                const int ll = rl_lanelet_of(v, q[0], q[1]);
                if (ll >= 0 && v.adj_left && v.adj_left[ll] == p) rel_c = true;
              }
            }
          }
        if (!rel_c) break;
        if (sh.front) break;
        if (!sh.yawok) break;
        sh.go = 1;
      } while (false);
    }
    __syncthreads();
    return sh.go != 0;
  }

  // ---------------------------------------------------------------- phase 6: the two rectangle fits
  // rectangle fits on a 0.1 m lattice (:695-726): lane-aligned rectangle clipped to the region -> area, centroid, Jaccard
  // similarity with the minimum rotated rectangle of the clipped part.  NX = rint(length / fh), NY = rint(width / fh) as
  // constants: the index split is a multiplication instead of two divisions per point.
  // clip: writes fitok[0, NX NY), sh.a0 / a1, fit, fitany; red[0, 48): the waves' partial sums; borrows `el`.  False: nothing
  // clipped in, or nothing clipped off (Jaccard 1)
  template <int NX, int NY>
  __device__ __forceinline__ bool clip(double ccx, double ccy, double length, double width) {
    constexpr int nx_ = NX, ny_ = NY, np_ = NX * NY;
    static_assert(NY <= RL_FITROWS && NX * NY <= 1536, "sh.a0 / a1 hold a row each, fitok[0, 1 536) a point each");
    const int tid = threadIdx.x, nth = blockDim.x;
    int cnt = 0;
    double fx = 0.0, fy = 0.0;
    if (plds) {   // the rectangle's extent in y (+ a micrometre for the roundings of the points' expression below)
      const double ext = fabs(fs) * (length / 2.0) + fabs(fc) * (width / 2.0) + 1e-6;
      edge_band(ccy - ext, ccy + ext);
      el_on = true;
    }
    for (int i = tid; i < np_; i += nth) {
      const double u = ((double)(i % nx_) + 0.5) * fh - length / 2.0, w_ = ((double)(i / nx_) + 0.5) * fh - width / 2.0;
      const double x = ccx + fc * u - fs * w_, y = ccy + fs * u + fc * w_;
      const bool ok = in_region(x, y);
      fitok[i] = ok ? 1 : 0;
      if (ok) { ++cnt; fx += x; fy += y; }
    }
    el_on = false;
    double fn = (double)cnt;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { fx += __shfl_xor(fx, off); fy += __shfl_xor(fy, off); fn += __shfl_xor(fn, off); }
    if ((tid & 63) == 0) { red[3 * (tid >> 6)] = fx; red[3 * (tid >> 6) + 1] = fy; red[3 * (tid >> 6) + 2] = fn; }
    __syncthreads();
    if (tid == 128) sh.ecnt = 0;   // (edge_band's count, read by the clipping above; barriers follow)
    // the clipped part's convex hull needs only the first and last clipped point of every lattice row (the rest of a row
    // lies between them): a thread per row finds them while thread 0 adds up the partial sums
    if (tid >= 64 && tid < 64 + ny_) {
      const int r = tid - 64;
      int a0 = -1, a1 = -1;
      for (int c = 0; c < nx_; ++c)
        if (fitok[r * nx_ + c]) { if (a0 < 0) a0 = c; a1 = c; }
      sh.a0[r] = a0; sh.a1[r] = a1;
    }
    if (tid == 0) {
      double sx_ = 0.0, sy_ = 0.0, n = 0.0;
      for (int w = 0; w < nth / 64; ++w) { sx_ += red[3 * w]; sy_ += red[3 * w + 1]; n += red[3 * w + 2]; }
      sh.fitany = n > 0.0;
      sh.fit[0] = n * fh * fh; sh.fit[1] = n > 0.0 ? sx_ / n : 0.0; sh.fit[2] = n > 0.0 ? sy_ / n : 0.0;
      sh.fit[3] = ((int)n == np_) ? 1.0 : 0.0;
    }
    __syncthreads();
    return !(!sh.fitany || sh.fit[3] == 1.0);
  }
  // reads sh.a0 / a1; writes sh.hull_r / hull_c, np2, nv, bestA and the Jaccard similarity sh.fit[3]
  template <int NX, int NY>
  __device__ __forceinline__ void fit(double ccx, double ccy, double length, double width) {
    constexpr int ny_ = NY;
    const int tid = threadIdx.x, nth = blockDim.x;
    if (!clip<NX, NY>(ccx, ccy, length, width)) return;
    // The smallest rectangle over the edge directions of the clipped part's convex hull (:716-724), without building the
    // hull: the enclosing rectangle of smallest area has a side along a hull edge (Freeman & Shapira), so the minimum over
    // the directions of ALL point pairs is the minimum over the hull's edge directions -- a superset of directions cannot
    // undercut the global optimum, and it contains the hull's.  <= 64 points (first and last clipped point of every lattice
    // row, integer lattice coordinates), <= 2 016 pairs over the workgroup, each spanning the extents of all points; the
    // smallest area is kept by atomicMin on its bit pattern (positive doubles order like their bits).  Fewer than three
    // points, or all on one line (QHull raises there): Jaccard 0.
    if (tid < 64) {
      // the candidate list (wave 0: a lane per lattice row): first and last clipped point of the row, but only where the left
      // (first points) or right (last points) chain turns strictly outwards against its neighbours in the rows below and
      // above -- every vertex of the convex hull does; points on straight stretches (most: the part is a clipped
      // rectangle) and in dents do not, they neither span an extent nor define a hull edge
      const int r = tid;
      const int a0 = r < ny_ ? sh.a0[r] : -1, a1 = r < ny_ ? sh.a1[r] : -1;
      int rp = -1, rn = -1;
      if (a0 >= 0) {
        for (int q = r - 1; q >= 0 && rp < 0; --q) if (sh.a0[q] >= 0) rp = q;
        for (int q = r + 1; q < ny_ && rn < 0; ++q) if (sh.a0[q] >= 0) rn = q;
      }
      bool k0 = a0 >= 0, k1 = a0 >= 0 && a1 != a0;
      if (a0 >= 0 && rp >= 0 && rn >= 0) {
        const int zl = (r - rp) * (sh.a0[rn] - a0) - (a0 - sh.a0[rp]) * (rn - r);   // > 0: the left chain bulges to smaller columns here
        const int zr = (r - rp) * (sh.a1[rn] - a1) - (a1 - sh.a1[rp]) * (rn - r);   // < 0: the right chain bulges to larger columns
        if (a1 != a0) { k0 = zl > 0; k1 = zr < 0; }
        else k0 = zl > 0 || zr < 0;
      }
      const int cnt = (k0 ? 1 : 0) + (k1 ? 1 : 0);
      int incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if (tid >= off) incl += t; }
      int pos = incl - cnt;
      if (k0) { sh.hull_r[pos] = r; sh.hull_c[pos] = a0; ++pos; }
      if (k1) { sh.hull_r[pos] = r; sh.hull_c[pos] = a1; }
      if (tid == 63) sh.np2 = incl;
      // a proper polygon?  fewer than three clipped points, or all of them on one line (QHull raises there): Jaccard 0
      const int n_all = __popcll(__ballot(a0 >= 0)) + __popcll(__ballot(a0 >= 0 && a1 != a0));
      const int rf = __ffsll((long long)__ballot(a0 >= 0)) - 1;      // first row that holds a point
      bool off = false;
      if (rf >= 0 && a0 >= 0) {
        const int c0 = sh.a0[rf];
        const int rl = 63 - __clzll((long long)__ballot(a0 >= 0));    // last such row; the line through (rf, c0) and (rl, its last point)
        const int dc = sh.a1[rl] - c0, dr = rl - rf;
        off = (dr * (a0 - c0) - dc * (r - rf) != 0) || (dr * (a1 - c0) - dc * (r - rf) != 0);
      }
      const bool proper = n_all >= 3 && __ballot(off) != 0;
      if (tid == 0) { sh.nv = proper ? 3 : 0; sh.bestA = 0x7ff0000000000000ull; }   // +inf
    }
    __syncthreads();
    const int np2 = sh.np2;
    for (int w = tid; w < np2 * np2; w += nth) {
      const int i = w / np2, j = w % np2;
      if (i >= j) continue;
      double ex = (double)(sh.hull_c[j] - sh.hull_c[i]), ey = (double)(sh.hull_r[j] - sh.hull_r[i]);
      const double nn = sqrt(ex * ex + ey * ey);
      ex /= nn; ey /= nn;
      double a1n = INFINITY, a1x = -INFINITY, a2n = INFINITY, a2x = -INFINITY;
      for (int q = 0; q < np2; ++q) {
        const double p1 = (double)sh.hull_c[q] * ex + (double)sh.hull_r[q] * ey, p2 = (double)sh.hull_c[q] * (-ey) + (double)sh.hull_r[q] * ex;
        a1n = fmin(a1n, p1); a1x = fmax(a1x, p1); a2n = fmin(a2n, p2); a2x = fmax(a2x, p2);
      }
      const double area = ((a1x - a1n) * fh + fh) * ((a2x - a2n) * fh + fh);
      atomicMin(&sh.bestA, (unsigned long long)__double_as_longlong(area));
    }
    __syncthreads();
    if (sh.nv < 3) return;   // degenerate (QHull raises): Jaccard 0
    if (tid == 0) sh.fit[3] = fmin(1.0, sh.fit[0] / __longlong_as_double((long long)sh.bestA));
    __syncthreads();
  }
  // the Car fit around the part's centroid, the Bicycle fit around the Car fit's; rec[2 .. 7]: the two spawn points
  __device__ __forceinline__ void fits(double *rec) {
    fc = cos(sh.yaw);
    fs = sin(sh.yaw);
    fit<55, 25>(sh.c[0], sh.c[1], 5.5, 2.5);
    if (!sh.fitany) return;
    const double car_a = sh.fit[0], car_x = sh.fit[1], car_y = sh.fit[2], car_j = sh.fit[3];
    __syncthreads();
    fit<20, 10>(car_x, car_y, 2.0, 1.0);
    if (threadIdx.x == 0) {
      if (car_a >= RL_AREA_CAR && car_j > 0.98) { rec[2] = 1.0; rec[3] = car_x; rec[4] = car_y; }
      if (sh.fitany && sh.fit[0] >= RL_AREA_BIKE && sh.fit[3] > 0.98) { rec[5] = 1.0; rec[6] = sh.fit[1]; rec[7] = sh.fit[2]; }
    }
  }
};

// rec: [0] distance, [1] role = 2, [2] car valid, [3] car x, [4] car y, [5] bicycle valid, [6] x, [7] y
// lab, red, ired, fitok, polyv: the kernel's LDS arrays; g_lab, g_cnt: the obstacle's lattice and ticket counter in HBM
__device__ __forceinline__ void rl_dynamic_rule(const RuleView &v, const RuleParams &pr, int o, const double *ocorn, const double *ocen,
                                const double *oyaw, const double *odims, double *rec, int *lab, double *red, int *ired,
                                unsigned char *fitok, double *polyv, int part, int *g_lab, int *g_cnt) {
  __shared__ RlDynShared sh;
  const double oy = oyaw[o];
  RlDyn d{v, pr, sh, lab, ired, red, fitok, polyv, g_lab, ocen[2 * o], ocen[2 * o + 1], odims[2 * o], odims[2 * o + 1], (int *)(red + 64)};
  if (!d.lanelet_flags(ocorn + 8 * (size_t)o, rec, part)) return;
  if (!d.decide(rec)) return;
  d.stage_polygons(oy);
  if (!d.lattice(part, g_cnt)) return;
  if (!pr.label_nodes && d.row_runs()) d.label_by_runs(); else d.label_by_nodes();
  d.best = sh.best;
  if (d.best < 0 || (double)sh.bestn * RlDyn::h * RlDyn::h < RL_MIN_AREA) return;                  // :282-284
  d.centroid();
  if (!d.checks()) return;
  d.fits(rec);
}

}  // namespace
