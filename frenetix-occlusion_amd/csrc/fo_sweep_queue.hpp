// fo_sweep_queue.hpp -- the queue kernel: the product's sweep (fo_sweep_queue_body, one function, and the kernel around it).
// A part of the fo_sweep.hip translation unit, included after fo_sweep_generic.hpp (whose helpers it uses); not a header
// to include on its own.
#pragma once

namespace {

// ================================================================================================ queue kernel
// Same arithmetic as the generic kernel, restructured around what the first profiles showed (profiles/r01_*):
// the kernel is fp64-VALU bound and 40 % of its instructions were the 36 erf evaluations of the CP box sums,
// executed by whole waves although only ~7 % of the (trajectory, agent, t) samples are inside the 5 m gate.
//   pass 1 (t loop)  DCE + gate test; in-gate (lane, t) samples are appended to a per-wave LDS queue with
//                    ballot/mbcnt; whenever 64 samples are queued the wave evaluates them with all lanes busy
//                    (each lane fetches "its" sample's ego/agent rows by index) and scatters cp into cpbuf[t][lane];
//   pass 2 (t loop)  harm + risk + running maxima + coalesced list stores, cp read back from cpbuf.
// exp() for the logistic models is a 64-entry 2^(j/64) table + degree-5 polynomial (~15 VALU ops).
// Supports T-1 <= TQ; longer horizons take the generic kernel.
enum { HM_LR4S = 0, HM_DVMAX = 1, HM_GENERIC = 2 };   // per-agent bodies by harm model (see agent_body in the kernel)
// What an agent's body is told about its harm model: hm_const<HM> -- a compile-time constant, one copy of the body per model
// -- or hm_any, the model as a run-time value in a single copy (the horizon-split form).
template <int HM> using hm_const = std::integral_constant<int, HM>;
struct hm_any { int value; };
template <class Tag> struct hm_fixed : std::true_type {};
template <> struct hm_fixed<hm_any> : std::false_type {};
constexpr int DVR = TC + 1;          // rows of the per-wave ring of relative speeds: samples t0-1 .. t1-1 are live at once
constexpr int WROWS = TC + DVR;      // LDS rows (64 doubles each) per wave
constexpr int QCAP = 128;
static_assert(TC <= 16, "two class bits per sample are kept in 32-bit lanes, 16 samples deep");

// v_max_f64 / v_min_f64 without the canonicalisation fmax()/fmin() add for loop-carried operands (IEEE quieting of
// signalling NaNs: two extra instructions per call); operands here are results of arithmetic, never signalling
__device__ __forceinline__ double fo_vmax(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double fo_vmin(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double fo_vmin_neg(double a, double b) {   // min(a, -b), the sign as a source modifier
  double r;
  asm("v_min_f64 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// exp(z) = 2^(k/256) * e^r, k = rint(256 z / ln 2), |r| <= ln2/512: 256-entry table of 2^(j/256) in LDS (2 KB) and a
// degree-3 polynomial (remainder r^4/24 < 1.5e-13 relative).  One-step argument reduction: ln2/256 cut to 43
// significant bits, so k * hi is exact for |k| < 2^10 and the dropped tail costs |k| * 2.1e-16 (< 1e-12 relative over
// the arguments the logistic models produce, z in [-5e3, 6]; a logistic value moves by a quarter of that).  Few distinct
// float64 constants on purpose: every one of them occupies an SGPR pair for the whole loop.
template <bool CLAMP = true, int DEG = 3>
__device__ __forceinline__ double fo_exp_tab(const double *__restrict__ tab2, double z) {
  if (CLAMP) z = fmin(fmax(z, -700.0), 700.0);  // CLAMP = false: the caller bounds the argument
  const double MAGIC = 6755399441055744.0;                          // 1.5 * 2^52
  const double tm = fma(z, 369.3299304675746, MAGIC);               // 256 / ln 2
  const double kf = tm - MAGIC;
  const int k = __double2loint(tm);
  const double r = fma(kf, -0x1.62e42fefa3800p-9, z);               // ln2/256, 43 significant bits
  const double tv = tab2[k & (EXP_N - 1)];
  double p;
  if (DEG >= 3) {
    p = fma(r, 1.0 / 6.0, 0.5);
    p = fma(p, r, 1.0);
  } else {
    p = fma(r, 0.5, 1.0);   // degree 2: remainder r^3/6 < 4.2e-10 relative (a logistic value moves by a quarter of that)
  }
  p = fma(p, r, 1.0);
  return ldexp(tv, k >> 8) * p;   // the scaling beside the polynomial, not behind it (exact either way)
}
// 1 + exp(z), the denominator of the logistic models: the table entry is scaled while the polynomial is evaluated, and
// the product and the 1 are one fma -- mul, ldexp, add in a row became ldexp and fma (one instruction less per logistic).
template <bool CLAMP = true, int DEG = 3>
__device__ __forceinline__ double fo_exp1p_tab(const double *__restrict__ tab2, double z) {
  if (CLAMP) z = fmin(fmax(z, -700.0), 700.0);
  const double MAGIC = 6755399441055744.0;
  const double tm = fma(z, 369.3299304675746, MAGIC);
  const double kf = tm - MAGIC;
  const int k = __double2loint(tm);
  const double r = fma(kf, -0x1.62e42fefa3800p-9, z);
  const double tv = ldexp(tab2[k & (EXP_N - 1)], k >> 8);
  double p;
  if (DEG >= 3) {
    p = fma(r, 1.0 / 6.0, 0.5);
    p = fma(p, r, 1.0);
  } else {
    p = fma(r, 0.5, 1.0);
  }
  p = fma(p, r, 1.0);
  return fma(tv, p, 1.0);
}

// 1 / (1 + exp(nz)); v_rcp_f64 (measured ~3e-8 relative) + one Newton step (1.6e-14 against the oracle)
template <bool CLAMP = true, int DEG = 3>
__device__ __forceinline__ double fo_logistic_neg(const double *__restrict__ tab2, double nz) {
  const double d = fo_exp1p_tab<CLAMP, DEG>(tab2, nz);
  const double y = __builtin_amdgcn_rcp(d);
  return fma(fma(-d, y, 1.0), y, y);
}

// (Round 5, measured and dropped: both logistic values of a sample through ONE reciprocal -- y = 1/(d1 d2), s1 = y d2,
// s2 = y d1: a quarter-rate v_rcp_f64 and a Newton step less for three multiplications -- 0.5398 against 0.5410 ms: the chain
// add -> mul -> rcp -> fma -> fma -> mul is two operations longer than add -> rcp -> fma -> fma, and the chain is what counts.)

// Box probabilities under a CORRELATED covariance (collision_probability.py:117 hands any 2x2 matrix to mvnun).  With
// L(h, k) = P(X > h, Y > k) for the standardised pair, Drezner & Wesolowsky / Genz write
//   L(h, k; rho) = Phi(-h) Phi(-k) + 1/(2 pi) Int_0^asin(rho) exp(-(h^2 + k^2 - 2 h k sin th) / (2 cos^2 th)) dth,
// and P(box) = L(a1,a2) - L(b1,a2) - L(a1,b2) + L(b1,b2): the Phi products add up to the diagonal box probability the
// kernel computes anyway, the integrals to a correction that vanishes with rho.  The integrand is smooth in th whatever
// the box and the variances are: Gauss-Legendre with 6 / 8 / 12 / 20 / 24 nodes for |rho| <= 0.5 / 0.7 / 0.9 / 0.97 /
// 0.99 is exact to 1e-11 (tools/corr_nodes.py), a tenth of what the erf table leaves.  Arguments here are in units of 1/(sigma sqrt 2), which cancels the 2 of the
// denominator.  sin over |th| <= asin(0.99) = 1.43: Taylor through th^21 (remainder 1e-18).
__device__ __forceinline__ double fo_sin_halfpi(double x) {
  const double z = x * x;
  double p = -1.0 / 51090942171709440000.0;            // 1/21!
  p = fma(p, z, 1.0 / 121645100408832000.0);           // 19!
  p = fma(p, z, -1.0 / 355687428096000.0);             // 17!
  p = fma(p, z, 1.0 / 1307674368000.0);                // 15!
  p = fma(p, z, -1.0 / 6227020800.0);                  // 13!
  p = fma(p, z, 1.0 / 39916800.0);                     // 11!
  p = fma(p, z, -1.0 / 362880.0);                      // 9!
  p = fma(p, z, 1.0 / 5040.0);                         // 7!
  p = fma(p, z, -1.0 / 120.0);                         // 5!
  p = fma(p, z, 1.0 / 6.0);                            // 3!  (sign below)
  return fma(-x * z, p, x);
}
// the four corner terms of one box at one node: s2 = 2 sin th, c2 = 1/cos^2 th  (four table exponentials in flight:
// serialising them to save registers was measured 40 % slower)
__device__ __forceinline__ double fo_corr_corners(const double *__restrict__ exp_tab, double A, double B, double Cc, double D,
                                                  double s2, double c2) {
  const double a2 = A * A, b2 = B * B;
  const double eAC = fo_exp_tab(exp_tab, -c2 * fma(-s2 * A, Cc, fma(Cc, Cc, a2)));
  const double eBC = fo_exp_tab(exp_tab, -c2 * fma(-s2 * B, Cc, fma(Cc, Cc, b2)));
  const double eAD = fo_exp_tab(exp_tab, -c2 * fma(-s2 * A, D, fma(D, D, a2)));
  const double eBD = fo_exp_tab(exp_tab, -c2 * fma(-s2 * B, D, fma(D, D, b2)));
  return (eAC - eBC) - (eAD - eBD);
}

// Whole millimetres of the distance sqrt(d2): rint(RN(d * 1000)) = 1000 np.round(d, 3) (dce.py:79, half to even).  fo_sqrt alone
// (~1e-14 relative) rounded distances at an exact half millimetre the other way -- two dyadic rectangles 19/16 m apart, 1187.5
// mm, came out as 1187 (tests/test_sweep_exact_gpu.py).  So the root gets one more correction from its exact residual,
// y += (d2 - y^2) / (2 y) with the residual from one fma: the error drops to ~1e-28 relative before the last rounding, so an
// exact root (every tie) comes out exact and every other root is rounded correctly unless it lies that close to a midpoint.  Two fma per exact distance.  (A branch to sqrt() next to a half millimetre instead cost
// the queue kernels 2 % on the headline: the kernel sits at its register cap.)
__device__ __forceinline__ double fo_mm(double d2) {
  const double g = __builtin_amdgcn_rsq(d2);
  double y = d2 * g;
  const double h = 0.5 * g;
  y = fma(y, fma(-h, y, 0.5), y);     // fo_sqrt's Goldschmidt step
  y = fma(fma(-y, y, d2), h, y);      // the correction
  double z;
  asm("v_max_f64 %0, %1, 0" : "=v"(z) : "v"(y));   // d2 = 0: NaN -> 0 (as in fo_sqrt)
  return __builtin_rint(z * 1000.0);
}

// Rounded distance (whole millimetres, rint(1000 d) = 1000 np.round(d, 3), dce.py:79) between the ego rectangle at
// rear-axle pose (ex, ey, heading (ec, es)) and the agent rectangle at (px, py, heading (pc, ps)): four-axis SAT
// (overlap -> 0), otherwise the minimum over the eight corner-to-box distances.
__device__ __forceinline__ double fo_rect_mm(double ex, double ey, double ec, double es, double px, double py, double pc,
                                             double ps, double hlA, double hwA, double wb, double hlB, double hwB) {
  const double cr = pc * ec + ps * es, sr = ps * ec - pc * es;
  const double ccx = ex + wb * ec, ccy = ey + wb * es;  // convert_dynamic_obstacle.py:73
  const double dx = px - ccx, dy = py - ccy;
  const double ax = ec * dx + es * dy, ay = ec * dy - es * dx;
  const double ux = hlB * cr, uy = hlB * sr, wx = -hwB * sr, wy = hwB * cr;
  const double bx = -(pc * dx + ps * dy), by = -(pc * dy - ps * dx);
  const double vx = hlA * cr, vy = -hlA * sr, zx = hwA * sr, zy = hwA * cr;
  const double s1 = fabs(ax) - (hlA + fabs(ux) + fabs(wx)), s2 = fabs(ay) - (hwA + fabs(uy) + fabs(wy));
  const double s3 = fabs(bx) - (hlB + fabs(vx) + fabs(zx)), s4 = fabs(by) - (hwB + fabs(vy) + fabs(zy));
  if (!(fmax(fmax(s1, s2), fmax(s3, s4)) > 0.0)) return 0.0;
  double d2 = fo_pt_box2(ax + ux + wx, ay + uy + wy, hlA, hwA);
  d2 = fmin(d2, fo_pt_box2(ax + ux - wx, ay + uy - wy, hlA, hwA));
  d2 = fmin(d2, fo_pt_box2(ax - ux + wx, ay - uy + wy, hlA, hwA));
  d2 = fmin(d2, fo_pt_box2(ax - ux - wx, ay - uy - wy, hlA, hwA));
  d2 = fmin(d2, fo_pt_box2(bx + vx + zx, by + vy + zy, hlB, hwB));
  d2 = fmin(d2, fo_pt_box2(bx + vx - zx, by + vy - zy, hlB, hwB));
  d2 = fmin(d2, fo_pt_box2(bx - vx + zx, by - vy + zy, hlB, hwB));
  d2 = fmin(d2, fo_pt_box2(bx - vx - zx, by - vy - zy, hlB, hwB));
  return fo_mm(d2);
}

// wave-uniform tables are read through the constant address space: the loads become s_load (scalar cache, results in
// SGPRs) instead of 64-lane broadcasts through the vector memory path.  The tables are written by an earlier launch
// (fo_prep_agents_kernel), so the scalar cache is coherent with them.
typedef const double __attribute__((address_space(4))) *cdp_t;
typedef const int32_t __attribute__((address_space(4))) *cip_t;
__device__ __forceinline__ cdp_t fo_const(const double *p) { return (cdp_t)(unsigned long long)p; }
__device__ __forceinline__ cip_t fo_const(const int32_t *p) { return (cip_t)(unsigned long long)p; }

// tuning builds (-DFO_TRACE=1): four more wall-clock stamps per workgroup, by wave 0, in rows [32768 + blockIdx] of the trace
// buffer (tools/split_trace.py): 0 the agent's constants and first rows resident, 1 pass 1 of the (last) chunk done, 2 pass 2
// done, 3 the agent's horizon segments folded
#if FO_TRACE
#define SW_STAMP(i) do { if (a.trace && threadIdx.x == 0) a.trace[4 * (size_t)(32768 + blockIdx.x) + (i)] = wall_clock64(); } while (0)
#else
#define SW_STAMP(i) do { } while (0)
#endif
// ALLM: the default metric set (dce, cp, ttc, ttce, hr all active, no debug ablation) is compiled with the flags as
// constants -- fewer wave-uniform masks to keep in SGPRs, fewer branches; any other selection takes the generic copy.
// SPLIT (small batches, where one agent per wave leaves most SIMDs with a single wave): the four waves of a workgroup
// take the SAME agent and a quarter of the horizon each (time chunk `wave`); every per-pair result is a minimum or a
// first maximum over time, so the segments are folded in time order through LDS at the end.  Needs T <= QWAVES * TC.
// CORR: the agent set holds a covariance with correlation (status[1] of fo_prep_agents_kernel): in-gate samples then
// add the correlation integral to their box probabilities (fo_corr_corners).  The kernel below carries both bodies and picks one at
// its start, so that the usual diagonal case keeps the registers and the code it had.
// Harm model: everything the body does per agent -- the DCE probe, both passes of every chunk, the pair outputs, the running
// extrema -- is one generic lambda (agent_body) that takes the agent's harm model as a tag.  On the full grid it is
// instantiated three times (hm_const<HM_LR4S | HM_DVMAX | HM_GENERIC>) and ONE wave-uniform three-way branch per agent picks
// the copy: at three waves per SIMD every instruction and every taken branch of the sample loops is paid in full, and the
// per-sample `is this agent LR4S` (three places in pass 1), the per-chunk choice of pass 2's body, the headings, the impact
// classes and their re-rating are gone from the copies that do not need them (pass-1 loop of the headline instantiation: 485
// -> 392 instructions, 136 -> 106 scalar, in the two non-LR4S copies).  The horizon-split form keeps ONE
// copy with the model as a run-time value (hm_any): its workgroups live for one chunk per wave, where the flags cost nothing
// that shows, and three copies there put 35-40 spilled VGPRs (96-112 B of scratch per lane) into the instantiations that
// tests/test_kernel_shape_cpu.py holds to 48 B.
// (Measured and dropped with it: a second copy of pass 1's sample loop without the two range tests, for chunks that lie wholly
// inside the agent's prediction -- four instructions and two branches less per sample, but twice the pass-1 copies: 105
// spilled VGPRs instead of 35 and scalar spills inside the loop, 0.533 / 0.542 ms against 0.497 / 0.500)
template <bool PAIR, int LISTS, bool ALLM, bool SPLIT, bool CORR>
__device__ __forceinline__ void fo_sweep_queue_body(const SweepArgs a, const double2 *__restrict__ erf_tab,
                                                    const double *__restrict__ exp_tab, const double *__restrict__ zc_tab,
                                                    double *__restrict__ hk_all, double *__restrict__ cpbuf_all,
                                                    unsigned short *__restrict__ queue_all, int *__restrict__ pool_i,
                                                    double *__restrict__ pool_hd) {
  constexpr int QCAPX = SPLIT ? TILE * TC : QCAP;           // queue entries per wave: a chunk's worth with the pool (pool_round)
  static_assert(!SPLIT || WROWS >= 10, "the horizon-split fold parks ten values per lane in the wave's rows");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int tile = (j % a.nt8) * 8 + r;
  const int chunk = j / a.nt8;
  if (tile >= a.n_tiles) return;
  // Lanes past the last trajectory hold copies of trajectory M-1 (fo_prep_traj_kernel pads the tile that way) and
  // run as its duplicates: they compute the same values and store them to the same addresses.  No output store is
  // predicated, on purpose: a skipped store path makes the compiler's s_waitcnt for the prefetched loads assume
  // that no store lies between issue and use, which drains the store queue in every iteration of pass 2.
  const int m = min(tile * TILE + lane, a.M - 1);
  const int T = a.T, Tm1 = a.T - 1, M = a.M, A = a.A;
  const double *tjb = a.traj + (size_t)tile * T * NEF * TILE;  // uniform tile base
  const double *tj = tjb + 2 * lane;
  double *cpw = cpbuf_all + wave * (WROWS * TILE);
  double *dvw = cpw + TC * TILE;
  double *hk = hk_all + wave * 4;
  unsigned short *q = queue_all + wave * QCAPX;
  const bool do_dce = ALLM || (a.mask & FO_M_DCE), do_cp = ALLM || (a.mask & FO_M_CP), do_hr = ALLM || (a.mask & FO_M_HR);
  const bool do_ttc = ALLM || (a.mask & FO_M_TTC), do_ttce = ALLM || (a.mask & FO_M_TTCE);
  const uint32_t ablate = ALLM ? 0u : a.ablate;
  const double hlA = a.hlA, hwA = a.hwA;

  double w_min_dce = INFINITY;
  // ttc / ttce are round3(time_dce * dt), monotone in time_dce: the minima over agents are kept as integer steps
  int w_min_tttc = 0x7fffffff, w_min_tttce = 0x7fffffff;
  double w_max_er = 0.0, w_max_or = 0.0, w_max_eh = 0.0, w_max_oh = 0.0, w_max_cp = 0.0, w_max_hwc = 0.0;
  int w_arg_dce = -1, w_arg_ttc = -1, w_arg_or = -1;  // agent indices as integers: three VGPRs less than as doubles
  bool w_dce_flag = false;


  // Evaluates queued in-gate samples, one per lane (collision_probability.py:77-122).  `item` = lane | row << 6 of a queue
  // entry of agent kq (half inflated length hdq) in the chunk whose buffer row 0 holds gate sample gbq; the probability goes
  // to row `row` of the cp rows at cpq.  With the workgroup-wide pool (below) the lanes of one call hold entries of up to
  // four agents -- whichever wave evaluates them.
  auto gate_items = [&](bool valid, int item, int kq, double hdq, int gbq, double *cpq) {
    if (valid) {
      const int src = item & 63, row = item >> 6, ti = gbq + row;
      const double *e = tjb + (size_t)(ti + 1) * NEF * TILE + 2 * src;  // ego sample ti+1 of trajectory `src`
      const fo_d2 qxy = fo_ld2(e), qcs = fo_ld2(e + EF(2));
      const double qex = qxy.x, qey = qxy.y, qec = qcs.x, qes = qcs.y;
      const double *g0 = a.atab + ((size_t)kq * a.Ta + ti) * NAF;      // agent mean / covariance: sample ti
      const double qpx = g0[0], qpy = g0[1], qisx = g0[6] * ERF_SCALE, qisy = g0[7] * ERF_SCALE;
      const double qc1 = g0[NAF + 2], qs1 = g0[NAF + 3];             // agent heading: sample ti+1 (Q1); ti+1 < L
      const double devx = qc1 * hdq, devy = qs1 * hdq;
      const double rx = qex - qpx, ry = qey - qpy;
      const double bxs = a.len3 * qec, bys = a.len3 * qes;           // rear-axle based boxes (Q2)
      double acc = 0.0;
      // The 36 erf arguments are affine in (mean j, box b, side): in units of the table spacing,
      //   X(j, b, +-) = (rx - j devx + b bxs +- off_x) 128 / (sigma_x sqrt 2)
      // -- scaled once per sample, then two running sums and one add per argument instead of an add and a multiplication
      // (four operations less per box; the arguments move by ~1e-13 of a table step)
      const double DX = devx * qisx, DY = devy * qisy, BX = bxs * qisx, BY = bys * qisy;
      const double ox = a.off_x * qisx, oy = a.off_y * qisy;
      double qx = fma(rx, qisx, DX), qy = fma(ry, qisy, DY);   // j = -1
#pragma unroll 1
      for (int jm = 0; jm < 3; ++jm) {
        double cx = qx - BX, cy = qy - BY;                      // b = -1
        // the three boxes of a mean side by side (twelve table reads in flight; with the three-term erf step the registers
        // are there in every form: 0.514 -> 0.508 ms on the headline; all nine boxes in a row: 0.520)
#pragma unroll 3
        for (int b = 0; b < 3; ++b) {
          const double fx = fo_erf_fast128(erf_tab, cx + ox) - fo_erf_fast128(erf_tab, cx - ox);
          const double fy = fo_erf_fast128(erf_tab, cy + oy) - fo_erf_fast128(erf_tab, cy - oy);
          acc = fma(fx, fy, acc);
          cx += BX; cy += BY;
        }
        qx -= DX; qy -= DY;
      }
      // (1/2)(1/2) of the two Phi differences, /3 (:122).  A row poisoned by fo_prep_agents_kernel (no usable
      // covariance: 1/sigma = NaN) must read NaN: the table erf clamps its argument, which would turn the NaN into
      // erf(+-6) and the probability into 0
      cpq[row * TILE + src] = (qisx != qisx || qisy != qisy) ? NAN : acc * (0.25 / 3.0);
    }
    if (CORR) {
      // Covariances with correlation: a second walk over the same queued samples adds the correlation integral of
      // the nine boxes to the value stored above.  It re-reads its operands (nothing of the evaluation above stays
      // live: this body shares the kernel's register budget with the usual one); whole batches without a
      // correlated sample skip it, and asin(rho) = 0 makes it vanish lane by lane.
      __asm__ volatile("" ::: "memory");
      const double asr = valid ? a.atab[((size_t)kq * a.Ta + gbq + (item >> 6)) * NAF + 11] : 0.0;
      if (__ballot(asr != 0.0)) {
        const double ar = fabs(asr);   // asin is monotonic: the rule thresholds are compared as angles
        const int rule = __ballot(ar > GL_ASR3) ? 4 : __ballot(ar > GL_ASR2) ? 3 : __ballot(ar > GL_ASR1) ? 2
                         : __ballot(ar > GL_ASR0) ? 1 : 0;
        const cdp_gl_t gl = (cdp_gl_t)(unsigned long long)(a.gl + 2 * gl_first(rule));
        const int nn = gl_nodes(rule);
        if (valid) {
          const int src = item & 63, row = item >> 6, ti = gbq + row;
          const double *e = tjb + (size_t)(ti + 1) * NEF * TILE + 2 * src;
          const double *g0 = a.atab + ((size_t)kq * a.Ta + ti) * NAF;
          const fo_d2 qxy = fo_ld2(e), qcs = fo_ld2(e + EF(2));
          // everything in units of the standard deviations (times sqrt 2) along x and y
          const double ix0 = g0[6], iy0 = g0[7];
          const double rx = (qxy.x - g0[0]) * ix0, ry = (qxy.y - g0[1]) * iy0;
          const double devx = g0[NAF + 2] * hdq * ix0, devy = g0[NAF + 3] * hdq * iy0;
          const double bxs = a.len3 * qcs.x * ix0, bys = a.len3 * qcs.y * iy0;
          const double ox = a.off_x * ix0, oy = a.off_y * iy0;
          double csum = 0.0;
#pragma unroll 1
          for (int i = 0; i < nn; ++i) {
            const double sn = fo_sin_halfpi(asr * gl[2 * i]);   // node and weight are wave-uniform: scalar loads
            const double c2 = 1.0 / fma(-sn, sn, 1.0);
            double S = 0.0;
#pragma unroll 1
            for (int jm = -1; jm <= 1; ++jm) {
              const double qx = rx - jm * devx, qy = ry - jm * devy;
#pragma unroll 1
              for (int b = -1; b <= 1; ++b) {
                const double cx = qx + b * bxs, cy = qy + b * bys;
                S += fo_corr_corners(exp_tab, cx - ox, cx + ox, cy - oy, cy + oy, 2.0 * sn, c2);
              }
            }
            csum = fma(gl[2 * i + 1], S, csum);
          }
          cpq[row * TILE + src] = fma(asr * (1.0 / 3.0), csum, cpq[row * TILE + src]);
        }
      }
    }
  };
  // Workgroup-wide pool (horizon-split form only: on the full grid, whose four waves hold four different agents, the lock step
  // of two barriers per chunk costs 9 %).  The gate work is the one part of the sweep that is NOT spread evenly: on the bench batch 56 of
  // the 256 agents have any sample inside the 5 m gate and 26 of them hold 84 % of the 1.4 million in-gate samples -- the wave
  // that holds such an agent evaluates up to seventeen batches of 36 x 64 erf for it while its three siblings have none, and
  // the workgroup lives as long as that wave (tools/sweep_stats.py; the model in DESIGN.md section 3.1 puts 5-20 % of the
  // wave slots of a launch into waiting for it).  So pass 1 only QUEUES its in-gate samples (a chunk's worth: up to 64 x TC per
  // wave), and at the end of pass 1 the four waves of the workgroup meet (the chunk loop runs in step for that: every wave
  // takes part in every round, with an empty queue where its agent slot is unused), pool their queues and deal the batches
  // of 64 round robin: every wave evaluates a quarter of the workgroup's samples, whoever queued them, and writes the
  // probabilities into the owner's rows.  A second barrier, then pass 2 as before.  Fuller batches come with it (one
  // remainder per workgroup and chunk instead of four).
  auto pool_round = [&](int qn_, int k_, double hd_, int gb_) {
    static_assert(!SPLIT || QWAVES == 4, "the pool's prefix over the waves' queue lengths is written for four waves");
    if (lane == 0) { pool_i[wave] = qn_; pool_i[QWAVES + wave] = k_; pool_i[2 * QWAVES + wave] = gb_; pool_hd[wave] = hd_; }
    __syncthreads();
    const int n0 = __builtin_amdgcn_readfirstlane(pool_i[0]), n1 = __builtin_amdgcn_readfirstlane(pool_i[1]);
    const int n2 = __builtin_amdgcn_readfirstlane(pool_i[2]), n3 = __builtin_amdgcn_readfirstlane(pool_i[3]);
    const int c1 = n0 + n1, c2 = c1 + n2, total = c2 + n3;
#pragma unroll 1
    for (int b = wave; (b << 6) < total; b += QWAVES) {
      const int i = (b << 6) + lane;
      const bool valid = i < total;
      const int o = valid ? (i >= n0) + (i >= c1) + (i >= c2) : 0;
      const int li = i - (o == 0 ? 0 : o == 1 ? n0 : o == 2 ? c1 : c2);
      int item = 0, kq = 0, gbq = 0;
      double hdq = 0.0;
      if (valid) { item = queue_all[o * QCAPX + li]; kq = pool_i[QWAVES + o]; gbq = pool_i[2 * QWAVES + o]; hdq = pool_hd[o]; }
      gate_items(valid, item, kq, hdq, gbq, cpbuf_all + o * (WROWS * TILE));
    }
    __syncthreads();
  };

  // agents of this wave: chunk -> (first agent, agents per wave), see SweepArgs::chunk_tab
  const int apw_ = SPLIT ? a.apw : fo_const(a.chunk_tab)[2 * chunk + 1];   // SPLIT: agents per WORKGROUP, one after the other
  const int k0 = SPLIT ? chunk * a.apw : fo_const(a.chunk_tab)[2 * chunk] + wave * apw_;
  // the samples this wave owns: everything, or time chunk `wave` of the agent the workgroup shares
  const int seg0 = SPLIT ? wave * TC : 0, seg1 = SPLIT ? min(seg0 + TC, a.T) : a.T;
  const int gfirst_ = max(seg0 - 1, 0);  // first harm / cp sample this wave evaluates for an agent
  for (int kk = 0; kk < apw_; ++kk) {
    const int k = k0 + kk;
    if (k >= A) break;
    const cdp_t G = fo_const(a.atab) + (size_t)k * a.Ta * NAF;
    const cdp_t C = fo_const(a.acst) + (size_t)k * NAC;
    const double hlB = C[0], hwB = C[1], hdev = C[2], Rsum = C[8];
    // coarse gate radius around the agent mean of the same sample, squared (fo_prep_agents_kernel, c[14]); wave-uniform
    double gate_far2;
    {
      const unsigned long long key = *(const __attribute__((address_space(4))) unsigned long long *)(C + 15);
      #ifdef FO_NO_SMAX   // (test-the-test builds: tests/test_sweep_gpu.py::test_gate_of_agents_that_jump_between_samples must fail)
      const double smax = 0.0 * (double)(unsigned)key;
#else
      const double smax = ((unsigned)(key >> 32) == (unsigned)a.gen) ? (double)__uint_as_float((unsigned)key) : 0.0;   // no key of this set: no step
#endif
      const double gf = (C[14] + smax + fabs(a.wb)) * (1.0 + 1e-9);
      const double gf2 = gf * gf;
      gate_far2 = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(gf2)), __builtin_amdgcn_readfirstlane(__double2loint(gf2)));
    }
    // Horizon-split form: the operands of the DCE probe (below) are asked for here, together with the agent's constants and
    // its length -- one round trip instead of two at the head of a workgroup that lives for ~15 us (the probe's choice of
    // samples only seeds a threshold; any sample of the segment serves).  Four samples, every second one of the segment.
    double sp_vx[4], sp_vy[4], sp_gx[4], sp_gy[4];
    if constexpr (SPLIT) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = min(seg0 + 2 * u, T - 1);
        const fo_d2 xy = fo_ld2(tj + (size_t)t * NEF * TILE);
        sp_vx[u] = xy.x; sp_vy[u] = xy.y;
        const cdp_t g = G + (size_t)t * NAF;
        sp_gx[u] = g[0]; sp_gy[u] = g[1];
      }
    }
    const int prot = fo_const(a.aint)[2 * k], L = fo_const(a.aint)[2 * k + 1];
    const int Lh = min(Tm1, L);

    if (L <= 0) {  // inactive slot (a spawn buffer that is only partly filled): no outputs enter any reduction
      if (SPLIT && wave > 0) continue;
      if (a.be_mask) a.be_mask[(size_t)k * a.Mp + m] = 0;
      if (PAIR) {
        const size_t ps_ = (size_t)A * M;
        for (int f = 0; f < FO_NPF; ++f) a.pair_f[(size_t)f * ps_ + (size_t)k * M + m] = NAN;
        for (int f = 0; f < FO_NPI; ++f) a.pair_i[(size_t)f * ps_ + (size_t)k * M + m] = 0;
      }
      if (LISTS) {
        const size_t ls = (size_t)A * Tm1 * M;
        for (int t = 0; t < Tm1; ++t) {
          if (lst_is32(LISTS)) fo_store_lists_f32((float *)a.lists, ls, ((size_t)k * Tm1 + t) * M + m, NAN, NAN, NAN, NAN, NAN);
          else fo_store_lists<false>(a.lists, ls, ((size_t)k * Tm1 + t) * M + m, NAN, NAN, NAN, NAN, NAN);
        }
      }
      continue;
    }

    // Everything below runs once per agent, on the full grid in one of three copies chosen at the end of this loop body
    // (wave-uniform): the harm model is a constant of the copy (HM; FIXED), so neither pass 1 nor pass 2 asks for it per sample
    // or per chunk, and what only the LR4S model reads -- the headings, the impact classes and their re-rating on a class
    // boundary -- is live in the LR4S copy alone.  (`lr4s` and `dvmax_mode` are plain constants rather than constexpr so that
    // the horizon-split form can run the same text with the model as a run-time value.)
    auto agent_body = [&](auto hm_tag) {
    constexpr bool FIXED = hm_fixed<decltype(hm_tag)>::value;
    const int HM = hm_tag.value;   // (a constant in the copies of the full grid)
    // Per-agent state that lives across the time chunks.
    // DCE (dce.py:69-99) = the minimum over t of the rounded rectangle distance and the EARLIEST t that attains it (the
    // reference's early stop at 0 only cuts samples after the first zero) -- a result that does not depend on the
    // order in which the samples are visited.  So a probe phase first finds, per lane, the sample where the reference
    // points are closest (a cheap loop over t) and evaluates the exact distance there; the time-ordered loop below
    // then only pays for the exact geometry of samples whose lower bound (centre distance minus circumradii, then
    // the four SAT separations) can still reach the running minimum or tie it -- a wave-level skip otherwise.
    // dce is kept in whole millimetres; thr2 = ((dce + 0.51) mm)^2 and thrR2 = ((dce + 0.51) mm + R)^2 are what the SAT
    // bound and the centre distance have to undercut (0.51: a sample that rounds to the same millimetre may still
    // win the tie on t).
    double dce = INFINITY, thr2 = INFINITY, thrR2 = INFINITY;
    int tdce = 0;
    if (do_dce && !(ablate & 1) && seg0 < min(L, seg1)) {
      const int Ld = min(L, seg1);
      double bestc = INFINITY;
      int tb = seg0;
      // latency-bound by construction (two loads, five operations per sample): eight samples in flight at a time.
      // Every second sample is enough for a seed (on the bench workload the exact geometry runs as rarely as with all
      // of them; stride 4 would cost a quarter more) -- and halves the loads of this phase.
      constexpr int PS = 2;
      // The running minimum carries its sample number in the low mantissa bits (v_bfi_b32 + v_min_f64: the earlier
      // sample wins a tie, a repeat of the last sample never does, as with a strict comparison) -- instead of a compare and
      // three v_cndmask_b32 on vcc per sample: a v_cndmask on vcc holds the SIMD for 14 cycles where an add holds it
      // for 4 (tools/microbench/valu_rate.hip; -1.4 % of the kernel).  The probe only SEEDS the bound: the 2^-47 it moves a
      // squared distance by cannot change a result.
      if constexpr (SPLIT) {
        asm volatile("; probe operands resident" ::"s"(sp_gx[0]), "s"(sp_gy[0]), "s"(sp_gx[1]), "s"(sp_gy[1]), "s"(sp_gx[2]),
                     "s"(sp_gy[2]), "s"(sp_gx[3]), "s"(sp_gy[3]));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = seg0 + 2 * u;
          const double rx = sp_gx[u] - sp_vx[u], ry = sp_gy[u] - sp_vy[u];
          const double c2 = fo_pack_low(fma(rx, rx, ry * ry), u);
          if (t < Ld) bestc = fo_vmin(bestc, c2);   // (wave-uniform)
        }
        tb = seg0 + 2 * (int)(__double2loint(bestc) & 7);   // (bestc = inf -- NaN positions only: sample 0 of the segment)
      } else {
        int slot = 0;
#pragma unroll 1
        for (int t8 = 0; seg0 + t8 * PS < Ld; t8 += 8) {
          double vx[8], vy[8], gpx[8], gpy[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int t = min(seg0 + (t8 + u) * PS, Ld - 1);
            const fo_d2 xy = fo_ld2(tj + (size_t)t * NEF * TILE);
            vx[u] = xy.x;
            vy[u] = xy.y;
            const cdp_t g = G + (size_t)t * NAF;   // eight scalar loads in flight as well (one lgkmcnt wait for all)
            gpx[u] = g[0];
            gpy[u] = g[1];
          }
          asm volatile("; probe operands resident" ::"s"(gpx[0]), "s"(gpy[0]), "s"(gpx[1]), "s"(gpy[1]), "s"(gpx[2]),
                       "s"(gpy[2]), "s"(gpx[3]), "s"(gpy[3]), "s"(gpx[4]), "s"(gpy[4]), "s"(gpx[5]), "s"(gpy[5]),
                       "s"(gpx[6]), "s"(gpy[6]), "s"(gpx[7]), "s"(gpy[7]));
          double blk = INFINITY;
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const double rx = gpx[u] - vx[u], ry = gpy[u] - vy[u];
            blk = fo_vmin(blk, fo_pack_low(fma(rx, rx, ry * ry), u));
          }
          // (block against block: one comparison per eight samples -- the mask in a scalar pair, not in vcc)
          const unsigned long long lt = __builtin_amdgcn_fcmp(blk, bestc, 4 /* olt */);
          bestc = fo_vmin(bestc, blk);
          slot = fo_sel_b32(lt, slot, t8);
        }
        tb = min(seg0 + (slot + (int)(__double2loint(bestc) & 7)) * PS, Ld - 1);
      }
      const double *e = tj + (size_t)tb * NEF * TILE;                   // per-lane sample: gathers
      const double *g = a.atab + ((size_t)k * a.Ta + tb) * NAF;
      const fo_d2 exy = fo_ld2(e), ecs = fo_ld2(e + EF(2));
      dce = fo_rect_mm(exy.x, exy.y, ecs.x, ecs.y, g[0], g[1], g[2], g[3], hlA, hwA, a.wb, hlB, hwB);
      tdce = tb;
      const double thr = (dce + 0.51) * 1e-3;
      thr2 = thr * thr;
      thrR2 = (thr + Rsum) * (thr + Rsum);
    }
    double max_er = -INFINITY, max_or = -INFINITY, max_eh = -INFINITY, max_oh = -INFINITY, max_cp = -INFINITY;
    double oh_at_cp = 0.0;
    int idx_or = 0, idx_cp = 0;
    // Without the per-sample lists the harm values are needed at the gate samples only (risk = harm x cp); their maxima
    // are the logistic of the smallest argument -- 1/(1 + exp(nz)) falls with nz -- so the other samples keep a running
    // minimum of the two arguments and the logistic is taken once per pair.
    double nze_min = INFINITY, nzo_min = INFINITY;
    // Without lists, for the agents of the two-coefficient models (pedestrian, LR1S: prot == 0) with the usual signs of
    // the speed coefficients (both slopes <= 0): the smallest logistic argument belongs to the LARGEST relative speed,
    // fma(k, dv, c) is monotonic in dv and so is its rounding -- pass 1 keeps the running maximum of dv (as -dv in
    // nze_min, no new register) and pass 2 visits the gate rows only.  Wave-uniform.
    // (round 4: in EVERY output mode -- the per-wave ring holds the SQUARED relative speed, pass 1 takes no square root, and
    // the agent runs in one of three bodies (agent_body's tag): HM_DVMAX for these agents, HM_LR4S, HM_GENERIC for the rest
    // -- agents without a harm model, speed coefficients of unusual sign.  With the lists the running maximum is kept by
    // pass 2, which walks every sample anyway; without them by pass 1, and pass 2 visits the gate rows only.  The maxima are
    // the same arithmetic in all three output modes: logistic at sqrt(max dv^2).)
    const bool dvmax_mode = HM == HM_DVMAX;
    // List stores: the three blocks (cp | harm pairs | risk pairs) from per-agent scalar bases plus two running 32-bit
    // lane offsets (element size 1x and 2x) -- no 64-bit address arithmetic per sample (fo_sweep_run sends batches whose
    // (T-1) M pair elements pass 4 GB to the generic kernel)
    const size_t ls = (size_t)A * Tm1 * M;
    constexpr unsigned LE = lst_is32(LISTS) ? 4u : 8u;   // list element size
    char *const lb0 = (char *)a.lists + (size_t)k * Tm1 * M * LE;
    char *const lb1 = (char *)a.lists + (ls + (size_t)k * Tm1 * M * 2) * LE;
    char *const lb2 = (char *)a.lists + (3 * ls + (size_t)k * Tm1 * M * 2) * LE;
    unsigned lo1 = (unsigned)(gfirst_ * M + m) * LE, lo2 = (unsigned)(gfirst_ * M + m) * (2u * LE);
    // logistic arguments as one fma of dv: the speed coefficient times the mass split is folded per agent
    // (harm_model.py:96-97: ego_dv = m_obs/(m_ego+m_obs) dv, obs_dv = m_ego/(m_ego+m_obs) dv)
    const bool lr4s = HM == HM_LR4S;
    // The logistic slopes and offsets (fo_prep_agents_kernel) are wave-uniform, but the scalar registers are taken:
    // parked in LDS, pass 2 reads them back into vector registers that are free by then (held across pass 1 they would
    // cost eight VGPRs at its register peak).
    if (lane < 4) hk[lane] = a.acst[(size_t)k * NAC + 10 + lane];
    // LR4S impact classes (0 front, 1 side, 2 rear) of the ego's and the obstacle's occupants: two bits per sample,
    // slot t & 15 (a chunk and its predecessor's last sample are live at once: TC + 1 <= 16 slots)
    [[maybe_unused]] unsigned cls_e = 0u, cls_o = 0u;   // (the LR4S copy's)

    // The horizon is walked in chunks of TC iterations, two passes per chunk.
    //  pass 1, iteration t: everything that needs the poses -- DCE(t); the relative speed of sample t (harm_model.py:
    //          92-94) into the wave's ring in LDS and, for LR4S agents, the impact classes of sample t; the gate of
    //          sample t-1 (ego t, agent mean t-1, agent heading t: Q1), so chunk [t0, t1) owns the gate samples
    //          [t0-1, t1-1), whose collision probabilities go to row (g - t0 + 1) of the wave's cp buffer.
    //  pass 2, samples [t0-1, t1-1): logistic models, risk, maxima, lists -- from LDS and registers only: no vector
    //          or scalar load shares a counter with the list stores (vmcnt retires loads and stores in issue order, so
    //          a load behind five stores per iteration used to wait for their acknowledgement).
    const int gfirst = gfirst_;
    // (Measured and not kept, round 3: two register sets for the current / next rows that swap roles, the loop
    // unrolled by two, instead of one set rotated by seven v_mov_b64 and ten s_mov per sample -- 0.552 against 0.541 ms:
    // 30 spilled registers instead of 8 and a quarter more code cost more than the copies.)
    // The ego row a chunk starts with is re-loaded at the chunk's start although pass 1 of the chunk before has already
    // fetched it (its last iteration prefetches row t1): carried over pass 2, the 14 live registers cost more than the
    // wait of the loads behind that pass's list stores (float32 lists 0.562 against 0.552 ms).
    fo_d2 nxy, ncs, nvv;
    [[maybe_unused]] double nth_ = 0.0;   // the ego's heading angle of the next sample: read by the LR4S copy only
    for (int t0 = seg0; t0 < seg1; t0 += TC) {
      const int t1 = min(t0 + TC, T);
      // A segment other than the first also needs the relative speed and the impact classes of the sample before it
      // (pass 2 covers the samples [t0-1, t1-1)): its pass 1 starts one sample early, for that part only.
      const int tl = (SPLIT && t0 > 0) ? t0 - 1 : t0;
      const int gbase = t0 - 1;  // gate sample of buffer row 0

      // (without the workgroup-wide pool: evaluates this wave's n (<= 64) queued samples)
      auto process = [&](int n) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        gate_items(lane < n, lane < n ? (int)q[lane] : 0, k, hdev, gbase, cpw);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      };

      // ---------------------------------------------------------------- pass 1: DCE + harm geometry + gate -> queue
      // Every operand of iteration t was requested one iteration earlier: the ego row t+1 (vector loads) and the
      // agent row t+1 (scalar loads) are issued at the top and first used at the top of the next iteration.
      unsigned gmask = 0u;  // bit row: gate sample gbase + row is inside the 5 m gate for this lane
      unsigned wgate = 0u;  // the same for the whole wave (uniform): some lane is inside the gate.  Bits 16 + (t & 15)
                            // of the same scalar: some lane's impact angle of sample t may sit on a class boundary
      int qn = 0;
      // Relative speeds: sample t sits in row t - gbase of the wave's DVR rows.  Pass 2 of this chunk starts one sample
      // before it (row 0), which the chunk before left in its last row.
      if (!(SPLIT && t0 > 0) && t0 > seg0) dvw[lane] = dvw[TC * TILE + lane];
      // the sample ranges of the DCE and of the gate as one unsigned comparison each (scalar instructions are not free:
      // DESIGN.md section 3.1): DCE on [t0, L), gate on [max(t0, 1), L)
      const bool dce_on = do_dce && !(ablate & 1), gate_on = do_cp && !(ablate & 2);
      const int rng_n = (dce_on || gate_on) ? max(L - t0, 0) : 0;
      const double gate_far2c = gate_on ? gate_far2 : -1.0;   // (no distance is below -1: the test never passes)
      // sample 0 has no gate (there is no sample -1): the radius of the chunk's first sample is -1 there, the loop sets
      // the real one from its second sample on -- cheaper than a test of t per sample
      double gate_far2t = (tl == 0) ? -1.0 : gate_far2c;
      if (!dce_on) thrR2 = -1.0;
      const bool geo = do_hr && !(ablate & 4);
      const double *e0_ = tj + (size_t)tl * NEF * TILE;
      nxy = fo_ld2(e0_); ncs = fo_ld2(e0_ + EF(2)); nvv = fo_ld2(e0_ + EF(6));
      if (lr4s) nth_ = e0_[EF(4)];
      // (rows are addressed without clamping -- rows past an agent's length are read but never used, every use sits
      // behind t < L; the tables end in spare rows, fo_sweep_set_agents / fo_sweep_run)
      const cdp_t gr0 = G + (size_t)tl * NAF;
      double px = gr0[0], py = gr0[1], npx = px, npy = py;
      // Only the mean of the next row is fetched a sample ahead (the first thing a sample needs); heading and velocity
      // are re-loaded IN PLACE right after their last use in a sample -- no second register set, no copies
      double pc = gr0[2], ps = gr0[3], pvx = gr0[8], pvy = gr0[9];
      [[maybe_unused]] double pyaw = 0.0;   // the agent's heading angle only enters the LR4S model
      if (!FIXED || lr4s) pyaw = gr0[4];
      // Scalar loads return out of order, so any use of an s_load result waits for lgkmcnt(0).  Pinning the per-agent
      // constants and the first rows here (an empty asm that names them as SGPR inputs) drains the counter before the
      // loop, which leaves the in-loop wait to cover only the row that was prefetched one iteration ago.
      if (!FIXED || lr4s)
        asm volatile("; scalar operands resident" ::"s"(hlB), "s"(hwB), "s"(hdev), "s"(Rsum), "s"(gate_far2), "s"(px),
                     "s"(py), "s"(pc), "s"(ps), "s"(pvx), "s"(pvy), "s"(pyaw));
      else
        asm volatile("; scalar operands resident" ::"s"(hlB), "s"(hwB), "s"(hdev), "s"(Rsum), "s"(gate_far2), "s"(px),
                     "s"(py), "s"(pc), "s"(ps), "s"(pvx), "s"(pvy));
      SW_STAMP(0);
      // rows t+1 as running 32-bit byte offsets from the (uniform) bases of this tile's and this agent's rows: one add
      // each per sample instead of a 64-bit multiply-add, and the loads take the base from scalar registers
      unsigned eoff = (unsigned)((tl * NEF * TILE + 2 * lane) * sizeof(double));
      unsigned goff = (unsigned)(tl * NAF * sizeof(double));
      for (int t = tl; t < t1; ++t) {
        // (Round 5, measured and dropped: the ego's velocity -- and heading -- of sample t asked for at the top of iteration t
        // instead of one iteration ahead with the pose -- three register pairs and three v_mov_b64 less per sample -- and no row
        // fetched ahead at all: 0.536-0.540 ms against 0.542, inside the noise, and 2 % slower together with the shorter erf step.)
        const double ex = nxy.x, ey = nxy.y, ec = ncs.x, es = ncs.y, evx = nvv.x, evy = nvv.y;
        [[maybe_unused]] const double eth = nth_;
        {
          eoff += (unsigned)(NEF * TILE * sizeof(double));
          goff += (unsigned)(NAF * sizeof(double));
          const double *e1 = (const double *)((const char *)tjb + eoff);
          nxy = fo_ld2(e1); ncs = fo_ld2(e1 + EF(2)); nvv = fo_ld2(e1 + EF(6));
          const cdp_t g1 = (cdp_t)((const __attribute__((address_space(4))) char *)G + goff);
          npx = g1[0]; npy = g1[1];
          if (lr4s) nth_ = e1[EF(4)];   // the headings only enter the LR4S model
        }
        const cdp_t g1 = (cdp_t)((const __attribute__((address_space(4))) char *)G + goff);
        if ((unsigned)(t - t0) < (unsigned)rng_n) {
          const double ccx = ex + a.wb * ec, ccy = ey + a.wb * es;  // convert_dynamic_obstacle.py:73
          const double dx = px - ccx, dy = py - ccy;
          const double dd = dx * dx + dy * dy;   // shared by the DCE and the gate: both start from a coarse distance test
          // the centres must be close enough.  (Nothing is to be gained after the earliest zero: the block below sets
          // thrR2 to -1 at the sample that holds it -- a zero found here, or the probe's, whose sample always passes this
          // test: overlapping rectangles have their centres within the sum of the circumradii -- so that one comparison
          // per sample serves both conditions.)
          const bool near = dd < thrR2;
          if (__ballot(near)) {
            const double cr = pc * ec + ps * es, sr = ps * ec - pc * es;
            const double ax = ec * dx + es * dy, ay = ec * dy - es * dx;   // agent centre in the ego frame
            const double ux = hlB * cr, uy = hlB * sr, wx = -hwB * sr, wy = hwB * cr;
            const double bx = -(pc * dx + ps * dy), by = -(pc * dy - ps * dx);  // ego centre in the agent frame
            const double vx = hlA * cr, vy = -hlA * sr, zx = hwA * sr, zy = hwA * cr;
            // separations along the four face normals: each is a lower bound of the distance, all <= 0 iff overlapping
            const double s1 = fabs(ax) - (hlA + fabs(ux) + fabs(wx)), s2 = fabs(ay) - (hwA + fabs(uy) + fabs(wy));
            const double s3 = fabs(bx) - (hlB + fabs(vx) + fabs(zx)), s4 = fabs(by) - (hwB + fabs(vy) + fabs(zy));
            const double lb = fmax(fmax(s1, s2), fmax(s3, s4));
            const bool overlap = !(lb > 0.0);
            bool need = near && (overlap || lb * lb < thr2);
            if (__ballot(need)) {
              // Second, tighter bound before the eight corner distances: separated along BOTH axes of one frame, the
              // rectangles are at least the diagonal of the two gaps apart (the other one's bounding box in that frame
              // misses the corner).  On the bench workload this takes a third off the exact evaluations.
              const double g1 = fmax(s1, 0.0), g2 = fmax(s2, 0.0), g3 = fmax(s3, 0.0), g4 = fmax(s4, 0.0);
              const double q = fmax(fma(g1, g1, g2 * g2), fma(g3, g3, g4 * g4));
              need = need && (overlap || q < thr2);
            }
            if (__ballot(need)) {
              double nmm = 0.0;
              if (__ballot(need && !overlap)) {
                double d2 = fo_pt_box2(ax + ux + wx, ay + uy + wy, hlA, hwA);
                d2 = fmin(d2, fo_pt_box2(ax + ux - wx, ay + uy - wy, hlA, hwA));
                d2 = fmin(d2, fo_pt_box2(ax - ux + wx, ay - uy + wy, hlA, hwA));
                d2 = fmin(d2, fo_pt_box2(ax - ux - wx, ay - uy - wy, hlA, hwA));
                d2 = fmin(d2, fo_pt_box2(bx + vx + zx, by + vy + zy, hlB, hwB));
                d2 = fmin(d2, fo_pt_box2(bx + vx - zx, by + vy - zy, hlB, hwB));
                d2 = fmin(d2, fo_pt_box2(bx - vx + zx, by - vy + zy, hlB, hwB));
                d2 = fmin(d2, fo_pt_box2(bx - vx - zx, by - vy - zy, hlB, hwB));
                if (!overlap) nmm = fo_mm(d2);
              }
              if (need && (nmm < dce || (nmm == dce && t < tdce))) {
                dce = nmm;
                tdce = t;
                const double thr = (nmm + 0.51) * 1e-3;
                thr2 = thr * thr;
                thrR2 = (thr + Rsum) * (thr + Rsum);
              }
            }
            if (near && dce == 0.0 && t >= tdce) thrR2 = -1.0;   // the earliest zero is in: no later sample can beat it
          }
          // gate of sample t-1 (collision_probability.py:44-67,75): ego sample t, agent mean t-1, agent heading t.  The two
          // displaced means are hdev away from the mean: beyond 5 m + hdev none of the three can be in the gate, and the
          // mean of sample t-1 is at most the agent's longest step from the one of sample t (gate_far2)
          if (__ballot(dd <= gate_far2t)) {
            // (scalar loads on the rare path; the row was read a sample ago)
            const cdp_t gq = (cdp_t)((const __attribute__((address_space(4))) char *)G + (goff - 2u * (unsigned)(NAF * sizeof(double))));
            const double m2 = fo_gate_d2(gq[0], gq[1], pc * hdev, ps * hdev, ex, ey);
            // the reference tests the ROUNDED distance, !(sqrt(m2) > 5.0) (collision_probability.py:67,75).  The
            // correctly rounded square root of m2 is 5.0 up to and including m2 = 25 + one ulp (sqrt(25 (1 + d)) = 5 (1 + d/2),
            // half an ulp of 5.0 is 4.4e-16, one ulp of 25 is 3.6e-15): no square root needed
            const bool ing = m2 <= 25.000000000000004;
            const unsigned long long bal = __ballot(ing);
            if (bal) {
              const int row = t - t0;  // = (t - 1) - gbase
              const int pos = qn + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
              if (ing) {
                q[pos] = (unsigned short)(lane | (row << 6));
                gmask |= 1u << row;
              }
              wgate |= 1u << row;
              qn += __popcll(bal);
              if (!SPLIT && qn >= 64) {
                process(64);
                const int rest = qn - 64;
                unsigned short tmp = 0;
                if (lane < rest) tmp = q[64 + lane];
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (lane < rest) q[lane] = tmp;
                qn = rest;
              }
            }
          }
        }
        // relative speed of sample t (harm_model.py:92-94): sqrt(ve^2 + va^2 + 2 ve va cos(pdof)), pdof = yaw - theta
        // + pi, is the length of the difference of the two velocity vectors; capped (1e4 m/s) so that the logistic
        // arguments of pass 2 stay in the range of the table exp without a clamp of their own
        double dvx = evx - pvx, dvy = evy - pvy;
        {
          // (last use of this sample's velocity above: the next row's takes its place.  The empty asm orders the load
          // behind the subtraction -- issued earlier it would need registers of its own and a copy)
          unsigned gb = __builtin_amdgcn_readfirstlane(goff);
#if !FO_TRACE   // (the time-line build does without the ordering: its extra kernel argument upsets the uniformity analysis)
          asm volatile("" : "+v"(dvx), "+v"(dvy), "+s"(gb));
#endif
          const cdp_t g2 = (cdp_t)((const __attribute__((address_space(4))) char *)G + gb);
          pvx = g2[8]; pvy = g2[9];
        }
        if (geo && t < Lh) {
          // squared (<= 1e8: the prep kernels cap the speeds at 5e3 m/s); pass 2 takes the root where it needs the speed
          const double dv2_ = fo_sq_sum_pos(dvx, dvy);
          dvw[(t - gbase) * TILE + lane] = dv2_;
          if (LISTS == LST_NONE && dvmax_mode) nze_min = fo_vmin_neg(nze_min, dv2_);
          if (lr4s) {
            // the impact angles only enter the LR4S model, and only through their class (front / side / rear)
            double ddx = px - ex, ddy = py - ey;
            // atan2(0, 0) = 0: dx = 1 for coincident centres -- |dx| + |dy| == 0, and only the high word of dx has to change
            ddx = __hiloint2double(fabs(ddx) + fabs(ddy) == 0.0 ? 0x3ff00000 : __double2hiint(ddx), __double2loint(ddx));
            const float relc = fo_atan2_crude((float)ddy, (float)ddx);
            bool be_, bo_;
            const unsigned ce = fo_lr4s_class(ddx, ddy, ec, es, relc, 0.0f, (float)eth, false, be_);
            const unsigned co = fo_lr4s_class(ddx, ddy, pc, ps, relc, 3.14159265f, (float)pyaw, true, bo_);
            // (a NaN or +-inf of the float32 estimate -- offsets of ~1e-40 m: both casts flush to zero -- goes the same way)
            if (__ballot(be_ || bo_ || !(fabsf(relc) <= 4.0f))) wgate |= 0x10000u << (t & 15);   // re-rated after the loop (rare; see there)
            const int sh = (t & 15) * 2;
            cls_e = (cls_e & ~(3u << sh)) | (ce << sh);
            cls_o = (cls_o & ~(3u << sh)) | (co << sh);
          }
        }
        {
          // the mean fetched at the top of this sample becomes the current one BEFORE the next loads are issued: scalar
          // loads return out of order, so the wait in front of these copies would otherwise cover the loads below
          px = npx; py = npy;
          unsigned gb = __builtin_amdgcn_readfirstlane(goff);
#if !FO_TRACE
          asm volatile("" : "+s"(px), "+s"(py), "+s"(gb));
#endif
          const cdp_t g2 = (cdp_t)((const __attribute__((address_space(4))) char *)G + gb);
          pc = g2[2]; ps = g2[3];
          if (lr4s) pyaw = g2[4];
        }
        gate_far2t = gate_far2c;
      }
      if (SPLIT) pool_round(qn, k, hdev, gbase);
      else if (qn > 0) process(qn);
      wgate = __builtin_amdgcn_readfirstlane(wgate);  // uniform by construction; says so to the register allocator
      if (const unsigned wband = wgate >> 16; lr4s && wband) {
        // Impact angles on a class boundary to within rounding: the reference's own floating-point route (float64 atan2,
        // the subtraction, the comparison with 45/180 pi; harm_model.py:86-90, logistic_regression.py:28-42) decides
        // those samples -- here, outside the loop whose registers a float64 atan2 does not fit into.
        for (unsigned wb = wband; wb; wb &= wb - 1u) {
          const int slot = __builtin_ctz(wb), t = tl + ((slot - tl) & 15);
          const double *e0 = tj + (size_t)t * NEF * TILE;
          const fo_d2 xy = fo_ld2(e0), cs = fo_ld2(e0 + EF(2));
          const double th0 = e0[EF(4)];
          const cdp_t g0 = G + (size_t)min(t, L - 1) * NAF;
          double ddx = g0[0] - xy.x, ddy = g0[1] - xy.y;
          if (ddx == 0.0 && ddy == 0.0) ddx = 1.0;
          // (an offset whose float32 casts under- or overflow -- the estimate above was NaN and "far" read false: both classes
          // by the float64 route)
          const float crude_ = fo_atan2_crude((float)ddy, (float)ddx);
          const bool nf_ = !(fabsf(crude_) <= 4.0f);   // NaN (0 * inf) or +-inf (a float32 denormal times the reciprocal of one)
          const bool be_ = nf_ || fo_lr4s_on_boundary(ddx, ddy, cs.x, cs.y), bo_ = nf_ || fo_lr4s_on_boundary(ddx, ddy, g0[2], g0[3]);
          if (be_ || bo_) {
            const unsigned both = fo_lr4s_classes_ref(ddx, ddy, th0, g0[4]);
            const int sh = slot * 2;
            if (be_) cls_e = (cls_e & ~(3u << sh)) | ((both & 3u) << sh);
            if (bo_) cls_o = (cls_o & ~(3u << sh)) | ((both >> 2) << sh);
          }
        }
      }

      SW_STAMP(1);
      // ---------------------------------------------------------------- pass 2: harm, risk, maxima, lists
      // of the gate samples g in [max(t0-1, 0), t1-1) -- harm index g, cp index g (Q6)
      const int g0s = max(gbase, 0), g1s = t1 - 1;
      if ((do_cp || do_hr) && g0s < g1s) {
        // one instantiation per harm model: the LR4S path (impact classes -> logistic offsets) and the pedestrian /
        // LR1S path keep separate register and constant sets
        auto pass2 = [&](auto hm_tag) {
          constexpr int HM = decltype(hm_tag)::value;
          constexpr bool LR4S = HM == HM_LR4S, DVMAX = HM == HM_DVMAX;
          const double ke_ = hk[0], ko_ = hk[1], ce_ = hk[2], co_ = hk[3];
          // float32 list entries of the two-coefficient models: logistic arguments in units of ln 2 (v_exp_f32 is 2^x)
          const float kef_ = (float)(ke_ * 1.4426950408889634), kof_ = (float)(ko_ * 1.4426950408889634);
          const float cef_ = (float)(ce_ * 1.4426950408889634), cof_ = (float)(co_ * 1.4426950408889634);
          // LDS reads of sample t+1 are issued while sample t is evaluated
          double dvn = dvw[(g0s - gbase) * TILE + lane];
          double zen = 0.0, zon = 0.0;
          if (LR4S) {
            const int sh = (g0s & 15) * 2;
            zen = zc_tab[(cls_e >> sh) & 3u];
            zon = zc_tab[(cls_o >> sh) & 3u];
          }
          // Rows that take the long way (wave-uniform mask, one bit per buffer row): some lane of the wave is inside the
          // gate, the wave's first sample (it seeds the running maxima and indices), and the samples past the harm
          // length.  On every other row -- 97 % of the samples of the bench workload -- every probability is zero, so are
          // the risks, and none of the maxima or indices can move.
          unsigned slow = wgate & 0xffffu;
          if (gfirst >= g0s) slow |= 1u << (gfirst - gbase);
          unsigned hvrows = geo ? ~0u : 0u;   // bit row: the sample lies inside the harm length
          if (geo && Lh < g1s) hvrows = ~(~0u << max(Lh - gbase, 0));
          slow = __builtin_amdgcn_readfirstlane(slow | ~hvrows);
          hvrows = __builtin_amdgcn_readfirstlane(hvrows);
          if (LISTS == LST_NONE && DVMAX) {
            // only the rows that take the long way; the harm maxima come from the running maximum of dv^2 (epilogue)
            unsigned todo = slow & (~0u << (g0s - gbase)) & ~(~0u << (g1s - gbase));
            while (todo) {
              const int row = __builtin_ctz(todo), t = gbase + row;
              todo &= todo - 1u;
              const double dv = fo_sqrt_pos(dvw[row * TILE + lane]);
              double cp = 0.0;
              if ((gmask >> row) & 1u) cp = cpw[row * TILE + lane];
              if ((hvrows >> row) & 1u) {
                const double eh = fo_logistic_neg<false>(exp_tab, fma(ke_, dv, ce_));
                const double oh = fo_logistic_neg<false>(exp_tab, fma(ko_, dv, co_));
                const double er = eh * cp, orr = oh * cp;
                if (er > max_er || er != er) max_er = er;
                if (orr > max_or) { max_or = orr; idx_or = t; }
                if (cp > max_cp) { max_cp = cp; idx_cp = t; oh_at_cp = oh; }
              } else if (cp > max_cp) {
                max_cp = cp; idx_cp = t; oh_at_cp = NAN;
              }
            }
          } else {
          auto row_step = [&](const int t, auto fast_tag) {
            // FASTROW (compile time): the row lies inside the harm length and no lane of the wave is inside the gate -- the
            // two mask tests, the branch on them and the long way's code are not in this copy of the body
            constexpr bool FASTROW = decltype(fast_tag)::value;
            const int row = t - gbase;
            const double dv = dvn, ze = zen, zo = zon;
            dvn = dvw[(row + 1) * TILE + lane];
            if (LR4S) {
              const int sh = ((t + 1) & 15) * 2;
              zen = zc_tab[(cls_e >> sh) & 3u];
              zon = zc_tab[(cls_o >> sh) & 3u];
            }
            double eh = NAN, oh = NAN, er = NAN, orr = NAN, cp = 0.0;
            float ehf = NAN, ohf = NAN;   // float32 lists: the harm entries
            // harm of a sample inside the harm length (wave-uniform)
            auto harm = [&]() {
              if (FO_X & 8) {
                eh = dv; oh = ze + zo;
                return;
              }
              if (DVMAX) {
                // two-coefficient model, the usual signs: the maxima come from the running maximum of dv^2 (epilogue); what
                // is left per sample is the list entry -- float64: root + two table logistics; float32: root, two fmas
                // and two logistics on the hardware transcendentals (|error| < 4e-7: v_sqrt_f32 and the float32 fma add
                // 1e-7 |nz| to the argument, the slope of the logistic is <= 1/4)
                if (LISTS != LST_NONE) nze_min = fo_vmin_neg(nze_min, dv);
                if (lst_exact(LISTS)) {
                  const double dvs = fo_sqrt_pos(dv);
                  eh = fo_logistic_neg<false>(exp_tab, fo_fma3(ke_, dvs, ce_));
                  oh = fo_logistic_neg<false>(exp_tab, fo_fma3(ko_, dvs, co_));
                } else if (LISTS == LST_F32) {
                  const float dvf = __builtin_amdgcn_sqrtf((float)dv);
                  ehf = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fmaf(kef_, dvf, cef_)));
                  ohf = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fmaf(kof_, dvf, cof_)));
                }
                return;
              }
              const bool model = LR4S || prot == 0;   // wave-uniform; otherwise harm is 1 on both sides
              const double dvs = fo_sqrt_pos(dv);      // (the ring holds dv^2)
              const double nze = LR4S ? fma(ke_, dvs, ze) : fo_fma3(ke_, dvs, ce_), nzo = LR4S ? fma(ko_, dvs, zo) : fo_fma3(ko_, dvs, co_);
              if (lst_exact(LISTS) || !model) {
                eh = model ? fo_logistic_neg<false>(exp_tab, nze) : 1.0;
                oh = model ? fo_logistic_neg<false>(exp_tab, nzo) : 1.0;
                max_eh = fo_vmax(max_eh, eh);
                max_oh = fo_vmax(max_oh, oh);
                if (LISTS == LST_F32) { ehf = 1.0f; ohf = 1.0f; }
              } else {
                nze_min = fo_vmin(nze_min, nze);   // (neither is ever NaN: no canonicalising pair of v_max around it)
                nzo_min = fo_vmin(nzo_min, nzo);
                if (LISTS == LST_F32) {   // float32 list entries: hardware exp / rcp (the maxima above stay float64)
                  ehf = fo_logistic_neg_f32(nze);
                  ohf = fo_logistic_neg_f32(nzo);
                }
              }
            };
            const bool hv = FASTROW ? true : (hvrows >> row) & 1u;  // wave-uniform: geo && t < Lh
            const bool slow_row = FASTROW ? false : (slow >> row) & 1u;
            if (hv) harm();
            float cpf = 0.0f, erf_ = 0.0f, orf = 0.0f;   // float32 lists: what they get (constants on the short branch)
            if (!slow_row) {
              er = 0.0;
              orr = 0.0;
            } else {
              if ((gmask >> row) & 1u) cp = cpw[row * TILE + lane];
              if (!lst_exact(LISTS) && hv && !(FO_X & 8) && (LR4S || DVMAX || prot == 0)) {   // the harm values themselves, where a risk may need them
                const double dvs = fo_sqrt_pos(dv);
                eh = fo_logistic_neg<false>(exp_tab, LR4S ? fma(ke_, dvs, ze) : fma(ke_, dvs, ce_));
                oh = fo_logistic_neg<false>(exp_tab, LR4S ? fma(ko_, dvs, zo) : fma(ko_, dvs, co_));
                if (LISTS == LST_F32) { ehf = (float)eh; ohf = (float)oh; }   // so that risk = harm x cp holds in the lists too
              }
              if (hv) {
                er = eh * cp;
                orr = oh * cp;
                // (a NaN probability -- an agent row without a usable covariance -- sticks in max_er, from where the
                // pair outputs below pick it up; v_max would drop it)
                if (er > max_er || er != er) max_er = er;
                if (orr > max_or) { max_or = orr; idx_or = t; }
              }
              if (cp > max_cp) { max_cp = cp; idx_cp = t; oh_at_cp = oh; }
              if (lst_is32(LISTS)) { cpf = (float)cp; erf_ = (float)er; orf = (float)orr; }
            }
            // FO_LISTS_F32_EXACT: the float64 harm values, rounded at the store.  (The probability and the risks are converted on
            // the rows that have them, above; on the others they are the float32 constants 0 -- converted behind the branches, the
            // zeros cost three v_mov_b64 and three v_cvt_f32_f64 per sample on 97 % of the rows.  Round 5: the stores moved INTO
            // the two branches, the short one with a single v_mov_b64 for its three zeros, made the allocator rotate the six
            // running maxima through copies in every iteration -- thirteen moves for two saved.)
            if (LISTS == LST_F32X) { ehf = (float)eh; ohf = (float)oh; }
            if (LISTS == LST_F64) {
              __builtin_nontemporal_store(cp, (double *)(lb0 + lo1));
              __builtin_nontemporal_store(fo_d2{eh, oh}, (fo_d2 *)(lb1 + lo2));
              __builtin_nontemporal_store(fo_d2{er, orr}, (fo_d2 *)(lb2 + lo2));
            } else if (lst_is32(LISTS)) {
              __builtin_nontemporal_store(cpf, (float *)(lb0 + lo1));
              __builtin_nontemporal_store(fo_f2{ehf, ohf}, (fo_f2 *)(lb1 + lo2));
              __builtin_nontemporal_store(fo_f2{erf_, orf}, (fo_f2 *)(lb2 + lo2));
            }
            lo1 += (unsigned)M * LE;
            lo2 += (unsigned)M * (2u * LE);
          };
          int t = g0s;
          // Float32 arithmetic only: runs of rows that take the short way (97 % of the rows of the bench workload, usually the
          // whole chunk) in a loop of their own: per row two scalar shifts, two ands, two compares and two branches less -- 71 ->
          // 53 instructions per row of the two-coefficient models.  Measured per list format, same flags on both sides: float32
          // arithmetic -1.9 % (0.4538 / 0.4564 -> 0.4463 / 0.4456 ms), float64 arithmetic with float32 stores +1.4 %, float64
          // lists +5 % (23 / 48 spilled VGPRs instead of 19 / 17, and those two are not bound by pass 2's issue).
          if constexpr (LISTS == LST_F32) {
            const unsigned fastrows = hvrows & ~slow;
            while (t < g1s) {
              const int row = t - gbase;
              const int run = min(__builtin_ctz(~(fastrows >> row) | 0x80000000u), g1s - t);
              if (run > 0) {
                const int te = t + run;
                for (; t < te; ++t) row_step(t, std::true_type{});
              } else {
                row_step(t, std::false_type{});
                ++t;
              }
            }
          }
          for (; t < g1s; ++t) row_step(t, std::false_type{});
          }
        };
        if constexpr (FIXED) pass2(hm_tag);
        else if (lr4s) pass2(hm_const<HM_LR4S>{});
        else if (dvmax_mode) pass2(hm_const<HM_DVMAX>{});
        else pass2(hm_const<HM_GENERIC>{});
      }
      SW_STAMP(2);
    }
    // (horizon-split form, a wave whose segment lies beyond the horizon: it still takes part in the agent's pool round)
    if (SPLIT && !(seg0 < seg1)) pool_round(0, 0, 0.0, 0);
    if (dvmax_mode) {
      if (nze_min < INFINITY) {   // nze_min = -(largest squared relative speed)
        const double dvm = fo_sqrt(-nze_min);
        max_eh = fo_vmax(max_eh, fo_logistic_neg<false>(exp_tab, fma(hk[0], dvm, hk[2])));
        max_oh = fo_vmax(max_oh, fo_logistic_neg<false>(exp_tab, fma(hk[1], dvm, hk[3])));
      }
    } else
    if (!lst_exact(LISTS) && nze_min < INFINITY) {   // (a wave whose samples carry no harm keeps -inf, as the lists path does)
      max_eh = fo_vmax(max_eh, fo_logistic_neg<false>(exp_tab, nze_min));
      max_oh = fo_vmax(max_oh, fo_logistic_neg<false>(exp_tab, nzo_min));
    }

    if (SPLIT) {
      // ---------------------------------------------------------------- fold the four time segments, in time order
      // (minimum with the earliest t for the DCE, first maximum for the risks and probabilities): each wave parks its
      // values in its own LDS rows, wave 0 folds them and goes on to the outputs alone
      if (wave > 0) {
        double *sp = cpw + lane;
        sp[0 * TILE] = dce; sp[1 * TILE] = (double)tdce; sp[2 * TILE] = max_er; sp[3 * TILE] = max_or;
        sp[4 * TILE] = (double)idx_or; sp[5 * TILE] = max_eh; sp[6 * TILE] = max_oh; sp[7 * TILE] = max_cp;
        sp[8 * TILE] = (double)idx_cp; sp[9 * TILE] = oh_at_cp;
      }
      __syncthreads();
      if (wave == 0)
      for (int w = 1; w < QWAVES; ++w) {
        const double *sp = cpbuf_all + w * (WROWS * TILE) + lane;
        const double d_w = sp[0 * TILE];
        const int t_w = (int)sp[1 * TILE];
        if (d_w < dce || (d_w == dce && t_w < tdce)) { dce = d_w; tdce = t_w; }
        { const double e_ = sp[2 * TILE]; if (e_ > max_er || e_ != e_) max_er = e_; }
        if (sp[3 * TILE] > max_or) { max_or = sp[3 * TILE]; idx_or = (int)sp[4 * TILE]; }
        max_eh = fmax(max_eh, sp[5 * TILE]);
        max_oh = fmax(max_oh, sp[6 * TILE]);
        if (sp[7 * TILE] > max_cp) { max_cp = sp[7 * TILE]; idx_cp = (int)sp[8 * TILE]; oh_at_cp = sp[9 * TILE]; }
      }
      // more agents to come: the other waves' rows are theirs again once wave 0 has read them
      if (kk + 1 < apw_ && k + 1 < A) __syncthreads();
      if (wave > 0) return;
    }
    SW_STAMP(3);
    // ------------------------------------------------------------------ per-pair scalars
    const double dce_m = (dce < INFINITY) ? fo_div1000(dce) : dce;                          // np.round(d, 3)
    const double ttce = fo_round3_fast((double)tdce * a.dt);                                // ttce.py:39
    const double ttc = (dce == 0.0) ? ttce : INFINITY;                                      // ttc.py:43-46
    if (a.be_mask) a.be_mask[(size_t)k * a.Mp + m] = (do_ttc && ttc < INFINITY && ttc > 0.0) ? 1 : 0;  // be.py:49-50
    const bool hr_valid = do_hr && Lh > 0;
    const double hwc = (max_cp > 0.01) ? oh_at_cp : 0.0;                                    // hr.py:81-84
    if (PAIR) {
      const size_t ps_ = (size_t)A * M;
      double *pf = a.pair_f + (size_t)k * M + m;
      pf[FO_PF_DCE * ps_] = do_dce ? dce_m : NAN;
      pf[FO_PF_TTC * ps_] = do_ttc ? ttc : NAN;
      pf[FO_PF_TTCE * ps_] = do_ttce ? ttce : NAN;
      if (hr_valid) {   // (wave-uniform)
        // a collision probability of this pair was NaN (see pass 2): NaN where the probability enters -- the high word alone
        const unsigned long long bad = __builtin_amdgcn_fcmp(max_er, max_er, 8 /* uno */);
        pf[FO_PF_MAX_EGO_RISK * ps_] = max_er;
        pf[FO_PF_MAX_OBST_RISK * ps_] = fo_sel_hi(bad, max_or, NAN);
        pf[FO_PF_HARM_WITH_CP * ps_] = fo_sel_hi(bad, hwc, NAN);
        pf[FO_PF_MAX_EGO_HARM * ps_] = max_eh;
        pf[FO_PF_MAX_OBST_HARM * ps_] = max_oh;
        pf[FO_PF_MAX_CP * ps_] = fo_sel_hi(bad, max_cp, NAN);
      } else {
        pf[FO_PF_MAX_EGO_RISK * ps_] = NAN; pf[FO_PF_MAX_OBST_RISK * ps_] = NAN; pf[FO_PF_HARM_WITH_CP * ps_] = NAN;
        pf[FO_PF_MAX_EGO_HARM * ps_] = NAN; pf[FO_PF_MAX_OBST_HARM * ps_] = NAN; pf[FO_PF_MAX_CP * ps_] = NAN;
      }
      pf[FO_PF_BE_DECEL * ps_] = NAN;
      pf[FO_PF_BE_BTN * ps_] = NAN;
      pf[FO_PF_SPARE * ps_] = NAN;
      int32_t *pi = a.pair_i + (size_t)k * M + m;
      pi[FO_PI_TIME_DCE * ps_] = do_dce ? tdce : 0;
      pi[FO_PI_RISK_INDEX * ps_] = hr_valid ? idx_or : 0;
      pi[FO_PI_CP_ARGMAX * ps_] = hr_valid ? idx_cp : 0;
      pi[FO_PI_HR_VALID * ps_] = hr_valid ? 1 : 0;
    }
    // The running extrema over the wave's agents as v_min / v_max plus ONE select of the index on a scalar-pair mask
    // (a compare followed by three v_cndmask on vcc holds the SIMD for ~25 cycles beyond the instructions' own issue --
    // tools/microbench/valu_rate.hip, "v_cmp_f64 + v_cndmask"; as plain C this epilogue costs the headline kernel +1 %); the
    // bare instruction instead of fmax() with its canonicalising v_max x, x in front (operands are results of arithmetic,
    // never signalling NaNs).
    if (do_dce) {
      const unsigned long long lt = __builtin_amdgcn_fcmp(dce_m, w_min_dce, 4 /* olt */);
      w_min_dce = fo_vmin(w_min_dce, dce_m);
      w_arg_dce = fo_sel_b32(lt, w_arg_dce, k);
      if (dce_m < a.thr_dce) w_dce_flag = true;
      if (do_ttc) {
        const unsigned long long z = __builtin_amdgcn_ballot_w64(dce == 0.0 && tdce < w_min_tttc);
        w_min_tttc = fo_sel_b32(z, w_min_tttc, tdce);
        w_arg_ttc = fo_sel_b32(z, w_arg_ttc, k);
      }
      if (do_ttce) w_min_tttce = min(w_min_tttce, tdce);
    }
    if (hr_valid) {
      w_max_er = fo_vmax(w_max_er, max_er);
      const unsigned long long gt = __builtin_amdgcn_fcmp(max_or, w_max_or, 2 /* ogt */);
      w_max_or = fo_vmax(w_max_or, max_or);
      w_arg_or = fo_sel_b32(gt, w_arg_or, k);
      w_max_eh = fo_vmax(w_max_eh, max_eh);
      w_max_oh = fo_vmax(w_max_oh, max_oh);
      w_max_cp = fo_vmax(w_max_cp, max_cp);
      w_max_hwc = fo_vmax(w_max_hwc, hwc);
    }
    };
    // the one place that asks for the agent's harm model (wave-uniform): LR4S; the two-coefficient models (pedestrian, LR1S:
    // prot == 0) with the usual signs of the speed coefficients; everything else -- agents without a harm model, speed
    // coefficients of unusual sign
    const bool dvmax_ = prot == 0 && C[10] <= 0.0 && C[11] <= 0.0 && !(FO_X & 8);
    if constexpr (SPLIT) agent_body(hm_any{prot == 1 ? HM_LR4S : dvmax_ ? HM_DVMAX : HM_GENERIC});
    else if (prot == 1) agent_body(hm_const<HM_LR4S>{});
    else if (dvmax_) agent_body(hm_const<HM_DVMAX>{});
    else agent_body(hm_const<HM_GENERIC>{});
  }

  // ---------------- combine the waves of the workgroup (ascending agent order); scratch aliases the cp buffers
  // (horizon-split form: wave 0 has folded every agent's segments and holds the workgroup's values -- no exchange, the other
  // waves are done)
  if (SPLIT && wave > 0) return;
  if (!SPLIT) __syncthreads();
  double *red = cpbuf_all;
  double w_min_ttc = w_min_tttc == 0x7fffffff ? INFINITY : fo_round3_fast((double)w_min_tttc * a.dt);
  double w_min_ttce = w_min_tttce == 0x7fffffff ? INFINITY : fo_round3_fast((double)w_min_tttce * a.dt);
  if (!SPLIT && wave > 0) {
    double *rp = red + (size_t)(wave - 1) * NPS * TILE + lane;
    rp[PS_MIN_DCE * TILE] = w_min_dce; rp[PS_ARG_DCE * TILE] = (double)w_arg_dce; rp[PS_MIN_TTC * TILE] = w_min_ttc;
    rp[PS_ARG_TTC * TILE] = (double)w_arg_ttc; rp[PS_MIN_TTCE * TILE] = w_min_ttce; rp[PS_MAX_ER * TILE] = w_max_er;
    rp[PS_MAX_OR * TILE] = w_max_or; rp[PS_ARG_OR * TILE] = (double)w_arg_or; rp[PS_MAX_EH * TILE] = w_max_eh;
    rp[PS_MAX_OH * TILE] = w_max_oh; rp[PS_MAX_CP * TILE] = w_max_cp; rp[PS_MAX_HWC * TILE] = w_max_hwc;
    rp[PS_DCE_FLAG * TILE] = w_dce_flag ? 1.0 : 0.0; rp[PS_MAX_BTN * TILE] = 0.0;
  }
  if (!SPLIT) __syncthreads();
  if (wave == 0) {
    if (!SPLIT)
    for (int w = 0; w < QWAVES - 1; ++w) {
      const double *rp = red + (size_t)w * NPS * TILE + lane;
      // (ties keep the value in hand: wave order = agent order, so that is the smaller agent index)
      const int ad_ = (int)rp[PS_ARG_DCE * TILE], at_ = (int)rp[PS_ARG_TTC * TILE], ao_ = (int)rp[PS_ARG_OR * TILE];
      if (rp[PS_MIN_DCE * TILE] < w_min_dce) { w_min_dce = rp[PS_MIN_DCE * TILE]; w_arg_dce = ad_; }
      if (rp[PS_MIN_TTC * TILE] < w_min_ttc) { w_min_ttc = rp[PS_MIN_TTC * TILE]; w_arg_ttc = at_; }
      w_min_ttce = fmin(w_min_ttce, rp[PS_MIN_TTCE * TILE]);
      w_max_er = fmax(w_max_er, rp[PS_MAX_ER * TILE]);
      if (rp[PS_MAX_OR * TILE] > w_max_or) { w_max_or = rp[PS_MAX_OR * TILE]; w_arg_or = ao_; }
      w_max_eh = fmax(w_max_eh, rp[PS_MAX_EH * TILE]);
      w_max_oh = fmax(w_max_oh, rp[PS_MAX_OH * TILE]);
      w_max_cp = fmax(w_max_cp, rp[PS_MAX_CP * TILE]);
      w_max_hwc = fmax(w_max_hwc, rp[PS_MAX_HWC * TILE]);
      w_dce_flag = w_dce_flag || rp[PS_DCE_FLAG * TILE] > 0.0;
    }
    const size_t PM = (size_t)a.Mp;
    double *pp = a.partial + (size_t)chunk * NPS * PM + (size_t)tile * TILE + lane;
    pp[PS_MIN_DCE * PM] = w_min_dce; pp[PS_ARG_DCE * PM] = (double)w_arg_dce; pp[PS_MIN_TTC * PM] = w_min_ttc;
    pp[PS_ARG_TTC * PM] = (double)w_arg_ttc; pp[PS_MIN_TTCE * PM] = w_min_ttce; pp[PS_MAX_ER * PM] = w_max_er;
    pp[PS_MAX_OR * PM] = w_max_or; pp[PS_ARG_OR * PM] = (double)w_arg_or; pp[PS_MAX_EH * PM] = w_max_eh;
    pp[PS_MAX_OH * PM] = w_max_oh; pp[PS_MAX_CP * PM] = w_max_cp; pp[PS_MAX_HWC * PM] = w_max_hwc;
    pp[PS_DCE_FLAG * PM] = w_dce_flag ? 1.0 : 0.0; pp[PS_MAX_BTN * PM] = 0.0;
  }
}

// Every output mode runs in one shape: chunks of FO_TC = 8 samples, FO_MINW = 3 waves per SIMD (the hot loops of the modes
// with per-sample lists need 164 VGPRs).  The four-wave shape -- chunks of four, 128 VGPRs, 37 KB of LDS -- was faster for
// the modes without lists until the scalar-instruction diet of round 3; since then it loses everywhere: reduced outputs 0.438
// against 0.417 ms, float32 lists 0.604 against 0.590, float64 lists 0.701-0.716 against 0.685.
template <bool PAIR, int LISTS, bool ALLM, bool SPLIT = false>
__global__ __launch_bounds__(TILE *QWAVES) __attribute__((amdgpu_waves_per_eu(FO_MINW, FO_MINW)))
void fo_sweep_queue_kernel(const SweepArgs a) {
  __shared__ double2 erf_tab[ERF_N];
  __shared__ double exp_tab[EXP_N];
  __shared__ double zc_tab[4];                      // LR4S logistic offsets by impact class: front, side, rear
  __shared__ double hk_all[QWAVES * 4];             // per wave: the current agent's logistic slopes and offsets
  constexpr int BUFROWS = QWAVES * WROWS > (QWAVES - 1) * NPS ? QWAVES * WROWS : (QWAVES - 1) * NPS;
  __shared__ double cpbuf_all[BUFROWS * TILE];  // per wave: TC rows of collision probabilities, DVR rows of
                                                       // relative speeds; also the cross-wave reduction scratch
  __shared__ unsigned short queue_all[QWAVES * (SPLIT ? TILE * TC : QCAP)];   // per wave: in-gate samples (lane | row << 6)
  __shared__ int pool_i[3 * QWAVES];       // pool_round, per wave: queue length, agent, gate sample of buffer row 0
  __shared__ double pool_hd[QWAVES];       //             half the agent's inflated length
  {
    // The two tables into LDS.  All of a thread's loads are issued before the first store (written as a loop the copy
    // compiles to five dependent round trips: load, wait, store, ...).  (A build WITHOUT the copy is no measure of its
    // cost: the compiler then knows the tables are never written and deletes the code that reads them.)
    static_assert(TILE * QWAVES == 256 && EXP_N == 256 && ERF_N > 768 && ERF_N <= 1024, "table copy written for 256 threads");
    const int tt = threadIdx.x;
    const double2 v0 = a.erf_tab[tt], v1 = a.erf_tab[tt + 256], v2 = a.erf_tab[tt + 512];
    const double2 v3 = a.erf_tab[min(tt + 768, ERF_N - 1)];
    const double x0 = a.exp_tab[tt];
    // (g / 128: fo_erf_fast128 measures the offset from a node in table steps)
    erf_tab[tt] = make_double2(v0.x, v0.y * 0x1p-7); erf_tab[tt + 256] = make_double2(v1.x, v1.y * 0x1p-7);
    erf_tab[tt + 512] = make_double2(v2.x, v2.y * 0x1p-7);
    if (tt + 768 < ERF_N) erf_tab[tt + 768] = make_double2(v3.x, v3.y * 0x1p-7);
    exp_tab[tt] = x0;
  }
  if (threadIdx.x < 4)
    zc_tab[threadIdx.x] = -a.hc.lr4s_const - (threadIdx.x == 0 ? 0.0 : threadIdx.x == 1 ? a.hc.lr4s_side : a.hc.lr4s_rear);
  const bool corr = a.status[1] == a.gen;   // scalar load; written by fo_prep_agents_kernel on this stream
#if FO_TRACE
  if (a.trace && threadIdx.x == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    a.trace[4 * (size_t)blockIdx.x + 0] = wall_clock64();
    a.trace[4 * (size_t)blockIdx.x + 2] = (long long)hw | ((long long)xcc << 32);
  }
#endif
  __syncthreads();
#if FO_TRACE
  if (a.trace && threadIdx.x == 0) a.trace[4 * (size_t)blockIdx.x + 3] = wall_clock64();   // tables in LDS
#endif
  if (__builtin_expect(!corr, 1))
    fo_sweep_queue_body<PAIR, LISTS, ALLM, SPLIT, false>(a, erf_tab, exp_tab, zc_tab, hk_all, cpbuf_all, queue_all, pool_i, pool_hd);
  else
    fo_sweep_queue_body<PAIR, LISTS, ALLM, SPLIT, true>(a, erf_tab, exp_tab, zc_tab, hk_all, cpbuf_all, queue_all, pool_i, pool_hd);
#if FO_TRACE
  if (a.trace && threadIdx.x == 0) a.trace[4 * (size_t)blockIdx.x + 1] = wall_clock64();
#endif
}

}  // namespace
