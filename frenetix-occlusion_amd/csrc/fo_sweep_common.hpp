// fo_sweep_common.hpp -- what both sweep kernels share: the compile-time switches of the device code, table sizes and
// partial-reduction slots, the Gauss-Legendre constants, the erf / exp table kernels and look-ups, square roots, select and
// pack helpers, the 1e-3 rounding, the CP gate's distance, the list stores, the LST_* output modes and SweepArgs.
// A part of the fo_sweep.hip translation unit, not a header to include on its own: it relies on what fo_sweep.hip has
// included before it (HIP, fo_ctx.hpp, fo_agent_rows.hpp, fo_prep_traj.hpp, fo_sweep_plan.hpp).
#pragma once

// (FO_TC and FO_QWAVES: fo_sweep_plan.hpp -- they move the launch plan as well)
#ifndef FO_MINW
#define FO_MINW 3    // waves per SIMD the register allocation has to allow (<= 168 VGPRs)
#endif
#ifndef FO_TRACE
#define FO_TRACE 0
#endif
#ifndef FO_X
#define FO_X 0       // timing experiments only (-DFO_X=8: pass 2 without its arithmetic -- WRONG results).  The last bit of a family
#endif               // of such switches: with its three tests folded away the product's device code changes, so it stays

namespace {

static_assert(TILE == FO_PREP_TILE, "fo_prep_traj.hpp");
constexpr int NEF = 8;     // ego fields per (t, trajectory): x, y, cos, sin, theta, v, v cos, v sin -- stored as four
                           // pairs per trajectory, [t][pair][trajectory][2]: one 16-byte load per lane fetches two
                           // fields (a vector-memory instruction costs the CU ~10 cycles whatever its width)
// Gauss-Legendre rules of the correlation integral (fo_corr_term): node counts by the largest |rho| they serve, and where
// each rule starts in the table ([t, w] pairs, t = (x + 1)/2, w = weight/(4 pi); host, fo_sweep_init_)
constexpr int GL_NR = 5;
__host__ __device__ constexpr int gl_nodes(int r) { return r == 0 ? 6 : r == 1 ? 8 : r == 2 ? 12 : r == 3 ? 20 : 24; }
__host__ __device__ constexpr int gl_first(int r) { return r == 0 ? 0 : r == 1 ? 6 : r == 2 ? 14 : r == 3 ? 26 : 46; }
constexpr int GL_TOTAL = 70;
// rule r serves asin|rho| up to GL_ASR[r] = asin(0.5, 0.7, 0.9, 0.97); the last rule the rest, |rho| <= 0.99
constexpr double GL_ASR0 = 0.5235987755982989, GL_ASR1 = 0.775397496610753, GL_ASR2 = 1.1197695149986342,
                 GL_ASR3 = 1.3252308092796046;
typedef const double __attribute__((address_space(4))) *cdp_gl_t;
                           // (96-byte rows: the 32-byte and 16-byte groups the scalar loads fetch stay naturally aligned)
// NAF = 12 agent fields per (k, t): px, py, cos, sin, yaw, v, 1/(sx*sqrt2), 1/(sy*sqrt2), v cos, v sin, rho, asin rho
// NAC = 16 per-agent constants: hl_raw, hw_raw, half_len_infl, f_ego, f_obs, prot, len, type, sum of the circumradii,
// far-gate radius^2, logistic slopes (ego, obstacle) and offsets, coarse gate radius, longest step (tagged) -- fo_agent_rows.hpp
constexpr int NPS = 14;    // partial-reduction slots
enum { PS_MIN_DCE = 0, PS_ARG_DCE, PS_MIN_TTC, PS_ARG_TTC, PS_MIN_TTCE, PS_MAX_ER, PS_MAX_OR, PS_ARG_OR, PS_MAX_EH,
       PS_MAX_OH, PS_MAX_CP, PS_MAX_HWC, PS_DCE_FLAG, PS_MAX_BTN };

// erf by table + 5th-order Taylor step.  Nodes x0 = i/128, i = 0..768 (|u| < 6; erf(6) == 1 in float64); each entry
// holds erf(x0) and g(x0) = 2/sqrt(pi) exp(-x0^2).  |delta| <= 1/256, remainder f^(6)/720 * delta^6 < 3e-16:
// the same absolute accuracy as libm erf/erfc for the box probabilities, at ~25 VALU ops + one 16-byte LDS gather
// instead of ~300 for the branchy ocml erfc (which dominated the first version of this kernel, profiles/r01_a_*).
constexpr int ERF_N = 769;
constexpr double ERF_SCALE = 128.0;

__global__ void fo_erf_table_kernel(double2 *tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ERF_N) return;
  const double x0 = (double)i / ERF_SCALE;
  tab[i] = make_double2(erf(x0), 1.1283791670955125738961589031 * exp(-x0 * x0));
}

// The queue kernel's erf: same nodes, fewer VALU operations.  Its copy of the table in LDS holds (erf(x0), g(x0)/128) and the
// caller hands over the argument already multiplied by 128 (folded into 1/(sigma sqrt 2), once per sample): the node index is
// the low word of |v| + 1.5 * 2^52 (no rint / convert instruction), d = |v| - node is the offset in table steps, and the
// Taylor step is evaluated in y = x0 d_true (= node * d * 2^-14) and s = d^2:
//   erf(x0 + d_true) = e + g d_true P,   P = (1 - s/3) + y (-1 + 2 y/3) + [y s/2 - y^3/3] + [s^2/10 - 2 s y^2/5 + 2 y^4/15] + ...
//   evaluated as  P = a0 + y (-1 + 2 y / 3),  a0 = 1 - s/3.
// The bracket is never evaluated: it contributes g(x0) d^5 (1/10 - 2 x0^2/5 + 2 x0^4/15) <= 1.13 * 0.1 * 256^-5 = 1.0e-13.
// The two cubic terms  y s/2 - y^3/3 = d^3 x0 (1/2 - x0^2/3)  are left out as well:  what is dropped is
// g(x0) d^4 x0 (1/2 - x0^2/3), at most 0.18 * 256^-4 = 4.3e-11 per erf (at x0 = 0.6, |d| = 1/256; a fifth of that on average
// over d), i.e. <= 2.6e-10 on a collision probability (nine products of two differences of erf, / 12; measured on the bench
// batch against the oracle: see parity.float_max_abs_err of the bench line) -- a quarter of the 1e-9 every float output of
// this library is tested to, four orders inside the 1e-5 the task allows, and far below what the float32 list storage keeps.
// The price of the two terms is three instructions per erf, and the 36 erf of an in-gate sample are the one part of the
// sweep kernel whose instructions count three times (the waves that hold the few agents next to the candidates' path carry
// all of it, and their workgroups wait for them): 19 -> 16 -> 14 operations per erf took 6.5 % off the kernel (round 5).
// The polynomial is grouped so that every fma has at most ONE constant that is not an inline operand (1.0, 2.0): a
// VOP3 instruction of this chip reads one literal / SGPR pair, and a second constant costs two v_mov_b32 per erf to park it.
// (Round 5, measured and dropped: the scale of y folded into the two constants of the inner fma, both parked in vector
// registers by the caller -- one multiplication less per erf -- 0.529 ms against 0.515: four registers more across the box
// loops of a kernel that sits at its register cap cost thirteen more spilled ones.)
__device__ __forceinline__ double fo_erf_fast128(const double2 *__restrict__ tab, double v) {
  constexpr double S = 0x1p-14;
  const double av = fmin(fabs(v), 768.0);
  const double MAGIC = 6755399441055744.0;  // 1.5 * 2^52
  const double tm = av + MAGIC;
  const double fi = tm - MAGIC;               // rint(|v|), exact
  const int i = __double2loint(tm);
  const double d = av - fi;
  const double2 e = tab[i];
  const double sq = d * d;
  const double a0 = fma(sq, -S / 3.0, 1.0);
  const double y = fi * (d * S);
  const double p = fma(fma(y, 2.0 / 3.0, -1.0), y, a0);
  return copysign(fma(e.y * d, p, e.x), v);
}

// offset of ego field f from a row pointer that already points at the lane's first pair (row base + 2 lane)
#define EF(f) ((((f) >> 1) * 2 * TILE) + ((f) & 1))
typedef double fo_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ fo_d2 fo_ld2(const double *p) { return *(const fo_d2 *)p; }

constexpr int EXP_N = 256;
__global__ void fo_exp_table_kernel(double *tab) {
  if (threadIdx.x < EXP_N) tab[threadIdx.x] = exp2((double)threadIdx.x / (double)EXP_N);
}

__device__ __forceinline__ double fo_erf_lds(const double2 *__restrict__ tab, double u) {
  const double au = fmin(fabs(u), 6.0);
  const double fi = __builtin_rint(au * ERF_SCALE);
  const double x0 = fi * (1.0 / ERF_SCALE);
  const double d = au - x0;
  const double2 e = tab[(int)fi];
  const double q = x0 * x0;
  const double a2 = (2.0 * q - 1.0) * (1.0 / 3.0);
  const double a3 = -x0 * (2.0 * q - 3.0) * (1.0 / 6.0);
  const double a4 = (4.0 * q * q - 12.0 * q + 3.0) * (1.0 / 30.0);
  const double p = 1.0 + d * (-x0 + d * (a2 + d * (a3 + d * a4)));
  return copysign(e.x + e.y * d * p, u);
}

// sqrt by one Goldschmidt step on v_rsq_f64 (relative error ~1e-14 instead of the correctly rounded ~25-instruction
// expansion of sqrt()); x >= 0, x = 0 -> 0.  Consumers are compared at 1e-9; the distances rounded to 1e-3 take one more
// correction (fo_mm).
__device__ __forceinline__ double fo_sqrt(double x) {
  // x = 0: rsq gives +inf, the Goldschmidt step NaN, and v_max_f64(NaN, 0) = 0 -- a guard that needs no float64 literal
  // (1e-300 costs two s_mov per use: a scalar instruction is as dear to its wave as a vector one)
  const double g = __builtin_amdgcn_rsq(x);
  double y = x * g;
  const double h = 0.5 * g;
  const double r = fma(-h, y, 0.5);
  y = fma(y, r, y);
  double z;
  asm("v_max_f64 %0, %1, 0" : "=v"(z) : "v"(y));
  return z;
}
// Round 5: the same for x > 0 -- the squared relative speeds of the ring, which pass 1 writes with the smallest denormal added
// (fo_sq_sum_pos: an inline integer constant 1 in a float64 operand IS that number, no literal, no extra instruction), so that
// the guard of fo_sqrt is not needed where pass 2 takes the root: one instruction per list entry.
__device__ __forceinline__ double fo_sqrt_pos(double x) {
  const double g = __builtin_amdgcn_rsq(x);
  const double y = x * g;
  const double h = 0.5 * g;
  const double r = fma(-h, y, 0.5);
  return fma(y, r, y);
}
__device__ __forceinline__ double fo_sq_sum_pos(double a, double b) {   // a^2 + b^2 (+ 4.9e-324)
  double t;
  asm("v_fma_f64 %0, %1, %1, 1" : "=v"(t) : "v"(b));
  return fma(a, a, t);
}
// value with its three lowest mantissa bits replaced by u (0..7)
__device__ __forceinline__ double fo_pack_low(double v, int u) {
  const unsigned lo = ((unsigned)__double2loint(v) & ~7u) | (unsigned)u;   // (v_and_or_b32 with two inline constants)
  return __hiloint2double(__double2hiint(v), (int)lo);
}
// lanes of `mask`: b, the others a -- v_cndmask_b32 with the mask in a scalar pair (not vcc)
__device__ __forceinline__ int fo_sel_b32(unsigned long long mask, int a, int b) {
  int r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
  return r;
}
// the same for a float64 whose LOW word may stay (b = NaN or +-inf or 1.0 over a value with a zero low word, or a NaN over
// anything: a NaN is a NaN whatever its payload) -- one v_cndmask_b32 on the high word
__device__ __forceinline__ double fo_sel_hi(unsigned long long mask, double a, double b) {
  return __hiloint2double(fo_sel_b32(mask, __double2hiint(a), __double2hiint(b)), __double2loint(a));
}
// a * b + c with three distinct register operands (the compiler prefers v_mov_b64 + v_fmac_f64 when c outlives the result)
__device__ __forceinline__ double fo_fma3(double a, double b, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ __forceinline__ double fo_round3(double v) { return __builtin_rint(v * 1000.0) / 1000.0; }  // np.round(v,3)
// Squared distance of the CP gate (collision_probability.py:49-67,75): the nearest of the three means mean + j dev,
// j = 0, +1, -1, to the ego sample, in the reference's order -- the mean is displaced first, then the ego is subtracted,
// each square is rounded on its own, then the two are added.  No contraction: a fused x^2 + y^2, or the displacement
// added to (ego - mean) instead of to the mean, decides a few per cent of the samples within a few ulps of the 5 m
// circle differently from the reference (tests/test_cp_gate_cpu.py), and each of those turns a CP of 1e-2 into 0.
__device__ __forceinline__ double fo_gate_d2(double mx, double my, double devx, double devy, double ex, double ey) {
#pragma clang fp contract(off)
  const double cx = mx - ex, cy = my - ey;
  const double fx = (mx + devx) - ex, fy = (my + devy) - ey;
  const double bx = (mx - devx) - ex, by = (my - devy) - ey;
  return fmin(cx * cx + cy * cy, fmin(fx * fx + fy * fy, bx * bx + by * by));
}
// r / 1000.0, correctly rounded, for finite r: q = r RN(1/1000), one fma for the exact remainder, one for the correction
// (three operations instead of the ~30 of a float64 division; checked against true division for every integer below 2e7)
__device__ __forceinline__ double fo_div1000(double r) {
  const double q = r * 0.001;
  return fma(fma(-q, 1000.0, r), 0.001, q);
}
__device__ __forceinline__ double fo_round3_fast(double v) { return fo_div1000(__builtin_rint(v * 1000.0)); }

// The five per-timestep lists of hr.py:87-98 for sample index i = (k (T-1) + t) M + m, n = A (T-1) M entries per list
// (layout of include/fo_hip.h): cp alone, the two harms and the two risks as interleaved pairs -- a lane writes 8 + 16 +
// 16 bytes with three store instructions, each covering one contiguous run of the wave (512 B / 1 KB / 1 KB).
template <bool NT = true>
__device__ __forceinline__ void fo_store_lists(double *lists, size_t n, size_t i, double cp, double eh, double oh,
                                               double er, double orr) {
  fo_d2 *h = (fo_d2 *)(lists + n) + i, *r = (fo_d2 *)(lists + 3 * n) + i;
  if (NT) {
    __builtin_nontemporal_store(cp, lists + i);
    __builtin_nontemporal_store(fo_d2{eh, oh}, h);
    __builtin_nontemporal_store(fo_d2{er, orr}, r);
  } else {
    lists[i] = cp;
    *h = fo_d2{eh, oh};
    *r = fo_d2{er, orr};
  }
}

// The same three blocks with float32 elements (fo_sweep_set_list_format(FO_LISTS_F32): the storage SURVEY 8d prices,
// 648 B per pair): cp float [n], (ego harm, obstacle harm) float2 [n], (ego risk, obstacle risk) float2 [n] -- a lane
// writes 4 + 8 + 8 bytes, each store one contiguous run of the wave (256 B / 512 B / 512 B).
typedef float fo_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void fo_store_lists_f32(float *lists, size_t n, size_t i, float cp, float eh, float oh, float er,
                                                   float orr) {
  __builtin_nontemporal_store(cp, lists + i);
  __builtin_nontemporal_store(fo_f2{eh, oh}, (fo_f2 *)(lists + n) + i);
  __builtin_nontemporal_store(fo_f2{er, orr}, (fo_f2 *)(lists + 3 * n) + i);
}
// 1 / (1 + exp(nz)) in float32 on the hardware transcendentals (v_exp_f32, v_rcp_f32: 8 cycles each against ~70 for the
// float64 table route): for the float32 list entries only -- every maximum, risk and cost entry stays float64.  |error|
// < 4e-7 absolute (argument rounding 6e-8 |nz| times the slope <= 1/4, one ulp each for exp2 and rcp).
__device__ __forceinline__ float fo_logistic_neg_f32(double nz) {
  const float e = __builtin_amdgcn_exp2f((float)nz * 1.44269504f);   // +inf for large nz -> rcp gives 0; 0 for very negative nz -> 1
  return __builtin_amdgcn_rcpf(1.0f + e);
}

// ------------------------------------------------------------------------------------------------ the sweep
enum { LST_NONE = 0, LST_F64 = 1, LST_F32 = 2, LST_F32X = 3 };   // per-timestep list output of a sweep instantiation
// LST_F32X (FO_LISTS_F32_EXACT): float32 elements like LST_F32, but every entry is the float64 result rounded at the store --
// the arithmetic of LST_F64, the bytes of LST_F32; what the float32 shortcut of LST_F32 saves is the difference of the two
__host__ __device__ constexpr bool lst_is32(int l) { return l == LST_F32 || l == LST_F32X; }
// (Round 5, measured and dropped for FO_LISTS_F32_EXACT, all within +-0.5 % of this form: the shape of the float32-list
// instantiation -- running minima of the logistic arguments, harm maxima from the epilogue -- with float64 list entries from a
// table exponential of degree 2 on the rows without a gate lane; both logistic values of a sample through one reciprocal; the
// square root of sample t+1 taken beside the exponentials of sample t.  The instantiation stays pass 2 of the float64 lists
// with conversions at the store: every entry is the float64-list mode's entry, rounded.)
__host__ __device__ constexpr bool lst_exact(int l) { return l == LST_F64 || l == LST_F32X; }
struct SweepArgs {
  int M, Mp, T, A, Ta, n_tiles, nt8, apw;  // apw = agents per wave
  const double *traj;    // [n_tiles][T][NEF][64]
  const double *atab;    // [A][Ta][NAF]
  const double *acst;    // [A][NAC]
  const double2 *erf_tab;  // [ERF_N]
  const double *exp_tab;   // [EXP_N]  2^(j/EXP_N)
  const double *gl;        // [GL_TOTAL][2] Gauss-Legendre nodes and weights (correlated covariances)
  const int *status;       // [3] generation tags of fo_prep_agents_kernel: [0] unusable covariance, [1] correlated one, [2] refused rule list
  int gen;                 // generation of the current agent set
  const int32_t *aint;     // [A][2] protection class, valid length
  double *partial;       // [n_chunks][NPS][Mp]
  double *pair_f;        // [NPF][A][M] or null
  int32_t *pair_i;       // [NPI][A][M] or null
  double *lists;         // [NL][A][T-1][M] or null
  signed char *be_mask;  // [A][Mp] 1 where the pair collides at ttc > 0 (only with FO_M_BE), else null
  double hlA, hwA, wb, len3, off_x, off_y;  // ego half dims, rear-axle offset, L/3, L/6, W/2
  fo_harm_coeff_t hc;
  double dt, thr_dce;
  uint32_t mask;
  uint32_t ablate;  // debug only (env FO_SWEEP_ABLATE): 1 skip DCE, 2 skip CP box sums, 4 skip harm -- wrong results, timing aid
  // Tapered grid: the chunks of a tile shrink towards the end of the launch (workgroups are dispatched in blockIdx order,
  // chunk-major): ph_n[0] chunks of 4 x ph_a[0] agents, then ph_n[1] of 4 x ph_a[1], ..., the rest of 4 x ph_a[3].
  // A workgroup lives ~40 us per agent of its waves; at the end of a launch the chip drains for about half a workgroup
  // life (tools/wg_trace.py: with 16 agents per workgroup throughout, the last fifth of the launch runs half empty) --
  // short workgroups there cut the drain, long ones before keep the per-workgroup start-up (table fill, cross-wave
  // fold) off most of the work.
  // The decode sits in a table, [chunk] -> (first agent of wave 0, agents per wave), which fo_prep_traj_kernel writes
  // before every sweep: two scalar loads here (a decode loop over the phases in this kernel tipped its register
  // allocation over: SGPR spills through scratch memory, twice the run time).
  const int *chunk_tab;
#if FO_TRACE
  long long *trace;  // tuning builds (-DFO_TRACE=1): per workgroup start / end wall clock (100 MHz) + hardware id
#endif
};

}  // namespace
