// fo_sweep_generic.hpp -- the prep kernels (tile table, agent rows) and the generic sweep kernel with its helpers: the
// straightforward form every batch shape can take, and the statement of the arithmetic the queue kernel restructures.
// A part of the fo_sweep.hip translation unit, included after fo_sweep_common.hpp; not a header to include on its own.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------ prep kernels
// trajectories [M][T] (row per trajectory) -> tile table [tile][T][NEF][64], transposed through LDS so that both the
// HBM read (along T) and the HBM write (along trajectories) are contiguous; sincos(theta) is taken once here.
// Within a tile every (t, field) row is 512 contiguous bytes = one wave-wide load, and field / timestep strides
// are compile-time constants (immediate offsets in the sweep's loads).
__global__ __launch_bounds__(256) void fo_prep_traj_kernel(const fo_prep_args_t p) {
  extern __shared__ double sh[];  // [2][tz][TILE+1]
  fo_prep_traj_block(p, blockIdx.x, blockIdx.y, blockIdx.z, sh);   // fo_prep_traj.hpp
}

// agent predictions -> [A][Ta][NAF] table + [A][NAC] constants (one thread per (k, t); fo_agent_rows.hpp)
__global__ void fo_prep_agents_kernel(int A, int Ta, const double *__restrict__ pos, const double *__restrict__ yaw,
                                      const double *__restrict__ v, const double *__restrict__ cov,
                                      const double *__restrict__ shape, const double *__restrict__ raw,
                                      const int32_t *__restrict__ type, const int32_t *__restrict__ len,
                                      double ego_mass, double hlA, double hwA, fo_harm_coeff_t hc,
                                      double *__restrict__ tab, double *__restrict__ cst,
                                      int32_t *__restrict__ aint, int *__restrict__ status, int gen) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A * Ta) return;
  fo_agent_row(i, Ta, pos, yaw, v, cov, shape, raw, type, len, ego_mass, hlA, hwA, hc, tab, cst, aint, status, gen);
}

__device__ __forceinline__ double fo_lr4s_coef(double ang, double side, double rear) {
  const double t_a = 45.0 / 180.0 * M_PI, t_b = 3.0 * t_a;  // logistic_regression.py:28-29
  if (-t_a < ang && ang < t_a) return 0.0;
  if (t_a <= ang && ang < t_b) return side;
  if (-t_a >= ang && ang > -t_b) return side;
  return rear;  // un-wrapped angle: everything else is "rear" (Q5)
}

// LR4S angle classes without atan2 (queue kernel).  The reference bins the UN-wrapped angle ang = rel - heading,
// rel = atan2(dy, dx) in (-pi, pi]  (logistic_regression.py:28-42, Q5): front |ang| < pi/4, side pi/4 <= |ang| < 3pi/4,
// rear otherwise.  Write ang = phi + 2 pi k with phi the wrapped angle: k != 0 implies |ang| >= pi, i.e. rear, and for
// k == 0 the class of phi follows exactly from the signs of  S = d x h  and  C = d . h  (h = unit heading):
// front  C > |S|,  rear  -C >= |S|,  side otherwise.  k != 0 <=> |rel - heading| > pi only has to be decided when phi is
// not rear, where |rel - heading| is either < 3pi/4 or > 5pi/4 -- a float32 atan2 estimate (error < 0.01) is enough.
__device__ __forceinline__ float fo_atan2_crude(float y, float x) {
  // The "diamond angle" -- pi/2 (1 - x / (|x| + |y|)) with the sign of y: monotonic in the true angle, exact on the
  // axes and the diagonals, 0.071 rad off at worst (the decision it feeds has pi/4 of room, see above).  No comparison, no
  // select: the three v_cmp + v_cndmask pairs of an octant form each hold the SIMD for ten cycles beyond their own issue.
  // (x = y = 0 does not get here: the caller puts dx = 1 for coincident centres.  Offsets that are nonzero in float64 but vanish
  // -- or overflow, or are denormal -- as float32 give 0 * inf = NaN or +-inf here, never a value in [-pi, pi]: the callers hand
  // such a sample to the reference's own float64 route, see the test |estimate| <= 4 in pass 1.)
  const float q = x * __builtin_amdgcn_rcpf(fabsf(x) + fabsf(y));
  return copysignf(fmaf(q, -1.57079633f, 1.57079633f), y);
}

// coefficient of the class: 0 (front), side, rear.  (dx, dy): from the vehicle whose occupants are rated to the other
// party, as seen by atan2; `turn` = what is added to rel before the heading is subtracted (0 for the ego, pi for the
// obstacle: obs_ang = pi + rel - yaw, harm_model.py:89-90).
__device__ __forceinline__ double fo_lr4s_coef_dir(double dx, double dy, double hc, double hs, float rel_crude, float turn,
                                                   double heading, double side, double rear) {
  const double sg = (turn != 0.0f) ? -1.0 : 1.0;  // direction of angle rel + turn
  const double S = sg * (dy * hc - dx * hs), Cc = sg * (dx * hc + dy * hs);
  const double aS = fabs(S);
  const bool unwrapped_far = fabsf(turn + rel_crude - (float)heading) > 3.14159265f;
  if (unwrapped_far || -Cc >= aS) return rear;
  if (Cc > aS) return 0.0;
  return side;
}

// the same decision as an index (0 front, 1 side, 2 rear) -- the queue kernel takes it in pass 1, where the poses are
// in registers anyway, and keeps two bits per sample until pass 2 looks the logistic offset up.  flip = obstacle side
// (angle rel + pi: both S and C change sign).
// `band` is raised where the sample may sit on a class boundary to within rounding (|C| = |S| up to 1e-13 relative): there
// the reference's own floating-point route -- atan2, the subtraction, the comparison with 45/180 pi -- decides, and may
// decide either way (a heading of exactly -pi/4 with the other party exactly on the x axis gives ang == t_a: "side",
// although cos of that heading is one ulp above |sin|); the caller re-rates those samples with fo_lr4s_class_ref.
__device__ __forceinline__ unsigned fo_lr4s_class(double dx, double dy, double hc, double hs, float rel_crude, float turn,
                                                  float heading, bool flip, bool &band) {
  double S = dy * hc - dx * hs, Cc = dx * hc + dy * hs;
  if (flip) Cc = -Cc;  // |S| is all that is used of S
  const double aS = fabs(S), aC = fabs(Cc);
  // coarse and cheap here (high words within one of each other: |C| = |S| to ~1e-6); the exact 1e-13 test is taken
  // by fo_lr4s_on_boundary where the flagged samples are re-rated
  band = (unsigned)(__double2hiint(aC) - __double2hiint(aS) + 1) <= 2u;
  const bool unwrapped_far = fabsf(turn + rel_crude - heading) > 3.14159265f;
  unsigned c = (Cc > aS) ? 0u : 1u;
  if (unwrapped_far || -Cc >= aS) c = 2u;
  return c;
}
__device__ __forceinline__ bool fo_lr4s_on_boundary(double dx, double dy, double hc, double hs) {
  const double aS = fabs(dy * hc - dx * hs), aC = fabs(dx * hc + dy * hs);
  return fabs(aC - aS) <= 1e-13 * (aC + aS);
}
// the reference's binning of the un-wrapped angle itself (logistic_regression.py:28-42) as a class index
__device__ __forceinline__ unsigned fo_lr4s_class_ref(double ang) {
  const double t_a = 45.0 / 180.0 * M_PI, t_b = 3.0 * t_a;
  if (-t_a < ang && ang < t_a) return 0u;
  if ((t_a <= ang && ang < t_b) || (-t_a >= ang && ang > -t_b)) return 1u;
  return 2u;
}
// both classes of one sample by the reference's route (harm_model.py:86-90): ego class | obstacle class << 2.  A real
// call on purpose: inlined, the float64 atan2 raises the register demand of the whole kernel (measured +7 % / +34 %).
__device__ __attribute__((noinline)) unsigned fo_lr4s_classes_ref(double ddx, double ddy, double theta, double yaw) {
  const double rel = atan2(ddy, ddx);
  return fo_lr4s_class_ref(rel - theta) | (fo_lr4s_class_ref(M_PI + rel - yaw) << 2);
}

// squared distance from point (px,py) to the axis-aligned box [-hl,hl]x[-hw,hw]
__device__ __forceinline__ double fo_pt_box2(double px, double py, double hl, double hw) {
  const double qx = fmax(fabs(px) - hl, 0.0), qy = fmax(fabs(py) - hw, 0.0);
  return qx * qx + qy * qy;
}

// 1-D normal box probability  P(lo <= X <= hi)  with arguments already divided by sigma*sqrt(2)
__device__ __forceinline__ double fo_phi_diff(const double2 *__restrict__ tab, double lo, double hi) {
  return 0.5 * (fo_erf_lds(tab, hi) - fo_erf_lds(tab, lo));
}

// the correlation integral of one box (see fo_corr_corners) for the generic kernel: libm, always the 24-node rule
__device__ __forceinline__ double fo_corr_term_plain(const double *__restrict__ gl, double A, double B, double Cc, double D,
                                                     double asr) {
  gl += 2 * gl_first(GL_NR - 1);
  double acc = 0.0;
#pragma unroll 1
  for (int i = 0; i < gl_nodes(GL_NR - 1); ++i) {
    const double sn = sin(asr * gl[2 * i]), c2 = 1.0 / (1.0 - sn * sn);
    const double f = exp(-c2 * (A * A + Cc * Cc - 2.0 * sn * A * Cc)) - exp(-c2 * (B * B + Cc * Cc - 2.0 * sn * B * Cc)) -
                     exp(-c2 * (A * A + D * D - 2.0 * sn * A * D)) + exp(-c2 * (B * B + D * D - 2.0 * sn * B * D));
    acc = fma(gl[2 * i + 1], f, acc);
  }
  return acc * asr;
}

template <bool PAIR, int LISTS>
__global__ __launch_bounds__(TILE *WAVES) void fo_sweep_generic_kernel(const SweepArgs a) {
  __shared__ double red[(WAVES - 1) * NPS * TILE];
  __shared__ double2 erf_tab[ERF_N];
  for (int i = threadIdx.x; i < ERF_N; i += TILE * WAVES) erf_tab[i] = a.erf_tab[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware decode: blocks b and b+8 share an XCD (and its L2); keep every chunk of one tile on one XCD
  const int r = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int tile = (j % a.nt8) * 8 + r;
  const int chunk = j / a.nt8;
  if (tile >= a.n_tiles) return;
  const int m = tile * TILE + lane;
  const bool valid = m < a.M;
  const int T = a.T, Tm1 = a.T - 1, M = a.M, A = a.A;
  const size_t Mp = TILE;  // field stride inside a tile
  const double *tj = a.traj + (size_t)tile * T * NEF * TILE + 2 * lane;
  const bool do_dce = a.mask & FO_M_DCE, do_cp = a.mask & FO_M_CP, do_hr = a.mask & FO_M_HR;
  const bool do_ttc = a.mask & FO_M_TTC, do_ttce = a.mask & FO_M_TTCE;

  // reductions over this wave's agents (metric.py / hr.py "all" values)
  double w_min_dce = INFINITY, w_min_ttc = INFINITY, w_min_ttce = INFINITY;
  double w_max_er = 0.0, w_max_or = 0.0, w_max_eh = 0.0, w_max_oh = 0.0, w_max_cp = 0.0, w_max_hwc = 0.0;
  double w_arg_dce = -1.0, w_arg_ttc = -1.0, w_arg_or = -1.0, w_dce_flag = 0.0;

  const int k0 = (chunk * WAVES + wave) * a.apw;
  for (int kk = 0; kk < a.apw; ++kk) {
    const int k = k0 + kk;
    if (k >= A) break;
    const double *G = a.atab + (size_t)k * a.Ta * NAF;
    const double *C = a.acst + (size_t)k * NAC;
    const double hlB = C[0], hwB = C[1], hdev = C[2], f_ego = C[3], f_obs = C[4];
    const int prot = (int)C[5], L = (int)C[6];
    const int Lh = min(Tm1, L);

    if (L <= 0) {  // inactive slot (a spawn buffer that is only partly filled): no outputs enter any reduction
      if (a.be_mask) a.be_mask[(size_t)k * a.Mp + m] = 0;
      if (PAIR && valid) {
        const size_t ps_ = (size_t)A * M;
        for (int f = 0; f < FO_NPF; ++f) a.pair_f[(size_t)f * ps_ + (size_t)k * M + m] = NAN;
        for (int f = 0; f < FO_NPI; ++f) a.pair_i[(size_t)f * ps_ + (size_t)k * M + m] = 0;
      }
      if (LISTS && valid) {
        const size_t ls = (size_t)A * Tm1 * M;
        for (int t = 0; t < Tm1; ++t) {
          if (lst_is32(LISTS)) fo_store_lists_f32((float *)a.lists, ls, ((size_t)k * Tm1 + t) * M + m, NAN, NAN, NAN, NAN, NAN);
          else fo_store_lists<false>(a.lists, ls, ((size_t)k * Tm1 + t) * M + m, NAN, NAN, NAN, NAN, NAN);
        }
      }
      continue;
    }

    double dce = INFINITY;
    int tdce = 0;
    bool done = false;
    double max_er = -INFINITY, max_or = -INFINITY, max_eh = -INFINITY, max_oh = -INFINITY, max_cp = -INFINITY;
    double oh_at_cp = 0.0;
    int idx_or = 0, idx_cp = 0;

    // Software pipeline.  Ego samples: E(t) and E(t+1) are in registers when iteration t starts (CP reads t+1 early),
    // the loads of E(t+2) are issued at the top of the iteration and first touched at its bottom.  Agent rows
    // (wave-uniform -> scalar loads): row t in SGPRs, row t+1 requested at the top and first read by the CP step.
    double ex = tj[EF(0)], ey = tj[EF(1)], ec = tj[EF(2)], es = tj[EF(3)], eth = tj[EF(4)], ev = tj[EF(5)];
    const double *tj1 = tj + (size_t)min(1, T - 1) * NEF * Mp;
    double ex1 = tj1[EF(0)], ey1 = tj1[EF(1)], ec1 = tj1[EF(2)], es1 = tj1[EF(3)], eth1 = tj1[EF(4)],
           ev1 = tj1[EF(5)];
    double px = G[0], py = G[1], pc = G[2], ps = G[3], pth = G[4], pv = G[5], isx = G[6], isy = G[7];
    double asr = G[11];   // asin of the covariance's correlation (0: the box probabilities factorise)
    for (int t = 0; t < T; ++t) {
      const double *tj2 = tj + (size_t)min(t + 2, T - 1) * NEF * Mp;
      const double ex2 = tj2[EF(0)], ey2 = tj2[EF(1)], ec2 = tj2[EF(2)], es2 = tj2[EF(3)], eth2 = tj2[EF(4)],
                   ev2 = tj2[EF(5)];
      const double *gn = G + (size_t)min(t + 1, L - 1) * NAF;
      const double npx = gn[0], npy = gn[1], pc1 = gn[2], ps1 = gn[3], npth = gn[4], npv = gn[5], nisx = gn[6],
                   nisy = gn[7], nasr = gn[11];
      const double cr = pc * ec + ps * es;  // cos(yaw - theta)
      const double sr = ps * ec - pc * es;  // sin(yaw - theta)

      // ---------------- DCE (dce.py:69-88): oriented rectangle distance, rounded to 1e-3, first minimum, stop at 0
      if (do_dce && t < L && !(a.ablate & 1)) {
        const double ccx = ex + a.wb * ec, ccy = ey + a.wb * es;  // convert_dynamic_obstacle.py:73
        const double dx = px - ccx, dy = py - ccy;
        // agent centre / half axes in the ego frame
        const double ax = ec * dx + es * dy, ay = ec * dy - es * dx;
        const double ux = hlB * cr, uy = hlB * sr, wx = -hwB * sr, wy = hwB * cr;
        // ego centre / half axes in the agent frame
        const double bx = -(pc * dx + ps * dy), by = -(pc * dy - ps * dx);
        const double vx = a.hlA * cr, vy = -a.hlA * sr, zx = a.hwA * sr, zy = a.hwA * cr;
        const bool sep = (fabs(ax) > a.hlA + fabs(ux) + fabs(wx)) || (fabs(ay) > a.hwA + fabs(uy) + fabs(wy)) ||
                         (fabs(bx) > hlB + fabs(vx) + fabs(zx)) || (fabs(by) > hwB + fabs(vy) + fabs(zy));
        double d2 = 0.0;
        if (sep) {
          d2 = fo_pt_box2(ax + ux + wx, ay + uy + wy, a.hlA, a.hwA);
          d2 = fmin(d2, fo_pt_box2(ax + ux - wx, ay + uy - wy, a.hlA, a.hwA));
          d2 = fmin(d2, fo_pt_box2(ax - ux + wx, ay - uy + wy, a.hlA, a.hwA));
          d2 = fmin(d2, fo_pt_box2(ax - ux - wx, ay - uy - wy, a.hlA, a.hwA));
          d2 = fmin(d2, fo_pt_box2(bx + vx + zx, by + vy + zy, hlB, hwB));
          d2 = fmin(d2, fo_pt_box2(bx + vx - zx, by + vy - zy, hlB, hwB));
          d2 = fmin(d2, fo_pt_box2(bx - vx + zx, by - vy + zy, hlB, hwB));
          d2 = fmin(d2, fo_pt_box2(bx - vx - zx, by - vy - zy, hlB, hwB));
        }
        const double dist = fo_round3(sqrt(d2));
        if (!done && dist < dce) { dce = dist; tdce = t; }
        if (dce == 0.0) done = true;
      }

      if (t < Tm1 && (do_cp || do_hr)) {
        // ---------------- CP (collision_probability.py:69-122): ego sample t+1, agent mean/cov t, agent yaw t+1 (Q1)
        double cp = 0.0;
        if (t + 1 < L) {
          const double devx = pc1 * hdev, devy = ps1 * hdev;
          const double rx = ex1 - px, ry = ey1 - py;  // ego(t+1) - mean
          if (!(sqrt(fo_gate_d2(px, py, devx, devy, ex1, ey1)) > 5.0) && !(a.ablate & 2)) {  // :67,75
            const double bxs = a.len3 * ec1, bys = a.len3 * es1;  // box centre step (L/3 along heading), rear-axle based (Q2)
            double acc = 0.0;
#pragma unroll
            for (int jm = -1; jm <= 1; ++jm) {    // three means
              const double qx = rx - jm * devx, qy = ry - jm * devy;  // ego - mean_j
#pragma unroll
              for (int b = -1; b <= 1; ++b) {     // three boxes
                const double cx = qx + b * bxs, cy = qy + b * bys;
                if (asr != 0.0)   // correlated covariance (wave-uniform: one agent per wave)
                  acc += fo_corr_term_plain(a.gl, (cx - a.off_x) * isx, (cx + a.off_x) * isx, (cy - a.off_y) * isy,
                                            (cy + a.off_y) * isy, asr);
                const double fx = fo_phi_diff(erf_tab, (cx - a.off_x) * isx, (cx + a.off_x) * isx);
                const double fy = fo_phi_diff(erf_tab, (cy - a.off_y) * isy, (cy + a.off_y) * isy);
                acc += fx * fy;
              }
            }
            cp = acc / 3.0;  // :122
          }
        }
        // ---------------- harm (harm_model.py:80-107) + risk (hr.py:78-79), same index on both sides
        double eh = NAN, oh = NAN, er = NAN, orr = NAN;
        if (do_hr && t < Lh && !(a.ablate & 4)) {
          const double dv = sqrt(fmax(ev * ev + pv * pv - 2.0 * ev * pv * cr, 0.0));  // cos(pdof) = -cos(yaw-theta)
          const double ego_dv = f_ego * dv, obs_dv = f_obs * dv;
          if (prot == 1) {
            const double rel = atan2(py - ey, px - ex);  // the impact angles only enter the LR4S model
            const double ego_ang = rel - eth;
            const double obs_ang = M_PI + rel - pth;
            eh = 1.0 / (1.0 + exp(-a.hc.lr4s_const - a.hc.lr4s_speed * ego_dv -
                                  fo_lr4s_coef(ego_ang, a.hc.lr4s_side, a.hc.lr4s_rear)));
            oh = 1.0 / (1.0 + exp(-a.hc.lr4s_const - a.hc.lr4s_speed * obs_dv -
                                  fo_lr4s_coef(obs_ang, a.hc.lr4s_side, a.hc.lr4s_rear)));
          } else if (prot == 0) {
            eh = 1.0 / (1.0 + exp(-a.hc.lr1s_const - a.hc.lr1s_speed * ego_dv));
            oh = 1.0 / (1.0 + exp(a.hc.ped_const - a.hc.ped_speed * obs_dv));
          } else {
            eh = 1.0;
            oh = 1.0;
          }
          er = eh * cp;
          orr = oh * cp;
          max_er = fmax(max_er, er);
          if (orr > max_or) { max_or = orr; idx_or = t; }
          max_eh = fmax(max_eh, eh);
          max_oh = fmax(max_oh, oh);
        }
        if (cp > max_cp) { max_cp = cp; idx_cp = t; oh_at_cp = oh; }
        if (LISTS == LST_F32 && valid)   // (this kernel converts at the store; the queue kernel has a float32 harm path)
          fo_store_lists_f32((float *)a.lists, (size_t)A * Tm1 * M, ((size_t)k * Tm1 + t) * M + m, (float)cp, (float)eh,
                             (float)oh, (float)er, (float)orr);
        else if (LISTS && valid)
          fo_store_lists(a.lists, (size_t)A * Tm1 * M, ((size_t)k * Tm1 + t) * M + m, cp, eh, oh, er, orr);
      }
      ex = ex1; ey = ey1; ec = ec1; es = es1; eth = eth1; ev = ev1;
      ex1 = ex2; ey1 = ey2; ec1 = ec2; es1 = es2; eth1 = eth2; ev1 = ev2;
      px = npx; py = npy; pc = pc1; ps = ps1; pth = npth; pv = npv; isx = nisx; isy = nisy; asr = nasr;
    }

    // ---------------- per-pair scalars
    const double ttc = (fabs(dce) <= 1e-8) ? fo_round3((double)tdce * a.dt) : INFINITY;  // ttc.py:43-46
    const double ttce = fo_round3((double)tdce * a.dt);                                   // ttce.py:39
    if (a.be_mask) a.be_mask[(size_t)k * a.Mp + m] = (do_ttc && ttc < INFINITY && ttc > 0.0) ? 1 : 0;  // be.py:49-50
    const bool hr_valid = do_hr && Lh > 0;
    const double hwc = (max_cp > 0.01) ? oh_at_cp : 0.0;                                   // hr.py:81-84
    if (PAIR && valid) {
      const size_t ps_ = (size_t)A * M;
      double *pf = a.pair_f + (size_t)k * M + m;
      pf[FO_PF_DCE * ps_] = do_dce ? dce : NAN;
      pf[FO_PF_TTC * ps_] = do_ttc ? ttc : NAN;
      pf[FO_PF_TTCE * ps_] = do_ttce ? ttce : NAN;
      pf[FO_PF_MAX_EGO_RISK * ps_] = hr_valid ? max_er : NAN;
      pf[FO_PF_MAX_OBST_RISK * ps_] = hr_valid ? max_or : NAN;
      pf[FO_PF_HARM_WITH_CP * ps_] = hr_valid ? hwc : NAN;
      pf[FO_PF_MAX_EGO_HARM * ps_] = hr_valid ? max_eh : NAN;
      pf[FO_PF_MAX_OBST_HARM * ps_] = hr_valid ? max_oh : NAN;
      pf[FO_PF_MAX_CP * ps_] = hr_valid ? max_cp : NAN;
      pf[FO_PF_BE_DECEL * ps_] = NAN;
      pf[FO_PF_BE_BTN * ps_] = NAN;
      pf[FO_PF_SPARE * ps_] = NAN;
      int32_t *pi = a.pair_i + (size_t)k * M + m;
      pi[FO_PI_TIME_DCE * ps_] = do_dce ? tdce : 0;
      pi[FO_PI_RISK_INDEX * ps_] = hr_valid ? idx_or : 0;
      pi[FO_PI_CP_ARGMAX * ps_] = hr_valid ? idx_cp : 0;
      pi[FO_PI_HR_VALID * ps_] = hr_valid ? 1 : 0;
    }
    // ---------------- fold into the wave's running "all agents" values (first-wins on ties = ascending k)
    if (do_dce) {
      if (dce < w_min_dce) { w_min_dce = dce; w_arg_dce = (double)k; }
      if (dce < a.thr_dce) w_dce_flag = 1.0;  // thr NaN -> never
      if (do_ttc && ttc < w_min_ttc) { w_min_ttc = ttc; w_arg_ttc = (double)k; }
      if (do_ttce) w_min_ttce = fmin(w_min_ttce, ttce);
    }
    if (hr_valid) {
      w_max_er = fmax(w_max_er, max_er);
      if (max_or > w_max_or) { w_max_or = max_or; w_arg_or = (double)k; }
      w_max_eh = fmax(w_max_eh, max_eh);
      w_max_oh = fmax(w_max_oh, max_oh);
      w_max_cp = fmax(w_max_cp, max_cp);
      w_max_hwc = fmax(w_max_hwc, hwc);
    }
  }

  // ---------------- combine the four waves (ascending agent order) and write one partial per (chunk, trajectory)
  if (wave > 0) {
    double *rp = red + (size_t)(wave - 1) * NPS * TILE + lane;
    rp[PS_MIN_DCE * TILE] = w_min_dce; rp[PS_ARG_DCE * TILE] = w_arg_dce; rp[PS_MIN_TTC * TILE] = w_min_ttc;
    rp[PS_ARG_TTC * TILE] = w_arg_ttc; rp[PS_MIN_TTCE * TILE] = w_min_ttce; rp[PS_MAX_ER * TILE] = w_max_er;
    rp[PS_MAX_OR * TILE] = w_max_or; rp[PS_ARG_OR * TILE] = w_arg_or; rp[PS_MAX_EH * TILE] = w_max_eh;
    rp[PS_MAX_OH * TILE] = w_max_oh; rp[PS_MAX_CP * TILE] = w_max_cp; rp[PS_MAX_HWC * TILE] = w_max_hwc;
    rp[PS_DCE_FLAG * TILE] = w_dce_flag; rp[PS_MAX_BTN * TILE] = 0.0;
  }
  __syncthreads();
  if (wave == 0) {
    for (int w = 0; w < WAVES - 1; ++w) {
      const double *rp = red + (size_t)w * NPS * TILE + lane;
      if (rp[PS_MIN_DCE * TILE] < w_min_dce) { w_min_dce = rp[PS_MIN_DCE * TILE]; w_arg_dce = rp[PS_ARG_DCE * TILE]; }
      if (rp[PS_MIN_TTC * TILE] < w_min_ttc) { w_min_ttc = rp[PS_MIN_TTC * TILE]; w_arg_ttc = rp[PS_ARG_TTC * TILE]; }
      w_min_ttce = fmin(w_min_ttce, rp[PS_MIN_TTCE * TILE]);
      w_max_er = fmax(w_max_er, rp[PS_MAX_ER * TILE]);
      if (rp[PS_MAX_OR * TILE] > w_max_or) { w_max_or = rp[PS_MAX_OR * TILE]; w_arg_or = rp[PS_ARG_OR * TILE]; }
      w_max_eh = fmax(w_max_eh, rp[PS_MAX_EH * TILE]);
      w_max_oh = fmax(w_max_oh, rp[PS_MAX_OH * TILE]);
      w_max_cp = fmax(w_max_cp, rp[PS_MAX_CP * TILE]);
      w_max_hwc = fmax(w_max_hwc, rp[PS_MAX_HWC * TILE]);
      w_dce_flag = fmax(w_dce_flag, rp[PS_DCE_FLAG * TILE]);
    }
    const size_t PM = (size_t)a.Mp;
    double *pp = a.partial + (size_t)chunk * NPS * PM + (size_t)tile * TILE + lane;
    pp[PS_MIN_DCE * PM] = w_min_dce; pp[PS_ARG_DCE * PM] = w_arg_dce; pp[PS_MIN_TTC * PM] = w_min_ttc;
    pp[PS_ARG_TTC * PM] = w_arg_ttc; pp[PS_MIN_TTCE * PM] = w_min_ttce; pp[PS_MAX_ER * PM] = w_max_er;
    pp[PS_MAX_OR * PM] = w_max_or; pp[PS_ARG_OR * PM] = w_arg_or; pp[PS_MAX_EH * PM] = w_max_eh;
    pp[PS_MAX_OH * PM] = w_max_oh; pp[PS_MAX_CP * PM] = w_max_cp; pp[PS_MAX_HWC * PM] = w_max_hwc;
    pp[PS_DCE_FLAG * PM] = w_dce_flag; pp[PS_MAX_BTN * PM] = 0.0;
  }
}

}  // namespace
