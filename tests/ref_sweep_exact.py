"""Exact references for the sweep's two discrete / accuracy-critical places, and the inputs that probe them.

DCE (metrics/dce.py:69-88): the reference rounds the polygon distance with np.round(d, 3) = rint(RN(d * 1000)) / 1000,
half to even, keeps the first strict minimum over t and stops at 0.0.  Here the distance of the two float64 rectangles
(vertices formed as the reference forms them, c*lx - s*ly + cx) is computed EXACTLY -- squared distance as a Fraction,
correctly rounded square root through `decimal` at 60 digits -- and rounded as numpy rounds it.

CP (metrics/utils/collision_probability.py:44-122): the box corners and means are formed in float64 as the reference
forms them, the gate is the reference's float64 test; each box probability is then evaluated in mpmath: products of
normal-CDF differences for a diagonal covariance, the bivariate normal box probability (a one-dimensional integral of
the conditional erf difference, split at its narrow features) for a correlated one.

The inputs are built here (deterministic, no random state that depends on a library version) and written, with the
expected outputs, by tests/golden/gen_sweep_exact.py to tests/golden/dce_rounding.npz and tests/golden/cp_exact.npz.
"""
import functools
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- DCE
# Dyadic vehicle: half length 2.25, half width 0.875, rear axle 1.5 behind the centre; with headings of 0 and positions
# on fine dyadic grids every formulation (the reference's vertices and GEOS, the oracle, the kernels' ego-frame corner
# distances) forms the gap without rounding.
DCE_VEH = (4.5, 1.75, 1.5, 1093.3, 11.5)
DCE_DT = 0.1
W = 6                      # samples per agent window: agent k is next to the ego only at t in [W k, W k + W)
U = 2.0 ** -51             # the coordinate step every formulation represents exactly at |coordinates| < 4
TIE_K = (0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6, 8, -8, 12, -12, 16, -16, 24, -24, 32, -32, 48, -48, 64, -64)
# Rotated near-ties (heading pi/6 at a 1 km map offset): a sample is kept only if its exact distance is more than
# ROT_MARGIN from a half millimetre.  Derivation: at |coordinates| < 2^11 one ulp is 2^-42 = 2.3e-13 m.  The reference
# forms each vertex with three rounded operations (c*lx, s*ly, + cx): <= 1.5 ulp = 3.4e-13 m per coordinate, so its
# rectangles sit within 2 * sqrt(2) * 3.4e-13 = 1e-12 m of the exact ones; GEOS then works on differences of a few metres
# (relative 1e-16: < 1e-15 m).  The kernels' ego-frame form (dx = px - ccx, one ulp of 2^11, then rotations of a few
# metres by float64 cos / sin) lands within the same 1e-12 m.  ROT_MARGIN = 1e-9 m leaves a factor of 500 over the sum.
ROT_MARGIN = 1e-9
ROT_OFF = (1000.0, 1000.0)
ROT_TH = math.pi / 6


def rect_vertices(cx, cy, yaw, length, width):
    """the reference's polygon (and fo_oracle_rect_vertices): float64, c*lx - s*ly + cx"""
    c, s = math.cos(yaw), math.sin(yaw)
    lx = (-0.5 * length, -0.5 * length, 0.5 * length, 0.5 * length)
    ly = (-0.5 * width, 0.5 * width, 0.5 * width, -0.5 * width)
    return [(c * lx[i] - s * ly[i] + cx, s * lx[i] + c * ly[i] + cy) for i in range(4)]


def _fr(q):
    return [(Fraction(x), Fraction(y)) for x, y in q]


def _separated(qa, qb):
    """exact SAT on the edge normals of both convex quads: True iff the interiors and boundaries do not meet"""
    for q in (qa, qb):
        for i in range(4):
            ax, ay = q[i]
            bx, by = q[(i + 1) % 4]
            nx, ny = by - ay, ax - bx
            pa = [nx * x + ny * y for x, y in qa]
            pb = [nx * x + ny * y for x, y in qb]
            if max(pa) < min(pb) or max(pb) < min(pa):
                return True
    return False


def _pt_seg2(p, a, b):
    px, py = p
    ax, ay = a
    bx, by = b
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    r = ((px - ax) * dx + (py - ay) * dy)
    if l2 == 0 or r <= 0:
        return (px - ax) ** 2 + (py - ay) ** 2
    if r >= l2:
        return (px - bx) ** 2 + (py - by) ** 2
    cr = (px - ax) * dy - (py - ay) * dx
    return cr * cr / l2


def quad_dist2_exact(qa, qb):
    """exact squared distance (Fraction) between two float64 convex quads; 0 when they touch or overlap"""
    qa, qb = _fr(qa), _fr(qb)
    if not _separated(qa, qb):
        return Fraction(0)
    best = None
    for p, q in ((qa, qb), (qb, qa)):
        for v in p:
            for i in range(4):
                d = _pt_seg2(v, q[i], q[(i + 1) % 4])
                if best is None or d < best:
                    best = d
    return best


getcontext().prec = 60


def sqrt_rn(d2):
    """correctly rounded float64 square root of a non-negative Fraction"""
    if d2 == 0:
        return 0.0
    return float((Decimal(d2.numerator) / Decimal(d2.denominator)).sqrt())


def round_mm(d):
    """np.round(d, 3) * 1000 = rint(RN(d * 1000)), half to even (dce.py:79)"""
    return float(round(d * 1000.0))


def half_mm_gap(d2):
    """|1000 d - (n + 1/2)| in mm for the exact distance sqrt(d2) (how far the sample is from a rounding tie)"""
    x = (Decimal(d2.numerator) / Decimal(d2.denominator)).sqrt() * 1000
    return float(abs(x - (x - Decimal("0.5")).to_integral_value(rounding="ROUND_FLOOR") - Decimal("0.5")))


def _robust(d2):
    """the rounded millimetres do not move when the squared distance moves by 2^-50 relative (any float64 order of
    forming dx^2 + dy^2, fused or not, stays within that)"""
    e = Fraction(1, 2 ** 50)
    return round_mm(sqrt_rn(d2 * (1 - e))) == round_mm(sqrt_rn(d2 * (1 + e)))


def _ego_centre(x, y, th, wb):
    return x + wb * math.cos(th), y + wb * math.sin(th)


@functools.lru_cache(maxsize=None)
def sample_mm(x, y, th, veh, px, py, pyaw, raw_l, raw_w):
    """(rounded millimetres, exact squared distance) of one sample: ego rear-axle pose vs agent pose"""
    cx, cy = _ego_centre(x, y, th, veh[2])
    d2 = quad_dist2_exact(rect_vertices(cx, cy, th, veh[0], veh[1]), rect_vertices(px, py, pyaw, raw_l, raw_w))
    return round_mm(sqrt_rn(d2)), d2


def _np_dist(x, y, th, veh, px, py, pyaw, rl, rw):
    """float64 prefilter (vectorised corner-to-box distance in the ego / agent frames); within 1e-9 of the exact one"""
    cx, cy = x + veh[2] * np.cos(th), y + veh[2] * np.sin(th)
    dx, dy = px - cx, py - cy
    ec, es, pc, ps = np.cos(th), np.sin(th), np.cos(pyaw), np.sin(pyaw)
    cr, sr = pc * ec + ps * es, ps * ec - pc * es
    hlA, hwA, hlB, hwB = veh[0] / 2, veh[1] / 2, rl / 2, rw / 2
    ax, ay = ec * dx + es * dy, ec * dy - es * dx
    bx, by = -(pc * dx + ps * dy), -(pc * dy - ps * dx)
    ux, uy, wx, wy = hlB * cr, hlB * sr, -hwB * sr, hwB * cr
    vx, vy, zx, zy = hlA * cr, -hlA * sr, hwA * sr, hwA * cr
    sep = ((np.abs(ax) > hlA + np.abs(ux) + np.abs(wx)) | (np.abs(ay) > hwA + np.abs(uy) + np.abs(wy)) |
           (np.abs(bx) > hlB + np.abs(vx) + np.abs(zx)) | (np.abs(by) > hwB + np.abs(vy) + np.abs(zy)))

    def box2(qx, qy, hl, hw):
        return np.maximum(np.abs(qx) - hl, 0) ** 2 + np.maximum(np.abs(qy) - hw, 0) ** 2
    d2 = np.minimum.reduce([box2(ax + s1 * ux + s2 * wx, ay + s1 * uy + s2 * wy, hlA, hwA)
                            for s1 in (1, -1) for s2 in (1, -1)] +
                           [box2(bx + s1 * vx + s2 * zx, by + s1 * vy + s2 * zy, hlB, hwB)
                            for s1 in (1, -1) for s2 in (1, -1)])
    return np.where(sep, np.sqrt(d2), 0.0)


def build_dce_inputs():
    """sweep inputs of tests/golden/dce_rounding.npz and one label per trajectory (what it probes).

    Six agents, each next to the ego only in its own window of W samples (elsewhere 300 m away); each trajectory visits
    one agent's window, and sits 300 m off elsewhere.  Agents 0..4 are axis-aligned and stationary in their window, the
    trajectories move the ego, so a gap g is the ego's rear axle at -g: every coordinate is a multiple of 2^-51 below 4.
      0  face to face along x (agent 0.5 x 2.0 ahead, wider than the ego: GEOS' vertex-to-segment path divides by 4)
      1  face to face along y (agent 8.0 x 0.5 beside the ego)
      2  corner to corner (agent 1 x 1, diagonal offsets 3-4-5 and 5-12-13 scaled by odd multiples of 1/16)
      3  walks: several tied or near-tied samples per pair, one later sample at n + 0.5 mm +- ulps
      4  the 0.5 mm boundary: gaps on the 2^-51 grid next to 0.0005 m, touching and overlapping (TTC straddles)
      5  rotated: headings pi/6 (+ 0.4 for half of them) at a 1 km map offset, exact distances near half millimetres
    """
    A, T = 6, 6 * W
    FAR = 300.0
    raw = np.array([[0.5, 2.0], [8.0, 0.5], [1.0, 1.0], [0.5, 2.0], [0.5, 2.0], [4.0, 1.8]])
    canon = [(4.0, 0.0, 0.0), (1.5, 1.125, 0.0), (4.25, 1.375, 0.0), (4.0, 0.0, 0.0), (4.0, 0.0, 0.0), None]
    pos = np.zeros((A, T, 2))
    yaw = np.zeros((A, T))
    for k in range(A):
        pos[k, :, 0] = 20.0 * k
        pos[k, :, 1] = FAR
        if canon[k] is not None:
            pos[k, W * k:W * k + W] = canon[k][:2]
            yaw[k, W * k:W * k + W] = canon[k][2]
    rows = []        # (agent, [ (x, y, th) per window sample ], label)

    def xface(g):
        return (-g, 0.0, 0.0)

    def yface(g):
        return (0.0, -g, 0.0)

    def corner(gx, gy):
        return (-gx, -gy, 0.0)

    far = (None, None, None)
    # 0 / 1: faces at odd multiples of 1/16 m, +- k steps of 2^-51 m: the first sample is the tie, the rest far
    for k_agent, mk, jmax in ((0, xface, 12), (1, yface, 12)):
        for j in range(jmax):
            g0 = (2 * j + 1) / 16.0
            for k in TIE_K:
                g = g0 + k * U
                rows.append((k_agent, [mk(g)] + [mk(g0 + 0.25 + 0.0078125 * (i + 1)) for i in range(W - 1)],
                             f"face{k_agent} {g0} {k:+d}"))
    # 2: corners (3n/16, 4n/16), (4n/16, 3n/16), (5n/16, 12n/16), (12n/16, 5n/16), n odd; +- k steps on the x gap
    for a, b in ((3, 4), (4, 3), (5, 12), (12, 5)):
        for n in ((1, 3, 5) if a == 3 else (1, 3) if a == 4 else (1,)):
            for k in TIE_K[:17]:
                gx, gy = a * n / 16.0 + k * U, b * n / 16.0
                if k and not _robust(Fraction(gx) ** 2 + Fraction(gy) ** 2):
                    continue      # closer to the tie than the float64 forms of the squared distance can resolve
                rows.append((2, [corner(gx, gy)] + [corner(gx + 0.3125, gy)] * (W - 1), f"corner {a}-{b} n{n} {k:+d}"))
    # 3: walks -- deterministic pseudo-random picks from ties, near-ties and whole-millimetre neighbours
    rng = np.random.Generator(np.random.PCG64(20261016))
    for w in range(96):
        j = int(rng.integers(0, 8))
        g0 = (2 * j + 1) / 16.0
        ks = [int(rng.choice(TIE_K[:9])) for _ in range(W - 1)]
        gaps = [g0 + k * U for k in ks]
        if w % 3 == 0:
            gaps[int(rng.integers(0, W - 1))] = g0 + 0.00125     # 1.25 mm farther
        if w % 4 == 1:
            gaps[int(rng.integers(0, W - 1))] = g0 - 0.0009765625   # a millimetre nearer (2^-10)
        # the last sample sits at the tie +- ulps: next to the (nmm + 0.51) mm pruning bound of the queue kernels
        gaps.append(g0 + int(rng.choice((0, 1, -1, 2, -2, 8, -8))) * U)
        rows.append((3, [xface(g) for g in gaps], f"walk {w}"))
    # 4: the 0.5 mm boundary (TTC finite iff the rounded distance is 0.0)
    g05 = math.floor(0.0005 / U) * U
    for i, k in enumerate((-3, -2, -1, 0, 1, 2, 3, 4)):
        g = g05 + k * U
        t_at = 1 + i % (W - 1)
        gaps = [0.01 + 0.001 * s for s in range(W)]
        gaps[t_at] = g
        rows.append((4, [xface(q) for q in gaps], f"half-mm {k:+d}"))
    for g in (0.0, -U, -0.0009765625, 0.0009765625):        # touching, overlapping by one step / by 2^-10, 2^-10 apart
        rows.append((4, [xface(0.02), xface(0.01), xface(g), xface(0.0), xface(0.5), xface(g)], f"touch {g}"))
    # 5: rotated near-ties at a 1 km offset
    rot = []
    for i in range(48):
        th_a = ROT_TH + (0.4 if i % 2 else 0.0)
        nmm = 40 + 7 * i
        delta = (2.0, -2.0, 5.0, -5.0, 20.0, -20.0, 100.0, -100.0)[i % 8] * ROT_MARGIN
        rot.append((th_a, (nmm + 0.5) * 1e-3 + delta))
    A5, k5 = 5, 5
    pos[A5, W * k5:W * k5 + W] = (ROT_OFF[0] + 3.0, ROT_OFF[1] + 2.0)
    yaw[A5, W * k5:W * k5 + W] = [ROT_TH, ROT_TH, ROT_TH + 0.4, ROT_TH + 0.4, ROT_TH, ROT_TH + 0.4]
    ax_, ay_ = ROT_OFF[0] + 3.0, ROT_OFF[1] + 2.0
    for i in range(0, len(rot), W):
        poses = []
        for s in range(W):
            th_a = float(yaw[A5, W * k5 + s])
            _, gap = rot[i + s] if i + s < len(rot) else (th_a, 1.0)
            # ego heading ROT_TH, centre `back` behind the agent centre along the ego heading, shifted across so that the
            # nearest feature is the agent's corner (tilted agent) or its face (parallel): the distance is then found by
            # bisection on the float64 position (the exact value is computed afterwards, not assumed)
            poses.append(_place_rotated(ax_, ay_, th_a, gap, raw[A5]))
        rows.append((5, poses, f"rotated {i // W}"))
    M = len(rows)
    x = np.empty((M, T))
    y = np.empty((M, T))
    th = np.zeros((M, T))
    for m, (k, poses, _) in enumerate(rows):
        x[m] = -3.75
        y[m] = -FAR
        for s, (ex, ey, et) in enumerate(poses):
            x[m, W * k + s], y[m, W * k + s], th[m, W * k + s] = ex, ey, et
    traj = {"x": x, "y": y, "theta": th, "v": np.zeros((M, T)), "a": np.zeros((M, T))}
    agents = {"pos": pos, "yaw": yaw, "v": np.zeros((A, T)), "cov": np.tile(np.eye(2) * 0.1, (A, T, 1, 1)),
              "shape": raw.copy(), "raw_dims": raw.copy(), "type": np.zeros(A, dtype=np.int32),
              "len": np.full(A, T, dtype=np.int32)}
    return traj, agents, [r[2] for r in rows], np.array([r[0] for r in rows])


def _place_rotated(ax, ay, th_a, gap, raw):
    """ego rear-axle pose (heading ROT_TH) whose float64 rectangle is `gap` from the agent's, to ~1e-15 m"""
    hlA, hwA = DCE_VEH[0] / 2, DCE_VEH[1] / 2
    c, s = math.cos(ROT_TH), math.sin(ROT_TH)

    def pose(back):
        ccx, ccy = ax - back * c + 0.3 * s, ay - back * s - 0.3 * c
        return ccx - DCE_VEH[2] * c, ccy - DCE_VEH[2] * s

    def dist(back):
        x, y = pose(back)
        return float(_np_dist(np.array(x), np.array(y), np.array(ROT_TH), DCE_VEH, np.array(ax), np.array(ay),
                              np.array(th_a), raw[0], raw[1]))
    lo, hi = hlA, hlA + raw[0] + raw[1] + 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if dist(mid) < gap:
            lo = mid
        else:
            hi = mid
        if hi - lo < 1e-15:
            break
    x, y = pose(hi)
    return (x, y, ROT_TH)


def expected_dce(traj, agents, veh, dt, ttc_thr):
    """exact dce [M, A] (metres), time_dce, ttc, ttce [M, A], safe [M] (TTC threshold only), and per-sample records
    (m, a, t, mm, exact tie?, gap to the nearest half millimetre in mm) of every sample evaluated exactly"""
    x, y, th = traj["x"], traj["y"], traj["theta"]
    M, T = x.shape
    A = agents["pos"].shape[0]
    dce = np.full((M, A), np.inf)
    tdce = np.zeros((M, A), dtype=np.int64)
    recs = []
    for k in range(A):
        L = min(int(agents["len"][k]), T)
        rl, rw = agents["raw_dims"][k]
        px, py, pyaw = agents["pos"][k, :L, 0], agents["pos"][k, :L, 1], agents["yaw"][k, :L]
        fd = _np_dist(x[:, :L], y[:, :L], th[:, :L], veh, px[None], py[None], pyaw[None], rl, rw)
        lim = fd.min(axis=1) + 0.003          # only samples within 3 mm of the nearest can attain the rounded minimum
        for m in range(M):
            best, bt = math.inf, 0
            for t in np.nonzero(fd[m] <= lim[m])[0]:
                t = int(t)
                mm, d2 = sample_mm(float(x[m, t]), float(y[m, t]), float(th[m, t]), tuple(veh), float(px[t]), float(py[t]),
                                   float(pyaw[t]), float(rl), float(rw))
                r = sqrt_rn(d2)
                tie = d2 != 0 and Fraction(r) ** 2 == d2 and (r * 1000.0) % 1.0 == 0.5
                recs.append((m, k, t, mm, tie, half_mm_gap(d2) if d2 else 0.5))
                if mm < best:
                    best, bt = mm, t
                if best == 0.0:
                    break
            dce[m, k] = best / 1000.0
            tdce[m, k] = bt
    ttc = np.where(np.abs(dce) <= 1e-8, np.round(tdce * dt, 3), np.inf)
    ttce = np.round(tdce * dt, 3)
    safe = ~(ttc < ttc_thr).any(axis=1)
    return dce, tdce, ttc, ttce, safe, np.array(recs, dtype=[("m", "i4"), ("a", "i4"), ("t", "i4"), ("mm", "f8"),
                                                             ("tie", "?"), ("gap_mm", "f8")])


# ----------------------------------------------------------------------------------------------------------------- CP
CP_VEH = DCE_VEH
CP_DT = 0.1
CP_T = 33
ZONE = 16.0                 # agent k sits at its own zone centre; a trajectory visits one zone, the others are > 5 m off
RHO_SWITCH = (0.5, 0.7, 0.9, 0.97)        # where the sweep changes its Gauss-Legendre rule (GL_ASR, fo_sweep_common.hpp)
RHO_EXTRA = (0.99, -0.99, 0.985, -0.985, 0.3, -0.6)
# (sxx, syy): powers of two, so that rho = sxy / sqrt(sxx syy) is the float64 rho exactly in every implementation.  Box
# widths in units of sigma sqrt 2: 34 x 40 (tight), 1.06 x 2.47, 0.023 x 0.055 (wide)
CORR_SIG = ((2.0 ** -10, 2.0 ** -10), (1.0, 0.25), (2.0 ** 11, 2.0 ** 9))
DIAG_SIG = ((0.5, 0.01), (0.01, 0.5), (1e-6, 1e-6), (1e-4, 1e-4), (1e-2, 1e-2), (1.0, 1.0), (1e2, 1e2), (1e4, 1e4),
            (0.0, 0.0))
STEP = 1.0 / (128 * 7)      # a seventh of an erf table step at sigma sqrt 2 = 1 (sigma^2 = 0.5)


def cp_rhos():
    r = []
    for v in RHO_SWITCH:
        r += [math.nextafter(v, 0.0), math.nextafter(v, 1.0)]
    return tuple(r) + RHO_EXTRA


def build_cp_inputs():
    """sweep inputs of tests/golden/cp_exact.npz: one agent per covariance, stationary at its zone centre with heading 0
    and inflated length 0.5 (means 0.25 apart); each trajectory visits one zone; the ego offsets from the mean are
      diagonal (sxx, syy) = (0.5, 0.01): x swept from -3.8 to 3.8 m in steps of 1/896 m -- every erf table node 0..768 at
        seven phases per step (sigma sqrt 2 = 1) -- plus a 64-per-step sweep where a box edge is at u = +-0.6 (the worst
        case of the dropped Taylor terms); (0.01, 0.5): the same across y, coarser;
      diagonal sigma^2 = 1e-6 ... 1e4 and the zero matrix (-> 0.1 I): half uniform in the gate, half within 4 sigma of
        a box edge (arguments far past the table's end for the tight ones);
      correlated: rho on both sides of each rule switch and at +-0.99, +-0.985, 0.3, -0.6, three variance pairs; means
        within 30 sigma of a box corner, half of them near h = +-k.
    Out-of-gate samples sit 9 m off."""
    rng = np.random.Generator(np.random.PCG64(20261017))
    covs, rows = [], []          # covs[k] = (sxx, sxy, syy); rows: (k, [offset (dx, dy) of ego rear axle - mean, per t])
    for sxx, syy in DIAG_SIG:
        covs.append((sxx, 0.0, syy))
    offs = []
    xs = np.arange(-3.8, 3.8, STEP)
    fine = np.concatenate([e - u + np.arange(-64, 65) / (128 * 64) for e in (-2.25, -0.75, 0.75, 2.25)
                           for u in (0.6, -0.6)])
    offs = [(float(v), 0.0) for v in np.concatenate([xs, fine])]
    rows += _chunk(0, offs)
    rows += _chunk(1, [(0.0, float(v)) for v in np.arange(-4.5, 4.5, 8 * STEP)])
    edges_x, edges_y = (-2.25, -0.75, 0.75, 2.25), (-0.875, 0.875)
    for k in range(2, len(DIAG_SIG)):
        s = math.sqrt(DIAG_SIG[k][0] or 0.1)
        o = [(float(rng.uniform(-3.5, 3.5)), float(rng.uniform(-3.0, 3.0))) for _ in range(32)]
        o += [(float(rng.choice(edges_x) + s * rng.uniform(-4, 4)), float(rng.choice(edges_y) + s * rng.uniform(-4, 4)))
              for _ in range(32)]
        rows += _chunk(k, o)
    for rho in cp_rhos():
        for sxx, syy in CORR_SIG:
            k = len(covs)
            covs.append((sxx, rho * math.sqrt(sxx * syy), syy))
            sx, sy = math.sqrt(sxx), math.sqrt(syy)
            o = []
            for i in range(4):
                ex, ey = float(rng.choice(edges_x)), float(rng.choice(edges_y))
                if sxx < 1e-2:      # tight: a corner of the box within 30 sigma of the mean, half near h = +-k
                    h = rng.uniform(-30, 30)
                    kk = (h if i % 2 else -h) * sx / sy + rng.uniform(-0.5, 0.5) if i >= 2 else rng.uniform(-30, 30)
                    o.append((ex - h * sx, ey - kk * sy))
                else:
                    o.append((float(rng.uniform(-3.0, 3.0)), float(rng.uniform(-2.5, 2.5))))
            rows += _chunk(k, [(float(a), float(b)) for a, b in o], per=4)
    A, T = len(covs), CP_T
    zc = np.array([(ZONE * (k % 8), ZONE * (k // 8)) for k in range(A)])
    M = len(rows)
    x, y = np.empty((M, T)), np.empty((M, T))
    for m, (k, o) in enumerate(rows):
        x[m], y[m] = zc[k, 0], zc[k, 1] + 9.0
        for i, (dx, dy) in enumerate(o):
            x[m, 1 + i], y[m, 1 + i] = zc[k, 0] + dx, zc[k, 1] + dy
    cov = np.array([[[a, b], [b, c]] for a, b, c in covs])
    agents = {"pos": np.repeat(zc[:, None, :], T, 1), "yaw": np.zeros((A, T)), "v": np.zeros((A, T)),
              "cov": np.repeat(cov[:, None], T, 1), "shape": np.tile([0.5, 0.5], (A, 1)),
              "raw_dims": np.tile([0.5, 0.5], (A, 1)), "type": np.full(A, 4, dtype=np.int32),
              "len": np.full(A, T, dtype=np.int32)}
    traj = {"x": x, "y": y, "theta": np.zeros((M, T)), "v": np.zeros((M, T)), "a": np.zeros((M, T))}
    return traj, agents, np.array([r[0] for r in rows])


def _chunk(k, offs, per=CP_T - 1):
    """trajectories for agent k: `per` in-gate samples each (the rest of the T - 1 CP samples 9 m off)"""
    return [(k, offs[i:i + per]) for i in range(0, len(offs), per)]


_L_CACHE = {}


def _bvn_corr(h, k, rho):
    """(1 / 2 pi) Int_0^asin(rho) exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt: L(h, k; rho) - Phi(-h) Phi(-k)"""
    import mpmath as mp
    key = (h, k, rho)
    if key not in _L_CACHE:
        f = lambda t: mp.exp(-(h * h + k * k - 2 * h * k * mp.sin(t)) / (2 * mp.cos(t) ** 2))  # noqa: E731
        _L_CACHE[key] = mp.quad(f, [0, mp.asin(rho)]) / (2 * mp.pi)
    return _L_CACHE[key]


def expected_cp(traj, agents, veh):
    """exact per-sample CP lists [M, A, T-1] and the per-argument record (u = argument in units of sigma sqrt 2) of
    every diagonal erf evaluated"""
    import mpmath as mp
    mp.mp.dps = 20
    x, y, th = traj["x"], traj["y"], traj["theta"]
    M, T = x.shape
    A = agents["pos"].shape[0]
    cp = np.zeros((M, A, T - 1))
    us = []
    off = np.array([veh[0] / 6, veh[1] / 2])
    ncdf = {}

    def Phi(z):
        if z not in ncdf:
            ncdf[z] = mp.ncdf(z)
        return ncdf[z]
    for k in range(A):
        L = min(int(agents["len"][k]), T)
        pos, yaw, covs = agents["pos"][k], agents["yaw"][k], agents["cov"][k]
        length = agents["shape"][k, 0]
        # the reference's gate, vectorised over (m, i): (mean + j dev) - ego, each square rounded, then the sum
        devs = np.stack((np.cos(yaw[1:L]), np.sin(yaw[1:L])), -1) * length / 2
        mean_all = np.array([pos[:L - 1], pos[:L - 1] + devs, pos[:L - 1] - devs])
        egos = np.stack((x[:, 1:L], y[:, 1:L]), -1)
        dist = mean_all[:, None] - egos[None]
        ing = ~(np.sqrt(dist[..., 0] ** 2 + dist[..., 1] ** 2).min(axis=0) > 5.0)
        for m, i in zip(*np.nonzero(ing)):
            i = int(i) + 1
            ego = egos[m, i - 1]
            means = mean_all[:, i - 1]
            c = covs[i - 1]
            if c[0, 0] == 0 and c[0, 1] == 0 and c[1, 0] == 0 and c[1, 1] == 0:
                c = np.array([[0.1, 0.0], [0.0, 0.1]])
            sx, sy = mp.sqrt(mp.mpf(c[0, 0])), mp.sqrt(mp.mpf(c[1, 1]))
            rho = mp.mpf(c[0, 1]) / (sx * sy)
            r_x = veh[0] / 2
            a_x = np.array([np.cos(th[m, i]), np.sin(th[m, i])])
            centres = np.array([ego, ego + r_x * (2 / 3) * a_x, ego - r_x * (2 / 3) * a_x])
            ur, ll = centres + off, centres - off
            acc = mp.mpf(0)
            for mu in means:
                for b in range(3):
                    hx = [(mp.mpf(float(v)) - mp.mpf(float(mu[0]))) / sx for v in (ll[b, 0], ur[b, 0])]
                    hy = [(mp.mpf(float(v)) - mp.mpf(float(mu[1]))) / sy for v in (ll[b, 1], ur[b, 1])]
                    p = (Phi(hx[1]) - Phi(hx[0])) * (Phi(hy[1]) - Phi(hy[0]))
                    if rho != 0:
                        p += (_bvn_corr(hx[0], hy[0], rho) - _bvn_corr(hx[1], hy[0], rho)
                              - _bvn_corr(hx[0], hy[1], rho) + _bvn_corr(hx[1], hy[1], rho))
                    elif m < M:
                        us += [float(v / mp.sqrt(2)) for v in hx + hy]
                    acc += p
            cp[m, k, i - 1] = float(acc / 3)
    return cp, np.array(us)
