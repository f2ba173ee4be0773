"""Two plain references of the brake evaluation (metrics/be.py:31-193), NumPy and the standard library only.  Neither shares
code with the CPU oracle (oracle/fo_oracle.c) or the device kernel (csrc/fo_sweep_be_reduce.hpp).

be_exact  -- be.py:31-193 in fractions.Fraction for the geometry a rational can hold: a straight ego path along +x with
             theta = 0 and axis-aligned agents (yaw = 0).  Every input is a float and is taken at its exact value; the speed
             profile, the left-Riemann arc, the clamp at the path end, the re-sampling, the rectangle test (touching counts) and
             the bracket with its stop rule are exact.  The candidates are the doubles the reference's float bisection visits:
             a midpoint (lo + hi) / 2 is rounded to the nearest double (`_nearest_double`, a conversion, not an operation; the
             identity whenever the bracket starts at 0, where every midpoint is a short dyadic).
be_float  -- find_minimum_deceleration (be.py:66-193) for one (trajectory, agent) pair in float64 with NumPy's operation
             order: cumsum arcs, searchsorted(side="left") clipped to [1, T - 1], scipy's slope * (s - x_lo) + y_lo, and a
             separating-axis test of its own that returns a signed separation (hit: sep <= 0).  Its `info` says what neither
             the device nor the oracle can report: iterations, whether the end-of-path clamp engaged, whether a zero-length
             segment was read, and the smallest |sep| over every rectangle test of the bisection.

Two deviations from the reference, shared with the oracle and the device: an arc length past the end of the path is clamped
(scipy raises ValueError), and a zero-length path segment returns its left knot (scipy divides by zero: NaN)."""
from fractions import Fraction

import numpy as np

MAX_DECEL, STOP_WIDTH, MAX_ITER = 5, 0.1, 10          # be.py:66 (max_decel, threshold, max_iterations)


# ----------------------------------------------------------------------------------------------------------- exact
def _nearest_double(q):
    return Fraction(float(q))


def _round_half_even_2(q):
    """np.round(q, 2) for q >= 0: rint(q * 100) / 100 -- the integer exactly, the quotient as the nearest double"""
    n = round(q * 100)                                  # Fraction.__round__: half to even, like rint
    return _nearest_double(Fraction(n, 100))


def _exact_pose_x(dist, x, s, j=0):
    """interp1d(dist, x)(s) with searchsorted-left, clipped; the left knot on a zero-length segment.  j: a knot index known
    to be at or below the one searched for (the arc lengths of one profile never decrease); returns (x, the index found)"""
    T = len(dist)
    while j < T and dist[j] < s:
        j += 1
    idx = min(max(j, 1), T - 1)
    lo, hi = dist[idx - 1], dist[idx]
    if hi == lo:
        return x[idx - 1], j
    return (x[idx] - x[idx - 1]) / (hi - lo) * (s - lo) + x[idx - 1], j


def _exact_touch(cx, cy, hl, hw, px, py, al, aw):
    """axis-aligned rectangles intersect, a shared boundary point included (shapely `intersects`)"""
    return abs(cx - px) <= hl + al / 2 and abs(cy - py) <= hw + aw / 2


def _exact_collides(x, y0, v, dist, decel, agent_pos, agent_dims, L, veh, dt):
    length, width, wb = (Fraction(q) for q in veh[:3])
    T = len(x)
    s, j = Fraction(0), 0
    for i in range(min(T, L)):                    # (the samples the agent exists at; be.py:165-167 tests no other)
        xn, j = _exact_pose_x(dist, x, min(s, dist[-1]), j)
        if _exact_touch(xn + wb, y0, length / 2, width / 2, agent_pos[i][0], agent_pos[i][1], *agent_dims):
            return True
        vn = v[0] if i == 0 else max(v[1] - decel * ((i - 1) * dt), Fraction(0))
        s += vn * dt
    return False


def be_exact(x, y0, v, a, agent_pos, agent_dims, L, veh, dt):
    """(required constant deceleration, brake threat number) of be.py:31-62 as Fractions, or (None, None) for L == 0 (no
    prediction: no entry).  x, v, a: the ego's samples [T] (y = y0, theta = 0); agent_pos [>= min(L, T)][2], agent_dims
    (length, width) at yaw = 0; veh = (length, width, wb_rear_axle, mass, a_max)."""
    F = Fraction
    x, v, a = [F(float(q)) for q in x], [F(float(q)) for q in v], [F(float(q)) for q in a]
    y0, dt = F(float(y0)), F(float(dt))
    agent_pos = [(F(float(p[0])), F(float(p[1]))) for p in agent_pos]
    agent_dims = (F(float(agent_dims[0])), F(float(agent_dims[1])))
    if L <= 0:
        return None, None
    T = len(x)
    length, width, wb = (F(float(q)) for q in veh[:3])
    # ttc (dce.py:79-86, ttc.py:43 on this geometry): the first sample whose rectangle distance rounds to 0.000 -- the walk ends
    # there, and a distance of up to half a millimetre counts as a collision although no candidate of the bisection touches
    def collides(i):
        gx = max(abs(x[i] + wb - agent_pos[i][0]) - length / 2 - agent_dims[0] / 2, F(0))
        gy = max(abs(y0 - agent_pos[i][1]) - width / 2 - agent_dims[1] / 2, F(0))
        return gx * gx + gy * gy <= F(1, 2000) ** 2
    first = next((i for i in range(min(L, T)) if collides(i)), None)
    if first is None or first == 0 or T < 2:
        return F(0), F(0)
    dist = [F(0)]
    for i in range(1, T):
        dist.append(dist[-1] + abs(x[i] - x[i - 1]))                            # sqrt(dx^2 + 0^2)
    lo, hi = _round_half_even_2(abs(min(min(a), F(0)))), F(MAX_DECEL)
    cur = F(0)
    for _ in range(MAX_ITER):
        cur = _nearest_double((lo + hi) / 2)
        if _exact_collides(x, y0, v, dist, cur, agent_pos, agent_dims, L, veh, dt):
            lo = cur
        else:
            hi = cur
        if hi - lo < F(STOP_WIDTH):                                             # the double 0.1, at its exact value
            break
    return cur, cur / F(float(veh[4]))


# ----------------------------------------------------------------------------------------------------------- float64
def _separation(cx, cy, th, hlA, hwA, px, py, yaw, hlB, hwB):
    """signed separation of two rectangles (arrays over the samples): the largest gap along the four edge normals, > 0 iff
    the rectangles are apart, 0 when they touch"""
    ca, sa, cb, sb = np.cos(th), np.sin(th), np.cos(yaw), np.sin(yaw)
    dx, dy = px - cx, py - cy
    cr, sr = np.abs(ca * cb + sa * sb), np.abs(sa * cb - ca * sb)               # |cos|, |sin| of the relative heading
    g1 = np.abs(dx * ca + dy * sa) - (hlA + hlB * cr + hwB * sr)
    g2 = np.abs(dy * ca - dx * sa) - (hwA + hlB * sr + hwB * cr)
    g3 = np.abs(dx * cb + dy * sb) - (hlB + hlA * cr + hwA * sr)
    g4 = np.abs(dy * cb - dx * sb) - (hwB + hlA * sr + hwA * cr)
    return np.maximum(np.maximum(g1, g2), np.maximum(g3, g4))


def _resample(dist, ys, s, info):
    """scipy interp1d (linear) at s: y_lo + slope * (s - x_lo) on the searchsorted-left segment"""
    idx = np.clip(np.searchsorted(dist, s, side="left"), 1, len(dist) - 1)
    lo, hi = dist[idx - 1], dist[idx]
    flat = hi == lo
    if flat.any():
        info["zero_segment"] = True
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (ys[idx] - ys[idx - 1]) / (hi - lo)
        out = slope * (s - lo) + ys[idx - 1]
    return np.where(flat, ys[idx - 1], out)


def first_contact(traj_row, agent, veh):
    """index of the first of the ego's own samples at which the rectangles intersect (sep <= 0), None without one; and the
    smallest positive sep of those samples (the reference rounds its distances to the millimetre, dce.py:79: a gap below half a
    millimetre is a collision to ttc.py -- a caller that takes `first` for the time to collision wants that gap well above)"""
    x, y, th = (np.asarray(traj_row[k], dtype=np.float64) for k in ("x", "y", "theta"))
    n = min(int(agent["len"]), len(x), len(agent["yaw"]))
    if n <= 0:
        return None, np.inf
    pos, yaw = np.asarray(agent["pos"], dtype=np.float64)[:n], np.asarray(agent["yaw"], dtype=np.float64)[:n]
    length, width, wb = veh[:3]
    sep = _separation(x[:n] + wb * np.cos(th[:n]), y[:n] + wb * np.sin(th[:n]), th[:n], length / 2, width / 2, pos[:, 0], pos[:, 1],
                      yaw, agent["raw_dims"][0] / 2, agent["raw_dims"][1] / 2)
    hit = np.flatnonzero(sep <= 0)
    return (int(hit[0]) if len(hit) else None), float(sep[sep > 0].min()) if (sep > 0).any() else np.inf


def be_float(traj_row, agent, veh, dt, slack=0.0):
    """find_minimum_deceleration for one pair.  traj_row: x, y, theta, v, a [T]; agent: pos [Ta, 2], yaw [Ta], raw_dims (length,
    width), len.  Returns (decel, info).  slack: a hit is sep <= slack -- what another implementation's rounding may make of
    a pair whose rectangles come within |slack| of touching (0: the reference's predicate)."""
    x, y, th, v, a = (np.asarray(traj_row[k], dtype=np.float64) for k in ("x", "y", "theta", "v", "a"))
    T = len(x)
    n = min(int(agent["len"]), T, len(agent["yaw"]))
    pos, yaw = np.asarray(agent["pos"], dtype=np.float64)[:n], np.asarray(agent["yaw"], dtype=np.float64)[:n]
    hlB, hwB = agent["raw_dims"][0] / 2, agent["raw_dims"][1] / 2
    length, width, wb = veh[:3]
    info = {"iterations": 0, "clamped": False, "zero_segment": False, "min_abs_sep": np.inf}
    dist = np.insert(np.cumsum(np.sqrt(np.diff(x) ** 2 + np.diff(y) ** 2)), 0, 0)                       # be.py:100
    time = np.arange(T - 1) * dt                                                                       # be.py:103
    lo, hi = np.round(abs(min(min(a), 0)), 2), MAX_DECEL                                               # be.py:68
    cur = 0.0
    for _ in range(MAX_ITER):
        cur = (lo + hi) / 2
        info["iterations"] += 1
        v_new = np.insert(np.maximum(v[1] - cur * time, 0), 0, v[0:1])                                 # be.py:110
        s = np.insert(np.cumsum(v_new * dt), 0, 0)[:-1][:n]                                            # be.py:114
        past = s > dist[-1]                                                                            # (the reference raises)
        s = np.minimum(s, dist[-1])
        xn, yn, tn = _resample(dist, x, s, info), _resample(dist, y, s, info), _resample(dist, th, s, info)
        sep = _separation(xn + wb * np.cos(tn), yn + wb * np.sin(tn), tn, length / 2, width / 2, pos[:, 0], pos[:, 1], yaw, hlB, hwB)
        hit = np.flatnonzero(sep <= slack)
        upto = hit[0] + 1 if len(hit) else n                      # (the reference stops at the first intersecting sample)
        info["min_abs_sep"] = min(info["min_abs_sep"], float(np.abs(sep[:upto]).min()))
        info["clamped"] = info["clamped"] or bool(past[:upto].any())
        if len(hit):
            lo = cur
        else:
            hi = cur
        if hi - lo < STOP_WIDTH:
            break
    return float(cur), info
