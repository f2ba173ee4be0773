"""An independent statement of the phantom predictions (spawn point -> the rows the sweep reads): what
fo_spawn_rule_predict_kernel / fo_spawn_predict_kernel (csrc/fo_spawn_rules.hpp, csrc/fo_scene.hip), the C oracle
(fo_oracle_route_predictions, fo_oracle_cv_predictions, fo_oracle_spawn_headings) and the host path
(FOAgentManager._route_prediction, _cv_prediction, _heading_towards_path) all compute -- written a fourth time, but not as a
fourth float64 transcription: plain Python, nothing shared with oracle/ or the package.

  decisions   in exact rational arithmetic (fractions.Fraction) on the float64 inputs: the first lanelet in list order that
              holds the point, the first minimum of the squared distance over the segments, the nearest of {-0.5, 0, 0.5}
              (first of equally near ones), sk <= s_end, the segment under a sample.  Where a square root that a decision
              depends on is irrational the comparison is made at 60 digits.
  values      sqrt, atan2, pow, the quintic, sin / cos with mpmath at 60 digits, rounded once to float64.
  exception   the three-decimal rounding of the straight form's velocity is the reference's float64 statement,
              round(np.float64, 3) = rint(1000 x) / 1000, applied to the float64 product v cos(a) / v sin(a).

Every decision carries a margin (relative gap of the two smallest d2; ||d0| - 0.25|; |sk - s_end| and |sk - s[m]| at the samples
next to the end / a vertex; |frac(1000 x) - 0.5|).  A slot is `settled` when every margin exceeds 1e-9, `exact` when the margins
below that are 0 in rationals (the CPU test then shows that float64 evaluates them exactly), `open` otherwise: an open slot's
length may differ by one sample and its values are not compared.

Layouts are those of fo_scene_spawn_rule_agents: point records [type, x, y, orientation (NaN = derive), s, d, source, obstacle],
slot (i, r) = i R + r.  The covariance rows are written for every slot and sample (the kernels and the oracle do), everything
else behind `len` is zero."""
import math
from dataclasses import dataclass, field
from fractions import Fraction as Fr

import mpmath as mp
import numpy as np

mp.mp.dps = 60

TYPE_CAR, TYPE_BICYCLE, TYPE_PED = 0, 3, 4
SRC_LEFT, SRC_RIGHT = 3, 4
D1_TARGETS = (Fr(-1, 2), Fr(0), Fr(1, 2))
T1 = 3
SETTLED = 1e-9


def _m(x):
    return mp.mpf(x.numerator) / x.denominator if isinstance(x, Fr) else mp.mpf(x)


def _f(x):
    return float(x)          # Fraction and mpf both round to nearest


def _sqrt(x):
    """exact where the rational is a perfect square, 60 digits otherwise"""
    if isinstance(x, Fr):
        rn, rd = math.isqrt(x.numerator), math.isqrt(x.denominator)
        if rn * rn == x.numerator and rd * rd == x.denominator:
            return Fr(rn, rd)
    return mp.sqrt(_m(x))


def _mix(a, b, op):
    if isinstance(a, Fr) and isinstance(b, Fr):
        return op(a, b)
    return op(_m(a), _m(b))


def _add(a, b):
    return _mix(a, b, lambda p, q: p + q)


def _sub(a, b):
    return _mix(a, b, lambda p, q: p - q)


def _mul(a, b):
    return _mix(a, b, lambda p, q: p * q)


def _div(a, b):
    return _mix(a, b, lambda p, q: p / q)


@dataclass
class Scene:
    """the static map as the C ABI takes it: lanelet polygons, route table (R routes per lanelet), centre lines"""
    polys: list                      # P arrays [n, 2]
    R: int
    first: np.ndarray                # [P R]
    count: np.ndarray                # [P R]
    xy: np.ndarray                   # [NV, 2]
    s: np.ndarray                    # [NV]
    center_off: np.ndarray = None    # [P + 1] or None
    center_xy: np.ndarray = None
    _fr: dict = field(default_factory=dict, repr=False)

    def frac_poly(self, p):
        k = ("poly", p)
        if k not in self._fr:
            self._fr[k] = [(Fr(float(x)), Fr(float(y))) for x, y in self.polys[p]]
        return self._fr[k]

    def frac_route(self, ll, r):
        k = ("route", ll, r)
        if k not in self._fr:
            a, n = int(self.first[ll * self.R + r]), int(self.count[ll * self.R + r])
            self._fr[k] = (frac_curve(self.xy[a:a + n]), [Fr(float(v)) for v in self.s[a:a + n]], {})
        return self._fr[k]


class _Line(list):
    """vertices as Fractions; .fl: the float64 vertices they were made from"""


def frac_curve(c):
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1, 2)
    line = _Line((Fr(float(x)), Fr(float(y))) for x, y in c)
    line.fl = c
    return line


# ------------------------------------------------------------------------------------------------ decisions
def in_polygon(poly, x, y):
    """crossing number, half-open in y, behind the inclusive bounding box (the rule of the road raster)"""
    xs, ys = [p[0] for p in poly], [p[1] for p in poly]
    if x < min(xs) or x > max(xs) or y < min(ys) or y > max(ys):
        return False
    c, n = False, len(poly)
    for i in range(n):
        (xi, yi), (xj, yj) = poly[i], poly[i - 1]
        if (yi > y) != (yj > y) and x < xi + (y - yi) * (xj - xi) / (yj - yi):
            c = not c
    return c


def lanelet_of(scene, x, y):
    """first lanelet in list order that holds the point, -1 if none; also how many hold it"""
    hits = [p for p in range(len(scene.polys)) if in_polygon(scene.frac_poly(p), x, y)]
    return (hits[0] if hits else -1), hits


def closest_segment(q, px, py):
    """first minimum of the squared distance from (px, py) to the segments of the polyline q (Fractions).
    -> dict(seg, t, cx, cy, d2, gap (relative gap to the second smallest d2, inf for one segment), ties (indices at d2))"""
    d2s, feet = {}, {}
    cand = range(len(q) - 1)
    if len(q) > 9:
        # segments that cannot be the closest or the runner-up are left out by a float64 estimate with six orders of magnitude
        # to spare (its error is ~1e-10 of d2 at worst); among the rest the rationals decide
        a, e = q.fl[:-1], q.fl[1:] - q.fl[:-1]
        p = np.array([float(px), float(py)])
        t = np.clip(np.sum((p - a) * e, axis=1) / np.sum(e * e, axis=1), 0.0, 1.0)
        est = np.sum((a + t[:, None] * e - p) ** 2, axis=1)
        two = np.partition(est, 1)[1]
        cand = [int(i) for i in np.nonzero(est <= two * (1.0 + 1e-6) + 1e-9)[0]]
    for i in cand:
        (ax, ay), (bx, by) = q[i], q[i + 1]
        ex, ey = bx - ax, by - ay
        l2 = ex * ex + ey * ey
        t = Fr(0)
        if l2 > 0:
            t = min(max(((px - ax) * ex + (py - ay) * ey) / l2, Fr(0)), Fr(1))
        cx, cy = ax + t * ex, ay + t * ey
        d2s[i] = (px - cx) ** 2 + (py - cy) ** 2
        feet[i] = (t, cx, cy)
    best = min(d2s.values())
    ties = [i for i in cand if d2s[i] == best]
    seg = ties[0]
    rest = [d2s[i] for i in cand if i != seg]
    if not rest:
        gap = math.inf
    else:
        second = min(rest)
        gap = float((second - best) / second) if second > 0 else 0.0
    t, cx, cy = feet[seg]
    same_foot = all(feet[i][1:] == (cx, cy) for i in ties)      # tied at one shared point (a vertex between two segments)
    return dict(seg=seg, t=t, cx=cx, cy=cy, d2=best, gap=gap, ties=ties, same_foot=same_foot)


def heading_to_curve(curve_fr, px, py):
    """unit normal from the point towards the closest point of the curve as an angle in [0, 2 pi); 0 on the curve.
    -> (yaw float64, decision dict)"""
    c = closest_segment(curve_fr, px, py)
    vx, vy = c["cx"] - px, c["cy"] - py
    if vx == 0 and vy == 0:
        return 0.0, c
    a = mp.atan2(_m(vy), _m(vx))
    if a < 0:
        a += 2 * mp.pi
    return _f(a), c


def nearest_target(d0):
    """nearest of {-0.5, 0, 0.5}, the first of equally near ones; margin = ||d0| - 0.25| (the only switch points)"""
    best = D1_TARGETS[0]
    for d1 in D1_TARGETS[1:]:
        if abs(_sub(d1, d0)) < abs(_sub(best, d0)):
            best = d1
    return best, abs(_sub(abs(d0), Fr(1, 4)))


def round3(p):
    """round(np.float64(p), 3): numpy's rint(1000 p) / 1000 in float64"""
    return float(np.rint(np.float64(p) * 1000.0) / 1000.0)


# ------------------------------------------------------------------------------------------------ values
_POW = {}


def variances(T, var0, factor):
    k = (T, var0, factor)
    if k not in _POW:
        f, v = _m(Fr(float(factor))), _m(Fr(float(var0)))
        _POW[k] = np.array([_f(v * mp.power(f, j)) for j in range(T)])
    return _POW[k]


_LAT = {}


def _lateral(diff, tk, spd):
    """quintic from d0 towards d1 = d0 + diff over T1 seconds at time tk: (fraction of the way, atan2(d', v), sqrt(v^2 + d'^2))"""
    key = (diff, tk, spd)
    if key not in _LAT:
        tau = min(tk / T1, Fr(1))
        w = tau ** 3 * (10 + tau * (-15 + 6 * tau))
        dd = _mul(diff, 30 * tau * tau * (1 + tau * (-2 + tau)) / T1)
        ddm, sm = _m(dd), _m(spd)
        _LAT[key] = (w, mp.atan2(ddm, sm), mp.sqrt(sm * sm + ddm * ddm))
    return _LAT[key]


def _status(margins, exact_ok):
    """settled / exact / open from the margins (name -> value) and whether the zero ones are rational zeros"""
    small = {k: v for k, v in margins.items() if not v > SETTLED}
    if not small:
        return "settled"
    if all(v == 0 and exact_ok.get(k, False) for k, v in small.items()):
        return "exact"
    return "open"


def straight(px, py, a, spd, T, dt):
    """constant velocity along heading a (float64): velocity components rounded to three decimals"""
    am = _m(Fr(a))
    cx, cy = _m(spd) * mp.cos(am), _m(spd) * mp.sin(am)
    margins = {}
    v = []
    for name, c in (("round_x", cx), ("round_y", cy)):
        fr = abs(c) * 1000 - mp.floor(abs(c) * 1000)
        margins[name] = float(abs(fr - mp.mpf(1) / 2))
        v.append(round3(_f(c)))
    vx, vy = Fr(v[0]), Fr(v[1])
    pos = np.zeros((T, 2))
    for k in range(T):
        tk = k * dt
        pos[k] = (_f(px + tk * vx), _f(py + tk * vy))
    return pos, np.full(T, a), np.full(T, _f(spd)), (v[0], v[1]), margins


def _straight_on(q, j, cache):
    """the route goes straight on at vertex j: which of the two segments a sample at the vertex is given to changes nothing"""
    if ("on", j) not in cache:
        ax, ay, bx, by = q[j][0] - q[j - 1][0], q[j][1] - q[j - 1][1], q[j + 1][0] - q[j][0], q[j + 1][1] - q[j][1]
        cache[("on", j)] = ax * by - ay * bx == 0 and ax * bx + ay * by > 0
    return cache[("on", j)]


def follow(route, px, py, spd, T, dt):
    """the reference's min-var(v) Frenet sample along a route (speed held, quintic lateral move over 3 s to the nearest of
    {-0.5, 0, 0.5}); ends where the route ends"""
    q, s, seg_cache = route           # (seg_cache: per-segment values shared by the slots that follow this route)
    nv = len(q)
    c = closest_segment(q, px, py)
    i = c["seg"]
    (ax, ay), (bx, by) = q[i], q[i + 1]
    ex, ey = bx - ax, by - ay
    l = _sqrt(ex * ex + ey * ey)
    s0 = _add(s[i], _mul(c["t"], l))
    d0 = _div((px - c["cx"]) * (-ey) + (py - c["cy"]) * ex, l)
    rational = isinstance(l, Fr)
    d1, m_d0 = nearest_target(d0)
    margins = {"d2": c["gap"], "d0": float(m_d0)}
    exact_ok = {"d2": True, "d0": rational}       # d2 is always rational
    s_end = s[-1]
    diff = _sub(d1, d0)
    pos, yaw, v = np.zeros((T, 2)), np.zeros(T), np.zeros(T)
    L, m = 0, 0
    m_end, m_vtx = math.inf, math.inf
    exact_k = []                                   # samples that sit exactly on the route's end or on a vertex where it turns
    for k in range(T):
        tk = k * dt
        sk = _add(s0, spd * tk)
        m_end = min(m_end, float(abs(_sub(sk, s_end))))
        if _sub(sk, s_end) == 0:
            exact_k.append(k)
        if _sub(sk, s_end) > 0:
            break                                  # sk does not decrease with k: the samples on the route are a prefix
        while m + 2 < nv and _sub(s[m + 1], sk) <= 0:       # largest m <= nv - 2 with s[m] <= sk
            m += 1
        for j in (m, m + 1):                       # interior vertices next to the sample
            if 1 <= j <= nv - 2 and not _straight_on(q, j, seg_cache):
                m_vtx = min(m_vtx, float(abs(_sub(sk, s[j]))))
                if _sub(sk, s[j]) == 0:
                    exact_k.append(k)
        if m not in seg_cache:
            (x0, y0), (x1, y1) = q[m], q[m + 1]
            fx, fy = x1 - x0, y1 - y0
            lm = _m(_sqrt(fx * fx + fy * fy))
            seg_cache[m] = (_m(x0), _m(y0), _m(fx) / lm, _m(fy) / lm, mp.atan2(_m(fy), _m(fx)))
        x0, y0, ux, uy, ang = seg_cache[m]
        w, dyaw, vk = _lateral(diff, tk, spd)
        dk = _m(d0) + _m(diff) * _m(w)
        loc = _m(_sub(sk, s[m]))
        pos[k] = (_f(x0 + loc * ux - dk * uy), _f(y0 + loc * uy + dk * ux))
        yaw[k] = _f(ang + dyaw)
        v[k] = _f(vk)
        L = k + 1
    margins["end"], margins["vertex"] = m_end, m_vtx
    exact_ok["end"] = exact_ok["vertex"] = rational
    dec = dict(seg=i, d1=float(d1), ties=c["ties"], d2=c["d2"], s0=s0, d0=d0, rational=rational, margins=margins, exact_ok=exact_ok,
               exact_k=exact_k, nv=nv)
    return pos, yaw, v, L, dec


# ------------------------------------------------------------------------------------------------ the stage
def predict(scene, points, n_points, path, T, dt, var0, factor, speed, raw_l, raw_w, infl_l, infl_w, routes=None, entry="rules",
            lanelets=None):
    """what fo_scene_spawn_rule_agents writes for the records `points` [max_points, 8] of which *d_n_points = n_points are live
    (entry "rules"), or what fo_scene_spawn writes for cell centres (entry "cells": records carry type, x, y only; `lanelets`
    = the lanelet raster's value at each cell; every heading comes from the path, i.e. a map without a heading raster).
    speed .. infl_w: per type 0 Car, 1 Bicycle, 2 Pedestrian.  -> dict of arrays + per-slot decisions"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 8)
    mp_, RT = len(points), (scene.R if routes is None else routes)
    R = RT if RT > 0 else 1
    n = min(max(int(n_points), 0), mp_)
    S = mp_ * R
    out = dict(pos=np.zeros((S, T, 2)), yaw=np.zeros((S, T)), v=np.zeros((S, T)), cov=np.zeros((S, T, 4)),
               len=np.zeros(S, dtype=np.int32), type=np.zeros(S, dtype=np.int32), shape=np.zeros((S, 2)), raw=np.zeros((S, 2)),
               pos0=np.zeros((mp_, 2)), yaw0=np.zeros(mp_), lanelet=np.full(mp_, -1, dtype=np.int32), dec=[None] * S,
               status=["settled"] * S, heading_dec=[None] * mp_, center_lanelet=np.full(mp_, -1, dtype=np.int32))
    var = variances(T, var0, factor)
    out["cov"][:, :, 0] = var
    out["cov"][:, :, 3] = var
    path_fr = frac_curve(path)
    dtf = Fr(float(dt))
    for i in range(mp_):
        on = i < n
        rec = points[i]
        typ = int(rec[0]) if (on or entry == "cells") else TYPE_PED      # (the cell sampler's slot j has the pattern's type j % 4)
        ti = 0 if typ == TYPE_CAR else 1 if typ == TYPE_BICYCLE else 2
        sl = slice(i * R, (i + 1) * R)
        out["type"][sl] = typ
        out["shape"][sl] = (infl_l[ti], infl_w[ti])
        out["raw"][sl] = (raw_l[ti], raw_w[ti])
        if not on:
            continue
        px, py = Fr(float(rec[1])), Fr(float(rec[2]))
        spd = Fr(float(speed[ti]))
        a0, ll, hdec = float(rec[3]), -1, None
        if entry == "cells":
            a0, hdec = heading_to_curve(path_fr, px, py)
            if ti != 2 and RT > 0:
                ll = int(lanelets[i])
            routed = ll >= 0 and scene.count[ll * scene.R] > 0
        elif ti == 2:
            if a0 != a0:
                curve = path_fr
                if int(rec[6]) in (SRC_LEFT, SRC_RIGHT) and scene.center_off is not None:      # mode 'lane_center'
                    lc, _ = lanelet_of(scene, px, py)
                    out["center_lanelet"][i] = lc
                    if lc >= 0 and scene.center_off[lc + 1] - scene.center_off[lc] >= 2:
                        curve = frac_curve(scene.center_xy[scene.center_off[lc]:scene.center_off[lc + 1]])
                a0, hdec = heading_to_curve(curve, px, py)
            routed = False
        else:
            ll = lanelet_of(scene, px, py)[0] if RT > 0 else -1
            if ll >= 0 and scene.count[ll * scene.R] >= 2:
                q = scene.frac_route(ll, 0)[0]
                a0 = _f(mp.atan2(_m(q[1][1] - q[0][1]), _m(q[1][0] - q[0][0])))
            else:
                ll = -1
                a0, hdec = heading_to_curve(path_fr, px, py)
            routed = ll >= 0
        out["pos0"][i], out["yaw0"][i], out["lanelet"][i], out["heading_dec"][i] = (float(rec[1]), float(rec[2])), a0, ll, hdec
        for r in range(R):
            slot = i * R + r
            if not routed:
                if r > 0:
                    continue
                pos, yaw, v, vxy, margins = straight(px, py, a0, spd, T, dtf)
                if hdec is not None:
                    margins["d2"] = hdec["gap"]
                out["pos"][slot], out["yaw"][slot], out["v"][slot], out["len"][slot] = pos, yaw, v, T
                out["dec"][slot] = dict(form="straight", vxy=vxy, margins=margins, exact_ok={"d2": True},
                                        ties=hdec["ties"] if hdec else [], seg=hdec["seg"] if hdec else -1)
                # (the heading sees the closest POINT only: segments tied at one shared vertex give the same heading)
                if hdec is not None and len(hdec["ties"]) > 1 and hdec["same_foot"]:
                    margins["d2"] = math.inf
            elif r < scene.R and scene.count[ll * scene.R + r] >= 2:
                pos, yaw, v, L, dec = follow(scene.frac_route(ll, r), px, py, spd, T, dtf)
                out["pos"][slot], out["yaw"][slot], out["v"][slot], out["len"][slot] = pos, yaw, v, L
                dec["form"] = "route"
                out["dec"][slot] = dec
            else:
                continue
            d = out["dec"][slot]
            out["status"][slot] = _status(d["margins"], d["exact_ok"])
    return out

