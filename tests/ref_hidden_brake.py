"""Plain-Python statement of the hidden-traffic brake clearance (DESIGN.md §5.10 "Brake clearance", include/fo_hip.h
fo_scene_hidden_brake), written from its definition -- not from the product code.

Loops over Python floats (IEEE float64) in the definition's operation order, a linear scan from the left for the segment index, no
shortcut for a standing ego.  ``A``, ``first``, ``heading``, ``arc`` and ``v`` are taken as data.  The footprint test is
tests/ref_hidden_reach.py's ``in_rectangle`` on the cells of a square that holds the whole rectangle, the rule outside the window
its ``arrival_at``.  The one economy: the smallest arrival step under a pose is remembered per pose VALUE (x, y, c, s), so a pose
that repeats -- a standing ego, the clamp at the end of the path -- is scanned once."""
import math

import numpy as np

import ref_hidden_reach as HR

NEVER = HR.NEVER


def fmax(a, b):
    """C's fmax: the operand that is no NaN"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def clip_len(T, lens, m):
    if lens is None:
        return T
    return min(max(int(lens[m]), 0), T)


def speed(vb, a_brake, dt, i, b):
    """vn(i) = fmax(v[b] - a_brake * ((double)(i - b) * dt), 0.0)"""
    return fmax(vb - a_brake * (float(i - b) * dt), 0.0)


def stop_sample(vb, a_brake, dt, b, Lm):
    for i in range(b, Lm):
        if speed(vb, a_brake, dt, i, b) == 0.0:
            return i
    return Lm


def manoeuvre(x, y, heading, arc, vb, Lm, b, a_brake, dt):
    """the poses of "follow until b, then brake" of ONE trajectory (rows of Python floats / [T][2] headings), one after the
    other: (i, xn, yn, c, s, idx, s_clamped) for i = b + 1 .. Lm - 1"""
    if b + 1 >= Lm:
        return
    s = arc[b]
    for i in range(b + 1, Lm):
        s = s + speed(vb, a_brake, dt, i - 1, b) * dt
        sc = fmin(s, arc[Lm - 1])
        j = Lm
        for t in range(Lm):
            if arc[t] >= sc:
                j = t
                break
        idx = min(max(j, 1), Lm - 1)
        xlo, xhi = arc[idx - 1], arc[idx]
        if xhi != xlo:
            w = sc - xlo
            inv = xhi - xlo
            xn = (x[idx] - x[idx - 1]) / inv * w + x[idx - 1]
            yn = (y[idx] - y[idx - 1]) / inv * w + y[idx - 1]
            h = idx - 1 if w + w <= inv else idx
        else:
            xn, yn = x[idx - 1], y[idx - 1]
            h = idx - 1
        yield i, xn, yn, heading[h][0], heading[h][1], idx, sc


class Footprints:
    """min of A over the footprint cells of a pose (255 = none), A extended beyond the window by the forecast's rule"""

    def __init__(self, A, win, road, origin, cs, hl, hw, wb):
        self.A, self.win, self.road, self.origin, self.cs = np.asarray(A), win, road, origin, cs
        self.hl, self.hw, self.wb = hl, hw, wb
        n = int(math.ceil((hl + hw) / cs)) + 2
        OX, OY = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1))
        self.OX, self.OY = OX.ravel(), OY.ravel()
        self.seen = {}
        self.scans = 0

    def min_arrival(self, xn, yn, c, s):
        key = (xn, yn, c, s)
        if key in self.seen:
            return self.seen[key]
        cx, cy = xn + self.wb * c, yn + self.wb * s
        out = NEVER
        if math.isfinite(cx) and math.isfinite(cy):
            self.scans += 1
            gx = int(math.floor((cx - self.origin[0]) / self.cs)) + self.OX
            gy = int(math.floor((cy - self.origin[1]) / self.cs)) + self.OY
            inside = HR.in_rectangle(gx, gy, self.origin, self.cs, np.float64(xn), np.float64(yn), np.float64(c), np.float64(s),
                                     self.hl, self.hw, self.wb)
            if inside.any():
                out = int(HR.arrival_at(self.A, self.win, self.road, gx[inside], gy[inside]).min())
        if key[0] == key[0] and key[1] == key[1]:      # (a NaN never equals itself: such a key would never be found again)
            self.seen[key] = out
        return out


def brake(A, win, road, first, origin, cs, x, y, heading, arc, v, hl, hw, wb, a_brake, dt, lens=None, stats=None):
    """(brake_first [M, T], stop [M, T], commit [M]) int32.  ``stats``: a dict that receives ``after_stop`` (manoeuvres whose first
    hit lies strictly after their stop), ``poses`` (manoeuvre poses looked at before the first hit) and ``longest``"""
    x, y, arc, v = (np.asarray(t, dtype=np.float64) for t in (x, y, arc, v))
    heading = np.asarray(heading, dtype=np.float64)
    M, T = x.shape
    a_brake, dt = float(a_brake), float(dt)
    fp = Footprints(A, win, road, origin, cs, hl, hw, wb)
    brake_first = np.full((M, T), -1, dtype=np.int32)
    stop = np.full((M, T), -1, dtype=np.int32)
    commit = np.full(M, -1, dtype=np.int32)
    after_stop = poses = longest = 0
    for m in range(M):
        Lm = clip_len(T, lens, m)
        xr, yr, ar, vr = x[m].tolist(), y[m].tolist(), arc[m].tolist(), v[m].tolist()
        hr = heading[m].tolist()
        fm = int(first[m])
        for b in range(Lm):
            st = stop_sample(vr[b], a_brake, dt, b, Lm)
            stop[m, b] = st
            bf = -1
            for n, (i, xn, yn, c, s, _, _) in enumerate(manoeuvre(xr, yr, hr, ar, vr[b], Lm, b, a_brake, dt)):
                poses += 1
                if fp.min_arrival(xn, yn, c, s) <= i:
                    bf = i
                    longest = max(longest, n + 1)
                    break
            brake_first[m, b] = bf
            after_stop += bf > st
            if commit[m] < 0 and ((0 <= fm <= b) or (0 <= bf < st)):
                commit[m] = b
    if stats is not None:
        stats.update(after_stop=after_stop, poses=poses, longest=longest, scans=fp.scans)
    return brake_first, stop, commit
