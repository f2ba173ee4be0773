"""Plain-Python statement of the hidden-traffic brake clearance by road users (DESIGN.md §5.10 "Brake clearance by road users",
include/fo_hip.h fo_scene_hidden_brake_users), written from its definition -- not from the product code, and not by calling the
classes checker row by row.

What it takes from the checkers it stands on are the statements the definition itself refers to: the manoeuvre (speed profile, stop
sample, re-sampled poses, heading rule) is tests/ref_hidden_brake.py's, the key of a world-raster cell -- the map inside the window,
0 on raster road and NONE elsewhere outside it -- is tests/ref_hidden_clearance.py's ``key_at``, the footprint test
tests/ref_hidden_reach.py's ``in_rectangle`` on the cells of a square that holds the whole rectangle.  The key maps, the qmin arrays,
``heading``, ``arc``, ``v``, the threshold table and ``map_of`` are taken as data.  Every class walks every manoeuvre for itself,
sample by sample, up to its first hit on ITS map: no shortcut for a standing ego, none across classes or maps.  The one economy: the
cells under a pose are found once per pose VALUE; the minimum over them is taken per map."""
import math

import numpy as np

import ref_hidden_brake as B
import ref_hidden_clearance as HC
import ref_hidden_reach as HR

NONE = HC.NONE
MAX_MAPS, MAX_CLASSES, MAX_TABLE = 3, 8, 896


class Footprint:
    """the world-raster cells under a pose, and per map the minimum of its key over them (NONE = no cell)"""

    def __init__(self, keys, win, road, origin, cs, hl, hw, wb):
        self.keys, self.win, self.road, self.origin, self.cs = [np.asarray(k) for k in keys], win, road, origin, cs
        self.hl, self.hw, self.wb = hl, hw, wb
        n = int(math.ceil((hl + hw) / cs)) + 2
        OX, OY = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1))
        self.OX, self.OY = OX.ravel(), OY.ravel()
        self.seen = {}
        self.scans = 0

    def min_keys(self, xn, yn, c, s):
        """[K] ints"""
        at = (xn, yn, c, s)
        if at in self.seen:
            return self.seen[at]
        cx, cy = xn + self.wb * c, yn + self.wb * s
        out = [NONE] * len(self.keys)
        if math.isfinite(cx) and math.isfinite(cy):
            self.scans += 1
            gx = int(math.floor((cx - self.origin[0]) / self.cs)) + self.OX
            gy = int(math.floor((cy - self.origin[1]) / self.cs)) + self.OY
            inside = HR.in_rectangle(gx, gy, self.origin, self.cs, np.float64(xn), np.float64(yn), np.float64(c), np.float64(s),
                                     self.hl, self.hw, self.wb)
            if inside.any():
                out = [int(HC.key_at(k, self.win, self.road, gx[inside], gy[inside]).min()) for k in self.keys]
        if at[0] == at[0] and at[1] == at[1]:      # (a NaN never equals itself: such an entry would never be found again)
            self.seen[at] = out
        return out


def brake_users(keys, win, road, qmins, origin, cs, x, y, heading, arc, v, hl, hw, wb, a_brake, dt, thr, map_of, lens=None, stats=None):
    """(brake_first [C, M, T], stop [M, T], commit [C, M], first [C, M]) int32.  ``keys``: K maps [ny, nx]; ``qmins``: K arrays [M, T];
    ``thr [C, T]``; ``map_of [C]`` in [0, K).  ``stats``: a dict that receives ``poses`` (poses a walk shared by the classes looks at:
    per manoeuvre the longest of the classes' walks), ``longest`` and ``scans``"""
    x, y, arc, v = (np.asarray(t, dtype=np.float64) for t in (x, y, arc, v))
    heading = np.asarray(heading, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.int64)
    qmins = [np.asarray(q, dtype=np.int64) for q in qmins]
    map_of = [int(k) for k in map_of]
    M, T = x.shape
    C, K = thr.shape[0], len(keys)
    assert 1 <= K <= MAX_MAPS and 1 <= C <= MAX_CLASSES and C * T <= MAX_TABLE and len(qmins) == K
    assert thr.shape == (C, T) and len(map_of) == C and all(0 <= k < K for k in map_of)
    a_brake, dt = float(a_brake), float(dt)
    fp = Footprint(keys, win, road, origin, cs, hl, hw, wb)
    brake_first = np.full((C, M, T), -1, dtype=np.int32)
    stop = np.full((M, T), -1, dtype=np.int32)
    commit = np.full((C, M), -1, dtype=np.int32)
    first = np.full((C, M), -1, dtype=np.int32)
    poses = longest = 0
    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        for c in range(C):                                       # 5. first[c][m]
            q = qmins[map_of[c]]
            for j in range(Lm):
                if q[m, j] <= thr[c, j]:
                    first[c, m] = j
                    break
        xr, yr, ar, vr = x[m].tolist(), y[m].tolist(), arc[m].tolist(), v[m].tolist()
        hr = heading[m].tolist()
        for b in range(Lm):
            st = B.stop_sample(vr[b], a_brake, dt, b, Lm)        # 1. stop, the profile and the poses: neither class nor map in them
            stop[m, b] = st
            walk = list(B.manoeuvre(xr, yr, hr, ar, vr[b], Lm, b, a_brake, dt))
            looked = 0
            for c in range(C):
                bf = -1
                for n, (i, xn, yn, hc, hs, _, _) in enumerate(walk):
                    looked = max(looked, n + 1)
                    if fp.min_keys(xn, yn, hc, hs)[map_of[c]] <= thr[c, i]:      # 2. q_k(i), 3. hit_c(i)
                        bf = i                                                   # 4. the first one
                        break
                brake_first[c, m, b] = bf
                fm = int(first[c, m])
                if commit[c, m] < 0 and ((0 <= fm <= b) or (0 <= bf < st)):      # 6.
                    commit[c, m] = b
            poses += looked
            longest = max(longest, looked)
    if stats is not None:
        stats.update(poses=poses, longest=longest, scans=fp.scans)
    return brake_first, stop, commit, first
