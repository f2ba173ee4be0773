"""Plain-Python statement of the hidden-traffic brake clearance by classes (DESIGN.md §5.10 "Brake clearance by classes",
include/fo_hip.h fo_scene_hidden_brake_classes), written from its definition -- not from the product code.

Built on what the two checkers it joins already state: the manoeuvre (speed profile, stop sample, re-sampled poses, heading rule)
is tests/ref_hidden_brake.py's, the key of a world-raster cell -- the map inside the window, 0 on raster road and NONE elsewhere
outside it -- is tests/ref_hidden_clearance.py's ``key_at``, the footprint test tests/ref_hidden_reach.py's ``in_rectangle`` on
the cells of a square that holds the whole rectangle.  ``key``, ``qmin``, ``heading``, ``arc``, ``v`` and the threshold table are
taken as data.  Every class walks every manoeuvre for itself, sample by sample, up to its first hit: no shortcut for a standing ego,
none across classes.  The one economy is ref_hidden_brake's: the smallest key under a pose is remembered per pose VALUE."""
import math

import numpy as np

import ref_hidden_brake as B
import ref_hidden_clearance as HC
import ref_hidden_reach as HR

NONE = HC.NONE


class Footprints:
    """min of key over the footprint cells of a pose (NONE = none), key extended beyond the window by the clearance's rule"""

    def __init__(self, key, win, road, origin, cs, hl, hw, wb):
        self.key, self.win, self.road, self.origin, self.cs = np.asarray(key), win, road, origin, cs
        self.hl, self.hw, self.wb = hl, hw, wb
        n = int(math.ceil((hl + hw) / cs)) + 2
        OX, OY = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1))
        self.OX, self.OY = OX.ravel(), OY.ravel()
        self.seen = {}
        self.scans = 0

    def min_key(self, xn, yn, c, s):
        k = (xn, yn, c, s)
        if k in self.seen:
            return self.seen[k]
        cx, cy = xn + self.wb * c, yn + self.wb * s
        out = NONE
        if math.isfinite(cx) and math.isfinite(cy):
            self.scans += 1
            gx = int(math.floor((cx - self.origin[0]) / self.cs)) + self.OX
            gy = int(math.floor((cy - self.origin[1]) / self.cs)) + self.OY
            inside = HR.in_rectangle(gx, gy, self.origin, self.cs, np.float64(xn), np.float64(yn), np.float64(c), np.float64(s),
                                     self.hl, self.hw, self.wb)
            if inside.any():
                out = int(HC.key_at(self.key, self.win, self.road, gx[inside], gy[inside]).min())
        if k[0] == k[0] and k[1] == k[1]:          # (a NaN never equals itself: such a key would never be found again)
            self.seen[k] = out
        return out


def first_from_qmin(qmin, thr, lens=None):
    """first [C, M]: min { k < Lm : qmin[m][k] <= thr[c][k] }, -1 = none"""
    qmin, thr = np.asarray(qmin, dtype=np.int64), np.asarray(thr, dtype=np.int64)
    M, T = qmin.shape
    first = np.full((thr.shape[0], M), -1, dtype=np.int32)
    for c in range(thr.shape[0]):
        for m in range(M):
            for k in range(B.clip_len(T, lens, m)):
                if qmin[m, k] <= thr[c, k]:
                    first[c, m] = k
                    break
    return first


def brake_classes(key, win, road, qmin, origin, cs, x, y, heading, arc, v, hl, hw, wb, a_brake, dt, thr, lens=None, stats=None):
    """(brake_first [C, M, T], stop [M, T], commit [C, M], first [C, M]) int32.  ``stats``: a dict that receives ``poses`` (poses a
    walk shared by the classes looks at: per manoeuvre the longest of the classes' walks) and ``longest``"""
    x, y, arc, v = (np.asarray(t, dtype=np.float64) for t in (x, y, arc, v))
    heading = np.asarray(heading, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.int64)
    M, T = x.shape
    C = thr.shape[0]
    assert thr.shape == (C, T)
    a_brake, dt = float(a_brake), float(dt)
    fp = Footprints(key, win, road, origin, cs, hl, hw, wb)
    first = first_from_qmin(qmin, thr, lens)
    brake_first = np.full((C, M, T), -1, dtype=np.int32)
    stop = np.full((M, T), -1, dtype=np.int32)
    commit = np.full((C, M), -1, dtype=np.int32)
    poses = longest = 0
    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        xr, yr, ar, vr = x[m].tolist(), y[m].tolist(), arc[m].tolist(), v[m].tolist()
        hr = heading[m].tolist()
        for b in range(Lm):
            st = B.stop_sample(vr[b], a_brake, dt, b, Lm)
            stop[m, b] = st
            walk = list(B.manoeuvre(xr, yr, hr, ar, vr[b], Lm, b, a_brake, dt))
            looked = 0
            for c in range(C):
                bf = -1
                for n, (i, xn, yn, hc, hs, _, _) in enumerate(walk):
                    looked = max(looked, n + 1)
                    if fp.min_key(xn, yn, hc, hs) <= thr[c, i]:
                        bf = i
                        break
                brake_first[c, m, b] = bf
                fm = int(first[c, m])
                if commit[c, m] < 0 and ((0 <= fm <= b) or (0 <= bf < st)):
                    commit[c, m] = b
            poses += looked
            longest = max(longest, looked)
    if stats is not None:
        stats.update(poses=poses, longest=longest, scans=fp.scans)
    return brake_first, stop, commit, first
