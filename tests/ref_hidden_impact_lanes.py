"""Plain-Python statement of the hidden-traffic impact verdict by approach angle (DESIGN.md §5.10 "Impact verdict by approach angle",
include/fo_hip.h fo_scene_hidden_brake_impact_lanes), written from its definition -- not from the product code.

The walk is the users entry's, taken whole as in tests/ref_hidden_impact.py: the stage is defined on what fo_scene_hidden_brake_users
writes (``brake_first``, ``stop``, ``first``) and on ``v``.  What is stated here is steps 2 - 5: the hit pose (the manoeuvre is
tests/ref_hidden_brake.py's), its hit cells (the footprint test tests/ref_hidden_reach.py's ``in_rectangle``, the key of a cell
tests/ref_hidden_clearance.py's ``key_at``), the OR of their move bytes, the approach cosine, the closing speed and the reductions --
plain loops over Python floats (IEEE float64) in the definition's operation order.  Steps 4 - 6 of the head-on stage (the logistics, the
choice of the user, the fail-closed row) are tests/ref_hidden_impact.py's, on the closing speed."""
import math

import numpy as np

import ref_hidden_brake as B
import ref_hidden_clearance as HC
import ref_hidden_impact as RI
import ref_hidden_reach as HR

ANY = 0xFF
R = math.sqrt(0.5)
LATTICE = ((1.0, 0.0), (R, R), (0.0, 1.0), (-R, R), (-1.0, 0.0), (-R, -R), (0.0, -1.0), (R, -R))     # the unit vector of direction k
BASE = math.pi / 8.0                                                                                # 22.5 degrees


def central(byte):
    """the directions k whose bits k - 1, k, k + 1 (mod 8) are all set"""
    return [k for k in range(8) if all(byte >> ((k + d) % 8) & 1 for d in (-1, 0, 1))]


def host_h(heading_slack):
    """(cos_h, sin_h) as the host hands them over: of h = 22.5 deg + heading_slack; (-1, 0) states h >= pi"""
    h = BASE + float(heading_slack)
    return (math.cos(h), math.sin(h)) if h < math.pi else (-1.0, 0.0)


def cosine(byte, bound, ct, st, cos_h, sin_h):
    """step 3: the greatest cos(pdof) the byte allows a class at a hit pose of unit heading (ct, st)"""
    ks = central(byte)
    if not bound or not ks or not cos_h > -1.0:
        return 1.0
    cm = None
    for k in ks:
        ck, sk = LATTICE[k]
        g = -(ct * ck + st * sk)
        c = 1.0 if g >= cos_h else g * cos_h + math.sqrt(B.fmax(0.0, 1.0 - g * g)) * sin_h
        if cm is None or c > cm:
            cm = c
    return cm


def closing(u, s, cm):
    """step 4"""
    if cm == 1.0:
        return u + s
    return math.sqrt(B.fmax(0.0, u * u + s * s + 2.0 * u * s * cm))


class HitCells:
    """step 2: the OR of the move bytes of the hit cells of a pose against one key map and one threshold"""

    def __init__(self, keys, win, road, moves, origin, cs, hl, hw, wb):
        self.keys, self.win, self.road, self.moves = [np.asarray(k) for k in keys], win, np.asarray(road), moves
        self.origin, self.cs, self.hl, self.hw, self.wb = origin, cs, hl, hw, wb
        n = int(math.ceil((hl + hw) / cs)) + 2
        OX, OY = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1))
        self.OX, self.OY = OX.ravel(), OY.ravel()

    def moves_or(self, xn, yn, c, s, k, thr):
        cx, cy = xn + self.wb * c, yn + self.wb * s
        if not (math.isfinite(cx) and math.isfinite(cy)):
            return 0
        gx = int(math.floor((cx - self.origin[0]) / self.cs)) + self.OX
        gy = int(math.floor((cy - self.origin[1]) / self.cs)) + self.OY
        inside = HR.in_rectangle(gx, gy, self.origin, self.cs, np.float64(xn), np.float64(yn), np.float64(c), np.float64(s),
                                 self.hl, self.hw, self.wb)
        gx, gy = gx[inside], gy[inside]
        hit = HC.key_at(self.keys[k], self.win, self.road, gx, gy) <= thr
        out = 0
        rny, rnx = self.road.shape
        for px, py in zip(gx[hit].tolist(), gy[hit].tolist()):
            out |= int(self.moves[py, px]) if 0 <= px < rnx and 0 <= py < rny else ANY
        return out


def impact_lanes(keys, win, road, moves, origin, cs, x, y, heading, arc, v, hl, hw, wb, a_brake, dt, thr, map_of, B_, rows, speed_of, dir_mask,
                 cos_h, sin_h, brake_first, stop, first, lens=None, finite=None):
    """steps 1 - 6 over what fo_scene_hidden_brake_users wrote: (harm [M, 2], user [M], closing [C, M], at [C, M], cosine [C, M], open
    choices of the user, the closing speeds of every (c, m) by start: a list of lists, for the open-choice condition)"""
    x, y, arc, v = (np.asarray(t, dtype=np.float64) for t in (x, y, arc, v))
    heading, thr = np.asarray(heading, dtype=np.float64), np.asarray(thr, dtype=np.int64)
    brake_first, stop, first = np.asarray(brake_first), np.asarray(stop), np.asarray(first)
    C, M, T = brake_first.shape
    a_brake, dt = float(a_brake), float(dt)
    cells = HitCells(keys, win, road, moves, origin, cs, hl, hw, wb) if dir_mask else None
    harm, user = np.zeros((M, 2)), np.full(M, -1, dtype=np.int32)
    clos, at, cosn = np.zeros((C, M)), np.full((C, M), -1, dtype=np.int32), np.ones((C, M))
    n_open, by_start = 0, []
    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        ends = min(int(B_), Lm)
        xr, yr, ar, vr, hr = x[m].tolist(), y[m].tolist(), arc[m].tolist(), v[m].tolist(), heading[m].tolist()
        walks = {}
        for c in range(C):
            bound = bool(dir_mask >> c & 1)
            fm = int(first[c, m])
            best, best_at, best_cm, ws = -math.inf, -1, 1.0, []
            for b in range(ends):
                bf, st = int(brake_first[c, m, b]), int(stop[m, b])
                met = 0 <= fm <= b
                if not (met or 0 <= bf < st):                                           # 1.
                    continue
                if met:                                                                 # 2. the hit pose, its sample and the speed
                    i, pose, u = fm, (xr[fm], yr[fm], hr[fm][0], hr[fm][1]), vr[fm]
                else:
                    if b not in walks:
                        walks[b] = {p[0]: p[1:5] for p in B.manoeuvre(xr, yr, hr, ar, vr[b], Lm, b, a_brake, dt)}
                    i, pose = bf, walks[b][bf]
                    u = B.fmax(vr[b] - a_brake * (float(bf - b) * dt), 0.0)
                byte = cells.moves_or(*pose, int(map_of[c]), int(thr[c, i])) if bound else 0
                cm = cosine(byte, bound, pose[2], pose[3], cos_h, sin_h)                # 3.
                w = closing(u, float(speed_of[c]), cm)                                  # 4.
                ws.append(w)
                if w > best:                                                            # 5.: ascending b, the lowest start stays
                    best, best_at, best_cm = w, b, cm
            by_start.append(ws)
            if best_at >= 0:
                clos[c, m], at[c, m], cosn[c, m] = best, best_at, best_cm
        zero = [0.0] * C
        ho, he, user[m], is_open = RI.choose(clos[:, m].tolist(), at[:, m].tolist(), rows, zero, True if finite is None else bool(finite[m]))
        harm[m] = (ho, he)
        n_open += bool(is_open)
    return harm, user, clos, at, cosn, n_open, by_start


def ulps_apart(a, b):
    """the number of float64 values between two finite non-negative numbers"""
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(ia) - int(ib))


def close_starts(by_start, ulps=4):
    """the open-choice condition on the starts: pairs of closing speeds of one (class, trajectory) that are within ``ulps`` of each other
    and are not the same number"""
    n = 0
    for ws in by_start:
        vals = sorted(set(w for w in ws if w == w))
        n += sum(1 for a, b in zip(vals, vals[1:]) if ulps_apart(a, b) <= ulps)
    return n
