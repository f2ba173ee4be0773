"""Plain-Python statement of the hidden-traffic harm ladder by approach angle (DESIGN.md §5.10 "Harm ladder by approach angle",
include/fo_hip.h fo_scene_hidden_brake_harm_ladder_lanes), written from its definition -- not from the product code.

The walk is not restated: the stage is defined on what fo_scene_hidden_brake_ladder_users writes with its detail (``brake_first
[C, M, B, L]``, ``stop [M, B, L]``, ``first [C, M]``) and on ``v``.  What is stated here is step 3: per hit the hit pose (the
manoeuvre is tests/ref_hidden_brake.py's at ``a_brake = levels[l]``), the OR of the move bytes of its hit cells, the approach
cosine and the closing speed (tests/ref_hidden_impact_lanes.py's ``HitCells``, ``cosine``, ``closing``) and the logistic of the
class's row at that closing speed.  Steps 4 - 6 are tests/ref_hidden_brake_harm_ladder.py's ``reduce_one``."""
import math

import numpy as np

import ref_hidden_brake as B
import ref_hidden_brake_harm_ladder as RH
import ref_hidden_impact_lanes as RL


def harm_ladder_lanes(keys, win, road, moves, origin, cs, x, y, heading, arc, v, hl, hw, wb, levels, dt, thr, map_of, B_, rows, speed_of, dir_mask,
                      cos_h, sin_h, harm_limit, brake_first, stop, first, lens=None, finite=None):
    """steps 1 - 6: a dict of the nine outputs as tests/ref_hidden_brake_harm_ladder.harm_ladder returns them, ``hits`` and ``closest``
    for the open-choice condition, and ``ho [C, M, B, L]`` float64: the harm of every hit, NaN where (c, m, b, l) is no hit"""
    x, y, arc, v = (np.asarray(t, dtype=np.float64) for t in (x, y, arc, v))
    heading, thr = np.asarray(heading, dtype=np.float64), np.asarray(thr, dtype=np.int64)
    brake_first, stop, first = np.asarray(brake_first), np.asarray(stop), np.asarray(first)
    C, M = first.shape
    T, L, dt = v.shape[1], len(levels), float(dt)
    cells = RL.HitCells(keys, win, road, moves, origin, cs, hl, hw, wb) if dir_mask else None
    out = dict(need=np.empty(M, np.int32), at=np.empty(M, np.int32), blocking=np.empty(M, np.int32), user=np.empty(M, np.int32),
               decel=np.empty(M, np.float64), need_of=np.empty((C, M), np.int32), first=np.array(first, dtype=np.int32).reshape(C, M),
               harm_at=np.empty((M, L), np.float64), user_at=np.empty((M, L), np.int32))
    all_ho = np.full((C, M, int(B_), L), math.nan)
    hits, closest = [], math.inf

    def price(c, pose, i, u):
        bound = bool(dir_mask >> c & 1)
        byte = cells.moves_or(*pose, int(map_of[c]), int(thr[c, i])) if bound else 0
        cm = RL.cosine(byte, bound, pose[2], pose[3], cos_h, sin_h)
        w = RL.closing(u, float(speed_of[c]), cm)
        return RH.logistic(rows[c][0], rows[c][1], w)

    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        ends = min(int(B_), Lm)
        xr, yr, ar, vr, hr = x[m].tolist(), y[m].tolist(), arc[m].tolist(), v[m].tolist(), heading[m].tolist()
        met_ho = {}                                                                     # one harm per class: pose fm, speed v[fm]
        ho = [[[None] * L for _ in range(ends)] for _ in range(C)]
        for b in range(ends):
            for n in range(L):
                level, walk = float(levels[n]), None
                st = int(stop[m, b, n])
                for c in range(C):
                    fm, bf = int(first[c, m]), int(brake_first[c, m, b, n])
                    met = 0 <= fm <= b
                    if not (met or 0 <= bf < st):                                       # 1.
                        continue
                    if met:
                        if c not in met_ho:
                            met_ho[c] = price(c, (xr[fm], yr[fm], hr[fm][0], hr[fm][1]), fm, vr[fm])
                        h = met_ho[c]
                    else:
                        if walk is None:
                            walk = {p[0]: p[1:5] for p in B.manoeuvre(xr, yr, hr, ar, vr[b], Lm, b, level, dt)}
                        h = price(c, walk[bf], bf, B.fmax(vr[b] - level * (float(bf - b) * dt), 0.0))     # 2., 3.
                    ho[c][b][n] = h
                    all_ho[c, m, b, n] = h
        fin = True if finite is None else bool(finite[m])
        got = RH.reduce_one(ho, list(levels), ends, float(harm_limit), fin)             # 4. - 6.
        out["need"][m], out["at"][m], out["blocking"][m], out["user"][m], out["decel"][m] = got[:5]
        out["need_of"][:, m], out["harm_at"][m], out["user_at"][m] = got[5], got[6], got[7]
        if fin:
            hits += got[8]
            for n in range(L):
                tops = sorted({got[9][c][n] for c in range(C) if got[9][c][n] >= 0.0})
                closest = min([closest] + [b - a for a, b in zip(tops, tops[1:])])
    out["hits"], out["closest"], out["ho"] = hits, closest, all_ho
    return out
