"""Plain-Python statement of the hidden-traffic harm ladder (DESIGN.md §5.10 "Harm ladder", include/fo_hip.h
fo_scene_hidden_brake_harm_ladder), written from its definition -- not from the product code.  The walk is not restated: the stage is
defined on what fo_scene_hidden_brake_ladder_users writes as ``brake_first [C, M, B, L]``, ``stop [M, B, L]`` and ``first [C, M]`` (from
the device with its detail, or from tests/ref_hidden_brake_ladder_users.py) and on ``v``.  What is stated here is steps 1 - 6 -- plain
loops over lists -- and what a test may rest on: the harms of all hits and the closest pair of class maxima."""
import math

import numpy as np

NOT_FINITE = -2
C_SAFE, C_RES0, C_RES1, NC = 12, 14, 15, 16      # FO_C_SAFE, FO_C_RES0, FO_C_RES1, FO_NC (include/fo_hip.h)
OPEN_TOL = 1e-9                                  # the float tolerance of the harm values: a comparison between closer ones is open
OUTPUTS = ("need", "at", "blocking", "user", "decel", "need_of", "first", "harm_at", "user_at")
SHARED = OUTPUTS[:7]                             # those the ladder verdict has too


def logistic(p_const, p_speed, w):
    return 1.0 / (1.0 + math.exp(p_const + p_speed * w))


def harm_of_hit(fm, b, bf, st, v_row, level, dt, row, speed_of):
    """steps 1 - 3 for one (class, brake start, level): the obstacle harm of the hit, None without a hit"""
    met = 0 <= fm <= b
    if not (met or 0 <= bf < st):                                                       # 1.
        return None
    left = float(v_row[b]) - level * ((bf - b) * dt)
    u = float(v_row[fm]) if met else (left if left > 0.0 else 0.0)                      # 2. (a NaN speed: fmax's 0)
    return logistic(row[0], row[1], u + speed_of)                                       # 3.


def first_not(flags):
    """the lowest index whose flag is not set, -1 if every one is"""
    return next((n for n, f in enumerate(flags) if not f), -1)


def reduce_one(ho, levels, ends, harm_limit, finite=True):
    """steps 4 - 6 for one trajectory from the harms of its hits: ``ho [C][B][L]``, None where (c, b, l) is no hit -> (need, at,
    blocking, user, decel, need_of [C], harm_at [L], user_at [L], the harms of all hits, the class maxima per level)"""
    C, L = len(ho), len(levels)
    need, at, blocking = -1, -1, 0
    need_of = [-1] * C
    best = [[-1.0] * L for _ in range(C)]          # per class and level the greatest harm of a hit (compared by > from below)
    hits = []
    for b in range(ends):
        over = [[False] * L for _ in range(C)]
        for n in range(L):
            for c in range(C):
                h = ho[c][b][n]
                if h is None:
                    continue
                hits.append(h)
                over[c][n] = h > harm_limit                                             # 4. (a NaN: False)
                if h > best[c][n]:
                    best[c][n] = h
        # 5.: the ladder-users entry's rules on `over`, then the ladder verdict's maxima over the brake starts (-1 counts as L)
        req = [first_not(over[c]) for c in range(C)]
        ra = first_not([any(over[c][n] for c in range(C)) for n in range(L)])
        lvl = L - 1 if ra < 0 else ra - 1
        blk = 0 if lvl < 0 else sum(1 << c for c in range(C) if over[c][lvl])
        rank = ra if ra >= 0 else L
        if rank > need:                                                                 # (strictly: a tie stays with the first start)
            need, at, blocking = rank, b, blk
        need_of = [max(need_of[c], req[c] if req[c] >= 0 else L) for c in range(C)]
    user = next((c for c in range(C) if blocking >> c & 1), -1)
    decel = 0.0 if need < 0 else math.inf if need == L else float(levels[need])
    harm_at, user_at = [0.0] * L, [-1] * L
    for n in range(L):                                                                  # 6.
        top = -1.0
        for c in range(C):
            if best[c][n] > top:                                                        # (strictly: a tie stays with the lowest class)
                top, harm_at[n], user_at[n] = best[c][n], best[c][n], c
    if not finite:
        need, at, blocking, user, decel = L, 0, 0, NOT_FINITE, math.inf
        harm_at, user_at = [1.0] * L, [NOT_FINITE] * L
    return need, at, blocking, user, decel, need_of, harm_at, user_at, hits, best


def one(brake_first, stop, first, v_row, levels, dt, ends, rows, speed_of, harm_limit, finite=True):
    """steps 1 - 6 for one trajectory: ``brake_first [C][B][L]``, ``stop [B][L]``, ``first [C]`` as lists -> what reduce_one returns"""
    C, L = len(first), len(levels)
    ho = [[[harm_of_hit(int(first[c]), b, int(brake_first[c][b][n]), int(stop[b][n]), v_row, float(levels[n]), dt, rows[c], float(speed_of[c]))
            for n in range(L)] for b in range(ends)] for c in range(C)]
    return reduce_one(ho, levels, ends, harm_limit, finite)


def harm_ladder(brake_first, stop, first, v, levels, dt, B, rows, speed_of, harm_limit, lens=None, finite=None):
    """steps 1 - 6 over ``brake_first [C, M, >= B, L]``, ``stop [M, >= B, L]``, ``first [C, M]`` and ``v [M, T]``: a dict of the nine
    outputs (int32 / float64 as the entry writes them) and, for the conditions a test rests on, ``hits`` -- the harms of all hits of
    finite candidates -- and ``closest`` -- the smallest positive distance between two classes' maxima at one (m, l), inf if none"""
    brake_first, stop, first, v = np.asarray(brake_first), np.asarray(stop), np.asarray(first), np.asarray(v, dtype=np.float64)
    C, M = first.shape
    T, L = v.shape[1], len(levels)
    out = dict(need=np.empty(M, np.int32), at=np.empty(M, np.int32), blocking=np.empty(M, np.int32), user=np.empty(M, np.int32),
               decel=np.empty(M, np.float64), need_of=np.empty((C, M), np.int32), first=np.array(first, dtype=np.int32).reshape(C, M),
               harm_at=np.empty((M, L), np.float64), user_at=np.empty((M, L), np.int32))
    hits, closest = [], math.inf
    for m in range(M):
        Lm = T if lens is None else min(max(int(lens[m]), 0), T)
        fin = True if finite is None else bool(finite[m])
        got = one(brake_first[:, m].tolist(), stop[m].tolist(), first[:, m].tolist(), v[m].tolist(), list(levels), float(dt), min(int(B), Lm),
                  rows, speed_of, float(harm_limit), fin)
        out["need"][m], out["at"][m], out["blocking"][m], out["user"][m], out["decel"][m] = got[:5]
        out["need_of"][:, m], out["harm_at"][m], out["user_at"][m] = got[5], got[6], got[7]
        if fin:
            hits += got[8]
            for n in range(L):
                tops = sorted({got[9][c][n] for c in range(C) if got[9][c][n] >= 0.0})
                closest = min([closest] + [b - a for a, b in zip(tops, tops[1:])])
    out["hits"], out["closest"] = hits, closest
    return out


def between(hits):
    """a limit strictly between two of the harms ``hits``: the middle of the widest gap between neighbouring distinct values, None
    where there are fewer than two"""
    vals = sorted(set(hits))
    if len(vals) < 2:
        return None
    gap, lo = max((b - a, a) for a, b in zip(vals, vals[1:]))
    return lo + 0.5 * gap


def fold(cost, safe, need, user, decel, L, a_limit):
    """the fold over cost [M, 16] / safe [M]: copies with decel and user in the two reserved columns, safety lost where need == L or
    decel > a_limit; nothing else changes"""
    cost, safe = np.array(cost, dtype=np.float64), np.array(safe, dtype=np.uint8)
    for m in range(len(safe)):
        cost[m, C_RES0], cost[m, C_RES1] = float(decel[m]), float(user[m])
        if int(need[m]) == L or float(decel[m]) > a_limit:
            safe[m], cost[m, C_SAFE] = 0, 0.0
    return cost, safe
