"""Plain-Python statement of the hidden-traffic ladder verdict (DESIGN.md §5.10 "Ladder verdict", include/fo_hip.h
fo_scene_hidden_brake_ladder_verdict), written from its definition -- not from the product code.  The verdict is defined on what
fo_scene_hidden_brake_ladder_users writes: the inputs here are that entry's outputs ``required_all``, ``blocking`` [M, B] and
``required`` [C, M, B] (from the device or from tests/ref_hidden_brake_ladder_users.py), and what is stated is steps 1 - 7 -- plain
loops over lists of ints."""
import math

import numpy as np

NOT_FINITE = -2
C_SAFE, C_RES0, C_RES1, NC = 12, 14, 15, 16      # FO_C_SAFE, FO_C_RES0, FO_C_RES1, FO_NC (include/fo_hip.h)
OUTPUTS = ("need", "at", "blocking", "user", "decel", "need_of", "first")


def worst(required, ends, L):
    """the maximum of steps 1 and 4 over one row of brake starts: (the largest rank over b < ends, the first b that has it);
    (-1, -1) when ends = 0"""
    need, at = -1, -1
    for b in range(ends):
        rank = int(required[b]) if int(required[b]) >= 0 else L
        if rank > need:                                                                 # (strictly: a tie stays with the first start)
            need, at = rank, b
    return need, at


def fold_one(ra, blk, req, ends, levels, finite=True):
    """steps 1 - 6 for one trajectory: ``ra``, ``blk`` the B ints of required_all and blocking, ``req`` the C rows of required ->
    (need, at, blocking, user, decel, need_of [C])"""
    L = len(levels)
    need, at = worst(ra, ends, L)                                                       # 1., 2.
    blocking = int(blk[at]) if at >= 0 else 0                                           # 3.
    user = next((c for c in range(32) if blocking >> c & 1), -1)
    need_of = [worst(row, ends, L)[0] for row in req]                                   # 4.
    decel = 0.0 if need < 0 else math.inf if need == L else float(levels[need])         # 5.
    if not finite:                                                                      # 6.
        need, at, blocking, user, decel = L, 0, 0, NOT_FINITE, math.inf
    return need, at, blocking, user, decel, need_of


def fold_row(cost_row, safe, need, user, decel, L, a_limit):
    """step 7 for one trajectory: (cost row [16] as a list of floats, safe) -> the new pair; nothing but the three columns changes"""
    row = list(cost_row)
    row[C_RES0], row[C_RES1] = float(decel), float(user)
    if need == L or decel > a_limit:
        safe, row[C_SAFE] = 0, 0.0
    return row, safe


def verdict(required_all, blocking, required, first, levels, B, T, lens=None, finite=None):
    """steps 1 - 6 over the ladder-users outputs ``required_all``, ``blocking`` [M, >= B], ``required`` [C, M, >= B] and ``first``
    [C, M]: a dict of ``need``, ``at``, ``blocking``, ``user`` [M] int32, ``decel`` [M] float64, ``need_of``, ``first`` [C, M] int32"""
    required_all, blocking, required = np.asarray(required_all), np.asarray(blocking), np.asarray(required)
    C, M = required.shape[:2]
    out = dict(need=np.empty(M, np.int32), at=np.empty(M, np.int32), blocking=np.empty(M, np.int32), user=np.empty(M, np.int32),
               decel=np.empty(M, np.float64), need_of=np.empty((C, M), np.int32), first=np.array(first, dtype=np.int32).reshape(C, M))
    for m in range(M):
        Lm = T if lens is None else min(max(int(lens[m]), 0), T)
        got = fold_one(required_all[m].tolist(), blocking[m].tolist(), [required[c, m].tolist() for c in range(C)], min(B, Lm), levels,
                       True if finite is None else bool(finite[m]))
        out["need"][m], out["at"][m], out["blocking"][m], out["user"][m], out["decel"][m] = got[:5]
        out["need_of"][:, m] = got[5]
    return out


def fold(cost, safe, need, user, decel, L, a_limit):
    """step 7 over cost [M, 16] / safe [M]: copies with the fold applied"""
    cost, safe = np.array(cost, dtype=np.float64), np.array(safe, dtype=np.uint8)
    for m in range(len(safe)):
        row, safe[m] = fold_row(cost[m].tolist(), int(safe[m]), int(need[m]), int(user[m]), float(decel[m]), L, a_limit)
        cost[m] = row
    return cost, safe
