"""Plain-Python statement of the hidden-traffic fail-safe verdict (DESIGN.md §5.10 "Fail-safe verdict", include/fo_hip.h
fo_scene_hidden_brake_verdict and fo_scene_hidden_poses), written from its definition -- not from the product code.  The walk is
tests/ref_hidden_brake_users.py's, taken whole: the verdict is defined on what fo_scene_hidden_brake_users writes.  What is stated here
is steps 1 - 5 -- plain loops over lists of ints -- and the pose preparation."""
import math

import numpy as np

import ref_hidden_brake_users as BU

NOT_FINITE = -2
C_SAFE, C_RES0, C_RES1, NC = 12, 14, 15, 16      # FO_C_SAFE, FO_C_RES0, FO_C_RES1, FO_NC (include/fo_hip.h)


def fold_one(commit_users, B, finite=True):
    """steps 1 - 4 for one trajectory: ``commit_users`` the C ints of fo_scene_hidden_brake_users -> (commit [C], fail_safe, user)"""
    commit = [int(c) if 0 <= int(c) < B else -1 for c in commit_users]                  # 1.
    fail_safe, user = B, -1
    for c, at in enumerate(commit):
        if at >= 0 and at < fail_safe:                                                  # 2., 3.: a tie stays with the lowest class
            fail_safe, user = at, c
    if not finite:                                                                      # 4.
        fail_safe, user = 0, NOT_FINITE
    return commit, fail_safe, user


def fold_row(cost_row, safe, fail_safe, user, commit_min):
    """step 5 for one trajectory: (cost row [16] as a list of floats, safe) -> the new pair; nothing but the three columns changes"""
    row = list(cost_row)
    row[C_RES0], row[C_RES1] = float(fail_safe), float(user)
    if fail_safe < commit_min:
        safe, row[C_SAFE] = 0, 0.0
    return row, safe


def verdict(commit_users, B, finite=None):
    """steps 1 - 4 over ``commit_users [C, M]``: (commit [C, M], fail_safe [M], user [M]) int32"""
    commit_users = np.asarray(commit_users)
    C, M = commit_users.shape
    commit = np.empty((C, M), dtype=np.int32)
    fail_safe, user = np.empty(M, dtype=np.int32), np.empty(M, dtype=np.int32)
    for m in range(M):
        col, fail_safe[m], user[m] = fold_one(commit_users[:, m].tolist(), B, True if finite is None else bool(finite[m]))
        commit[:, m] = col
    return commit, fail_safe, user


def fold(cost, safe, fail_safe, user, commit_min):
    """step 5 over cost [M, 16] / safe [M]: copies with the fold applied"""
    cost, safe = np.array(cost, dtype=np.float64), np.array(safe, dtype=np.uint8)
    for m in range(len(safe)):
        row, safe[m] = fold_row(cost[m].tolist(), int(safe[m]), int(fail_safe[m]), int(user[m]), commit_min)
        cost[m] = row
    return cost, safe


def finite_flags(x, y, theta, v, lens=None):
    """finite [M] uint8 of fo_scene_hidden_poses: every x, y, theta, v of the samples k < Lm is finite"""
    M, T = np.shape(x)
    out = np.ones(M, dtype=np.uint8)
    for m in range(M):
        Lm = T if lens is None else min(max(int(lens[m]), 0), T)
        for k in range(Lm):
            if not all(math.isfinite(float(a[m][k])) for a in (x, y, theta, v)):
                out[m] = 0
    return out


def brake_verdict(keys, win, road, qmins, origin, cs, x, y, heading, arc, v, hl, hw, wb, a_brake, dt, thr, map_of, B, lens=None, finite=None):
    """the whole definition: the users checker's walk, then steps 1 - 4: (fail_safe [M], user [M], commit [C, M], first [C, M])"""
    _, _, commit_users, first = BU.brake_users(keys, win, road, qmins, origin, cs, x, y, heading, arc, v, hl, hw, wb, a_brake, dt, thr,
                                               map_of, lens)
    commit, fail_safe, user = verdict(commit_users, B, finite)
    return fail_safe, user, commit, first
