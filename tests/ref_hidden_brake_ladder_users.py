"""Plain-Python statement of the hidden-traffic brake ladder by road users (DESIGN.md §5.10 "Brake ladder by road users",
include/fo_hip.h fo_scene_hidden_brake_ladder_users), written from its definition -- not from the product code, and not by calling
the users checker level by level or the ladder checker class by class (the CPU tests hold it against both).

Every (trajectory, brake start, level, class) is walked on its own with tests/ref_hidden_brake.py's ``manoeuvre`` and
``stop_sample``, up to that class's first hit on ITS map; the cells under a pose and the minimum key per map are
tests/ref_hidden_brake_users.py's ``Footprint`` (which remembers the pose values it has scanned).  The key maps, the qmin arrays,
``heading``, ``arc``, ``v``, the threshold table, ``map_of`` and the levels are taken as data.  ``unclear`` and everything made of it
are then the definition's sentences over the level, the brake-start and the class axis."""
from collections import namedtuple

import numpy as np

import ref_hidden_brake as B
import ref_hidden_brake_users as U

MAX_LEVELS, MAX_ARG_BYTES = 64, 3584

LadderUsers = namedtuple("LadderUsers", "required last_unclear commit first required_all last_unclear_all blocking brake_first stop")
SUMMARY = LadderUsers._fields[:7]


def blocking_mask(unclear, required_all):
    """step 4's mask of one (m, b): ``unclear [C][L]`` bools -> the classes unclear at level ``required_all - 1``, at ``L - 1`` where
    ``required_all`` is -1, none where it is 0"""
    n_levels = len(unclear[0])
    at = n_levels - 1 if required_all < 0 else required_all - 1
    return 0 if at < 0 else sum(1 << c for c, row in enumerate(unclear) if row[at])


def ladder_users(keys, win, road, qmins, origin, cs, x, y, heading, arc, v, hl, hw, wb, levels, starts, dt, thr, map_of, lens=None):
    """a ``LadderUsers`` of int32 arrays: required, last_unclear [C, M, B]; commit [C, M, L]; first [C, M]; required_all,
    last_unclear_all, blocking [M, B]; brake_first [C, M, B, L]; stop [M, B, L]"""
    x, y, arc, v = (np.asarray(t, dtype=np.float64) for t in (x, y, arc, v))
    heading = np.asarray(heading, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.int64)
    qmins = [np.asarray(q, dtype=np.int64) for q in qmins]
    map_of = [int(k) for k in map_of]
    levels = [float(a) for a in levels]
    M, T = x.shape
    C, K, n_levels, nb, dt = thr.shape[0], len(keys), len(levels), int(starts), float(dt)
    assert 1 <= K <= U.MAX_MAPS and 1 <= C <= U.MAX_CLASSES and C * T <= U.MAX_TABLE and len(qmins) == K
    assert thr.shape == (C, T) and len(map_of) == C and all(0 <= k < K for k in map_of)
    assert 1 <= n_levels <= MAX_LEVELS and 1 <= nb <= T and 4 * C * T + 8 * n_levels <= MAX_ARG_BYTES
    fp = U.Footprint(keys, win, road, origin, cs, hl, hw, wb)
    out = LadderUsers(required=np.full((C, M, nb), -1, dtype=np.int32), last_unclear=np.full((C, M, nb), -1, dtype=np.int32),
                      commit=np.full((C, M, n_levels), -1, dtype=np.int32), first=np.full((C, M), -1, dtype=np.int32),
                      required_all=np.full((M, nb), -1, dtype=np.int32), last_unclear_all=np.full((M, nb), -1, dtype=np.int32),
                      blocking=np.zeros((M, nb), dtype=np.int32), brake_first=np.full((C, M, nb, n_levels), -1, dtype=np.int32),
                      stop=np.full((M, nb, n_levels), -1, dtype=np.int32))
    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        for c in range(C):                                       # 1. first[c][m]: no level in it
            q = qmins[map_of[c]]
            out.first[c, m] = next((j for j in range(Lm) if q[m, j] <= thr[c, j]), -1)
        xr, yr, ar, vr = x[m].tolist(), y[m].tolist(), arc[m].tolist(), v[m].tolist()
        hr = heading[m].tolist()
        for b in range(min(nb, Lm)):
            unclear = [[False] * n_levels for _ in range(C)]
            for n, a_brake in enumerate(levels):
                st = B.stop_sample(vr[b], a_brake, dt, b, Lm)    # 1. stop: no class in it
                out.stop[m, b, n] = st
                walk = list(B.manoeuvre(xr, yr, hr, ar, vr[b], Lm, b, a_brake, dt))
                for c in range(C):
                    bf = next((i for i, xn, yn, hc, hs, _, _ in walk if fp.min_keys(xn, yn, hc, hs)[map_of[c]] <= thr[c, i]), -1)
                    out.brake_first[c, m, b, n] = bf
                    fm = int(out.first[c, m])
                    unclear[c][n] = (0 <= fm <= b) or (0 <= bf < st)                     # 2.
                    if unclear[c][n] and out.commit[c, m, n] < 0:                        # 3. (b ascends)
                        out.commit[c, m, n] = b
            for c in range(C):                                                           # 3.
                out.required[c, m, b] = next((n for n in range(n_levels) if not unclear[c][n]), -1)
                out.last_unclear[c, m, b] = next((n for n in reversed(range(n_levels)) if unclear[c][n]), -1)
            some = [any(unclear[c][n] for c in range(C)) for n in range(n_levels)]       # 4.
            out.required_all[m, b] = next((n for n in range(n_levels) if not some[n]), -1)
            out.last_unclear_all[m, b] = next((n for n in reversed(range(n_levels)) if some[n]), -1)
            out.blocking[m, b] = blocking_mask(unclear, int(out.required_all[m, b]))
    return out


def above_every_user(res, lens, T):
    """the (m, b) pairs with a manoeuvre at which ``required_all`` lies above EVERY class's own ``required`` -- the gentlest level
    clear of all of them is none of the classes' own answers (``required_all`` = -1 counts as above every level; a class that is
    never clear keeps a pair out)"""
    C, M, nb = res.required.shape
    pairs = []
    for m in range(M):
        for b in range(min(nb, B.clip_len(T, lens, m))):
            own = [int(res.required[c, m, b]) for c in range(C)]
            ra = int(res.required_all[m, b])
            if all(r >= 0 for r in own) and (ra < 0 or ra > max(own)):
                pairs.append((m, b))
    return pairs


def kinds(res, lens, T):
    """counts over the (m, b) pairs of a result: ``interior`` (required_all > 0), ``none`` (a manoeuvre and required_all = -1),
    ``zero`` (required_all = 0), ``non_monotone`` (required_all >= 0 and != last_unclear_all + 1), ``above`` (above_every_user),
    ``no_manoeuvre``"""
    M, nb = res.required_all.shape
    out = dict(interior=0, none=0, zero=0, non_monotone=0, above=len(above_every_user(res, lens, T)), no_manoeuvre=0)
    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        for b in range(nb):
            r, u = int(res.required_all[m, b]), int(res.last_unclear_all[m, b])
            if b >= Lm:
                assert (r, u, int(res.blocking[m, b])) == (-1, -1, 0)
                out["no_manoeuvre"] += 1
                continue
            out["interior"] += r > 0
            out["none"] += r < 0
            out["zero"] += r == 0
            out["non_monotone"] += r >= 0 and r != u + 1
    return out
