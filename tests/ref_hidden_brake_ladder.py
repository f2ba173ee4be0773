"""Plain-Python statement of the hidden-traffic brake ladder (DESIGN.md §5.10 "Brake ladder", include/fo_hip.h
fo_scene_hidden_brake_ladder), written from its definition -- not from the product code.

Every (trajectory, brake start, level) is walked on its own with tests/ref_hidden_brake.py's ``manoeuvre``, ``speed`` and
``stop_sample`` -- the definition says "steps 1 - 4 of fo_scene_hidden_brake word for word" --, no shortcut for a standing ego, no
sharing between the levels beyond ref_hidden_brake.Footprints' memory of poses it has already scanned.  ``unclear``, ``required``,
``last_unclear`` and ``commit`` are then the definition's sentences over the level axis and the brake-start axis."""
import numpy as np

import ref_hidden_brake as B


def ladder(A, win, road, first, origin, cs, x, y, heading, arc, v, hl, hw, wb, levels, starts, dt, lens=None):
    """(brake_first [M, B, K], stop [M, B, K], required [M, B], last_unclear [M, B], commit [M, K]) int32"""
    x, y, arc, v = (np.asarray(t, dtype=np.float64) for t in (x, y, arc, v))
    heading = np.asarray(heading, dtype=np.float64)
    M, T = x.shape
    levels = [float(a) for a in levels]
    K, nb, dt = len(levels), int(starts), float(dt)
    assert 1 <= nb <= T and K >= 1
    fp = B.Footprints(A, win, road, origin, cs, hl, hw, wb)
    brake_first = np.full((M, nb, K), -1, dtype=np.int32)
    stop = np.full((M, nb, K), -1, dtype=np.int32)
    required = np.full((M, nb), -1, dtype=np.int32)
    last_unclear = np.full((M, nb), -1, dtype=np.int32)
    commit = np.full((M, K), -1, dtype=np.int32)
    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        xr, yr, ar, vr = x[m].tolist(), y[m].tolist(), arc[m].tolist(), v[m].tolist()
        hr = heading[m].tolist()
        fm = int(first[m])
        for b in range(min(nb, Lm)):
            unclear = []
            for k, a_brake in enumerate(levels):
                st = B.stop_sample(vr[b], a_brake, dt, b, Lm)
                bf = -1
                for i, xn, yn, c, s, _, _ in B.manoeuvre(xr, yr, hr, ar, vr[b], Lm, b, a_brake, dt):
                    if fp.min_arrival(xn, yn, c, s) <= i:
                        bf = i
                        break
                brake_first[m, b, k], stop[m, b, k] = bf, st
                unclear.append((0 <= fm <= b) or (0 <= bf < st))
                if unclear[-1] and commit[m, k] < 0:
                    commit[m, k] = b
            required[m, b] = next((k for k in range(K) if not unclear[k]), -1)
            last_unclear[m, b] = next((k for k in reversed(range(K)) if unclear[k]), -1)
    return brake_first, stop, required, last_unclear, commit


def from_single_calls(A, win, road, first, origin, cs, x, y, heading, arc, v, hl, hw, wb, levels, starts, dt, lens=None):
    """the tie, level by level: (brake_first [M, B, K], stop [M, B, K], commit [M, K]) made of one ref_hidden_brake.brake call per
    level -- its rows at b < B, its commit where that is < B"""
    nb = int(starts)
    bfs, sts, cms = [], [], []
    for a_brake in levels:
        bf, st, cm = B.brake(A, win, road, first, origin, cs, x, y, heading, arc, v, hl, hw, wb, float(a_brake), dt, lens)
        bfs.append(bf[:, :nb])
        sts.append(st[:, :nb])
        cms.append(np.where(cm < nb, cm, -1))
    return np.stack(bfs, -1).astype(np.int32), np.stack(sts, -1).astype(np.int32), np.stack(cms, -1).astype(np.int32)


def classes(required, last_unclear, first, lens, T):
    """counts over the (m, b) pairs of a result: ``interior`` (0 < required), ``none_clear`` (a manoeuvre exists, the candidate's own
    first does not block it and no level is clear), ``all_clear`` (required == 0 and nothing unclear), ``non_monotone`` (required >= 0
    and required != last_unclear + 1), ``blocked`` (first <= b), ``no_manoeuvre``"""
    M, nb = required.shape
    out = dict(interior=0, none_clear=0, all_clear=0, non_monotone=0, blocked=0, no_manoeuvre=0)
    for m in range(M):
        Lm = B.clip_len(T, lens, m)
        for b in range(nb):
            r, u = int(required[m, b]), int(last_unclear[m, b])
            if b >= Lm:
                assert (r, u) == (-1, -1)
                out["no_manoeuvre"] += 1
                continue
            blocked = 0 <= int(first[m]) <= b
            out["blocked"] += blocked
            out["interior"] += r > 0
            out["none_clear"] += r < 0 and not blocked
            out["all_clear"] += r == 0 and u == -1
            out["non_monotone"] += r >= 0 and r != u + 1
    return out
