"""NumPy statement of the hidden-traffic clearance (DESIGN.md §5.10 "Clearance and critical speed"), written from its
definition -- not from the product code: brute-force squared distances and the heap Dijkstra of the two reach checkers, a
minimum over a square of cells per pose.

Windows, class bytes, ``road`` and ``hidden`` as in ``ref_hidden_reach``.  Integers only, apart from ``in_rectangle`` and
``critical_speed``."""
import math

import numpy as np

import ref_hidden_reach as HR
import ref_hidden_reach_road as RR

NONE = 2 ** 31 - 1
SLACK_NONE = 2 ** 31 - 1
NEVER = 255


def key_map(cls, win, road, r2_cap, metric="euclid", hidden=None):
    """(key [ny, nx] int64, D2, d): 169 D2 on road cells with D2 <= r2_cap, NONE elsewhere; "road": max(169 D2, d^2), NONE also
    where d is beyond Lcap = isqrt(169 r2_cap) or the cell cannot be reached over passable cells (d is None for "euclid")"""
    assert metric in ("euclid", "road") and r2_cap >= 0
    h = math.isqrt(int(r2_cap))
    D2 = HR.squared_distance(HR.sources(cls, win, road, hidden, h), win, h, int(r2_cap))      # -1 = none within the cap
    is_road = (np.asarray(cls, dtype=np.uint8) & 1) != 0
    ok = is_road & (D2 >= 0) & (D2 <= int(r2_cap))
    key = np.where(ok, 169 * D2, NONE).astype(np.int64)
    d = None
    if metric == "road":
        lcap = math.isqrt(169 * int(r2_cap))
        S, P = RR.passable(cls, win, road, hidden)
        d = RR.dijkstra(S, P, lcap)[1:-1, 1:-1]
        near = ok & (d != RR.NONE) & (d <= lcap)
        key = np.where(near, np.maximum(key, d * d), NONE).astype(np.int64)
    return key, D2, d


def key_at(key, win, road, gx, gy):
    """key of world-raster cells: the map inside the window; outside it 0 on road, NONE otherwise / off the raster"""
    ix0, iy0, nx, ny = win
    rny, rnx = road.shape
    gx, gy = np.asarray(gx), np.asarray(gy)
    out = np.full(gx.shape, NONE, dtype=np.int64)
    on = (gx >= 0) & (gx < rnx) & (gy >= 0) & (gy < rny)
    out[on] = np.where(road[gy[on], gx[on]] != 0, 0, NONE)
    inw = (gx >= ix0) & (gx < ix0 + nx) & (gy >= iy0) & (gy < iy0 + ny)
    out[inw] = key[gy[inw] - iy0, gx[inw] - ix0]
    return out


def clearance(key, win, road, origin, cs, x, y, heading, hl, hw, wb, lens=None):
    """qmin [M, T] int64: min of key over the footprint cells of every pose, NONE for an empty footprint and for k >= len[m].
    Per pose every cell of a square of half side ceil((hl + hw) / cs) + 2 about the cell of the rectangle's centre is tested
    (with a unit heading no point of the rectangle is farther than hl + hw from the centre)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    heading = np.asarray(heading, dtype=np.float64)
    M, T = x.shape
    n = int(math.ceil((hl + hw) / cs)) + 2
    OX, OY = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1))
    OX, OY = OX.ravel()[None, :], OY.ravel()[None, :]
    qmin = np.full((M, T), NONE, dtype=np.int64)
    for m in range(M):
        L = T if lens is None else min(T, max(int(lens[m]), 0))
        if L == 0:
            continue
        xs, ys, c, s = x[m, :L, None], y[m, :L, None], heading[m, :L, 0, None], heading[m, :L, 1, None]
        cx, cy = xs + wb * c, ys + wb * s
        ok = np.isfinite(cx) & np.isfinite(cy)
        bx = np.where(ok, np.floor((np.where(ok, cx, 0.0) - origin[0]) / cs), 0).astype(np.int64)
        by = np.where(ok, np.floor((np.where(ok, cy, 0.0) - origin[1]) / cs), 0).astype(np.int64)
        gx, gy = bx + OX, by + OY
        with np.errstate(invalid="ignore"):
            inside = HR.in_rectangle(gx, gy, origin, cs, xs, ys, c, s, hl, hw, wb)
        qmin[m, :L] = np.where(inside, key_at(key, win, road, gx, gy), NONE).min(axis=1)
    return qmin


def reach_from_qmin(qmin, r2):
    """(hit [M, T] bool, first [M], slack [M]) of the reach table r2 [T], by the tie: A <= j iff key <= 169 R2[j]"""
    qmin = np.asarray(qmin, dtype=np.int64)
    M, T = qmin.shape
    thr = [169 * int(v) for v in r2]
    assert len(thr) == T
    hit = np.zeros((M, T), dtype=bool)
    first = np.full(M, -1, dtype=np.int32)
    slack = np.full(M, SLACK_NONE, dtype=np.int64)
    for m in range(M):
        for k in range(T):
            q = int(qmin[m, k])
            j = next((j for j in range(T) if q <= thr[j]), NEVER)
            hit[m, k] = q <= thr[k]
            if hit[m, k] and first[m] < 0:
                first[m] = k
            if j != NEVER:
                slack[m] = min(slack[m], j - k)
    return hit, first, slack.astype(np.int32)


def critical_speed(qmin, cs, dt, margin):
    """v_crit [M] float64: min over samples of 0 / inf at k = 0 (qmin <= 169 floor(margin^2 / cs^2)), max(0, r - margin) / (k dt)
    at k >= 1 with r = sqrt(qmin / 169) cs; inf where nothing is within the cap"""
    qmin = np.asarray(qmin, dtype=np.int64)
    M, T = qmin.shape
    r2_0 = int(math.floor(margin * margin / (cs * cs)))
    out = np.full(M, np.inf)
    for m in range(M):
        for k in range(T):
            q = int(qmin[m, k])
            if q == NONE:
                continue
            if k == 0:
                v = 0.0 if q <= 169 * r2_0 else np.inf
            else:
                v = max(0.0, math.sqrt(q / 169.0) * cs - margin) / (k * dt)
            out[m] = min(out[m], v)
    return out
