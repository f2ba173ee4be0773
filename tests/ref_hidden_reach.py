"""NumPy statement of the hidden-traffic reach forecast, written from its definition -- not from the
product code.

Windows are (ix0, iy0, nx, ny) in world-raster cells; class bytes are [ny, nx] uint8 with the bits 1 road, 2 visible,
4 occluded; ``road`` is the world road raster [rny, rnx] (nonzero = road).  Everything is integer arithmetic except
``in_rectangle``, which evaluates the definition's float64 expression in its order on the (cos, sin) it is handed."""
import math

import numpy as np

NEVER = 255
SLACK_NONE = 2 ** 31 - 1


def reach_table(v_max, dt, margin, cs, J):
    """R2[j] = floor((v_max j dt + margin)^2 / cs^2), float64"""
    out = []
    for j in range(J):
        rho = v_max * (j * dt) + margin
        out.append(int(math.floor(rho * rho / (cs * cs))))
    return np.array(out, dtype=np.int64)


def sources(cls, win, road, hidden=None, h=0, over=None):
    """S over the region ``over`` (default: the window) grown by h cells on every side, bool [rows, columns]: inside the
    window ``hidden`` if given, else not visible and (road or occluded); outside it on the raster the road bit; off the
    raster 0"""
    cls = np.asarray(cls, dtype=np.uint8)
    rny, rnx = road.shape
    ix0, iy0, nx, ny = win
    ox0, oy0, onx, ony = win if over is None else over
    QX, QY = np.meshgrid(np.arange(ox0 - h, ox0 + onx + h), np.arange(oy0 - h, oy0 + ony + h))
    on = (QX >= 0) & (QX < rnx) & (QY >= 0) & (QY < rny)
    S = np.zeros(QX.shape, dtype=bool)
    S[on] = road[QY[on], QX[on]] != 0
    inside = ((cls & 2) == 0) & ((cls & 5) != 0) if hidden is None else np.asarray(hidden) != 0
    inw = (QX >= ix0) & (QX < ix0 + nx) & (QY >= iy0) & (QY < iy0 + ny)
    S[inw] = inside[QY[inw] - iy0, QX[inw] - ix0]
    return S


def squared_distance(S, win, h, r2max):
    """D2 [ny, nx] int64 over the region (ix0, iy0, nx, ny) that S (grown by h) was made for: min over sources q of
    |g - q|^2, brute force -- the source mask slid over every offset of the disc dx^2 + dy^2 <= r2max, farthest first so
    that the nearest is written last; -1 = none in the disc"""
    _, _, nx, ny = win
    offs = [(dx * dx + dy * dy, dx, dy) for dy in range(-h, h + 1) for dx in range(-h, h + 1) if dx * dx + dy * dy <= r2max]
    offs.sort(reverse=True)
    D2 = np.full((ny, nx), -1, dtype=np.int64)
    for d2, dx, dy in offs:
        np.copyto(D2, d2, where=S[h + dy:h + dy + ny, h + dx:h + dx + nx])
    return D2


def arrival_map(cls, win, road, r2, hidden=None):
    """(A [ny, nx] uint8, D2): A = min { j : D2 <= R2[j] } on road cells, 255 elsewhere"""
    r2 = [int(v) for v in r2]
    assert 1 <= len(r2) <= 254 and all(b >= a for a, b in zip(r2, r2[1:])) and r2[0] >= 0
    h = math.isqrt(r2[-1])
    D2 = squared_distance(sources(cls, win, road, hidden, h), win, h, r2[-1])
    is_road = (np.asarray(cls, dtype=np.uint8) & 1) != 0
    A = np.full(D2.shape, NEVER, dtype=np.uint8)
    for j in range(len(r2) - 1, -1, -1):
        A[is_road & (D2 >= 0) & (D2 <= r2[j])] = j
    return A, D2


def arrival_at(A, win, road, gx, gy):
    """A of world-raster cells (integer arrays): the map inside the window; outside it 0 on road, 255 otherwise / off the raster"""
    ix0, iy0, nx, ny = win
    rny, rnx = road.shape
    gx, gy = np.asarray(gx), np.asarray(gy)
    out = np.full(gx.shape, NEVER, dtype=np.int64)
    on = (gx >= 0) & (gx < rnx) & (gy >= 0) & (gy < rny)
    out[on] = np.where(road[gy[on], gx[on]] != 0, 0, NEVER)
    inw = (gx >= ix0) & (gx < ix0 + nx) & (gy >= iy0) & (gy < iy0 + ny)
    out[inw] = A[gy[inw] - iy0, gx[inw] - ix0]
    return out


def in_rectangle(gx, gy, origin, cs, x, y, c, s, hl, hw, wb):
    """the definition's test of the cells' centres, float64, its operation order (numpy forms no fused multiply-add)"""
    cx, cy = x + wb * c, y + wb * s
    px = origin[0] + (np.asarray(gx, dtype=np.float64) + 0.5) * cs
    py = origin[1] + (np.asarray(gy, dtype=np.float64) + 0.5) * cs
    ex, ey = px - cx, py - cy
    u = ex * c + ey * s
    w = ey * c - ex * s
    return (np.abs(u) <= hl) & (np.abs(w) <= hw)


def _reduce(counts, slack_mk, lens):
    M, T = counts.shape
    first = np.full(M, -1, dtype=np.int32)
    for m in range(M):
        k = np.nonzero(counts[m] > 0)[0]
        if len(k):
            first[m] = k[0]
    return counts.astype(np.int32), first, slack_mk.min(axis=1, initial=SLACK_NONE).astype(np.int32)


def trajectories(A, win, road, origin, cs, x, y, heading, hl, hw, wb, lens=None, chunk=64):
    """(cells [M, T], first [M], slack [M]).  Per pose every cell of a square of half side ceil((hl + hw) / cs) + 2 cells
    about the cell of the rectangle's centre is tested: with a unit heading no point of the rectangle is farther than
    hl + hw from the centre, so the square holds the whole footprint wherever the pose lies (window, raster or beyond)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    heading = np.asarray(heading, dtype=np.float64)
    M, T = x.shape
    n = int(math.ceil((hl + hw) / cs)) + 2
    chunk = max(1, min(chunk, 4096 // max(T, 1)))     # (memory of the [chunk, T, cells] intermediates)
    OX, OY = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1))
    OX, OY = OX.ravel()[None, None, :], OY.ravel()[None, None, :]
    counts = np.zeros((M, T), dtype=np.int64)
    slack = np.full((M, T), SLACK_NONE, dtype=np.int64)
    k = np.arange(T)[None, :, None]
    for m0 in range(0, M, chunk):
        sl = slice(m0, min(m0 + chunk, M))
        xs, ys, c, s = x[sl, :, None], y[sl, :, None], heading[sl, :, 0, None], heading[sl, :, 1, None]
        cx, cy = xs + wb * c, ys + wb * s
        ok = np.isfinite(cx) & np.isfinite(cy)
        bx = np.where(ok, np.floor((np.where(ok, cx, 0.0) - origin[0]) / cs), 0).astype(np.int64)
        by = np.where(ok, np.floor((np.where(ok, cy, 0.0) - origin[1]) / cs), 0).astype(np.int64)
        gx, gy = bx + OX, by + OY
        with np.errstate(invalid="ignore"):
            inside = in_rectangle(gx, gy, origin, cs, xs, ys, c, s, hl, hw, wb)
        a = arrival_at(A, win, road, gx, gy)
        live = inside & (a != NEVER)
        if lens is not None:
            live &= k < np.asarray(lens)[sl, None, None]
        counts[sl] = (live & (a <= k)).sum(axis=2)
        slack[sl] = np.where(live, a - k, SLACK_NONE).min(axis=2)
    return _reduce(counts, slack, lens)


def trajectories_whole_window(A, win, road, origin, cs, x, y, heading, hl, hw, wb, lens=None, ring=None):
    """the same outputs by testing, per pose, every cell of the window plus a ring of ``ring`` cells outside it (default:
    enough to hold a rectangle whose centre lies in the window) -- the plain form, for poses near the window"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    heading = np.asarray(heading, dtype=np.float64)
    M, T = x.shape
    ix0, iy0, nx, ny = win
    if ring is None:
        ring = int(math.ceil((hl + hw + abs(wb)) / cs)) + 2
    GX, GY = np.meshgrid(np.arange(ix0 - ring, ix0 + nx + ring), np.arange(iy0 - ring, iy0 + ny + ring))
    a = arrival_at(A, win, road, GX, GY)
    counts = np.zeros((M, T), dtype=np.int64)
    slack = np.full((M, T), SLACK_NONE, dtype=np.int64)
    for m in range(M):
        for k in range(T if lens is None else min(T, max(int(lens[m]), 0))):
            inside = in_rectangle(GX, GY, origin, cs, x[m, k], y[m, k], heading[m, k, 0], heading[m, k, 1], hl, hw, wb)
            live = inside & (a != NEVER)
            counts[m, k] = (live & (a <= k)).sum()
            if live.any():
                slack[m, k] = (a[live] - k).min()
    return _reduce(counts, slack, lens)
