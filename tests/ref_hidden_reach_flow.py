"""NumPy / heapq statement of the lane flow of the hidden-traffic reach forecast (DESIGN.md §5.10 "Lane flow"), written from its
definition -- not from the product code: heap Dijkstra over directed steps on the window grown by one cell, where the device
relaxes tiles in distance bands.

Windows, class bytes, ``road``, ``hidden``, sources, the passable set, ``L`` and ``A_geo`` as in ``ref_hidden_reach_road``; the move
table ``moves`` (uint8 over the world raster, bit k = step k may be taken out of the cell) is an INPUT.  Integers only."""
import heapq

import numpy as np

import ref_hidden_reach as HR
import ref_hidden_reach_road as RR

NONE = RR.NONE
ANY = 0xFF
# step k points at k * 45 degrees: E, NE, N, NW, W, SW, S, SE; 12 per axis step, 17 per diagonal one
DIRS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
COST = [RR.DIAG if dx and dy else RR.AXIS for dx, dy in DIRS]


def moves_over(moves, win, grow=1):
    """out(q) over the window grown by ``grow`` cells, uint8 [ny + 2 grow, nx + 2 grow]: the table's byte on the raster, 0xFF off it"""
    moves = np.asarray(moves, dtype=np.uint8)
    rny, rnx = moves.shape
    ix0, iy0, nx, ny = win
    out = np.full((ny + 2 * grow, nx + 2 * grow), ANY, dtype=np.uint8)
    qx, qy = np.arange(ix0 - grow, ix0 + nx + grow), np.arange(iy0 - grow, iy0 + ny + grow)
    okx, oky = (qx >= 0) & (qx < rnx), (qy >= 0) & (qy < rny)
    out[np.ix_(oky, okx)] = moves[np.ix_(qy[oky], qx[okx])]
    return out


def dijkstra(S, P, out, limit):
    """d_flow over the grid of S / P / out (NONE = not reached within ``limit``): the cheapest path from a source over allowed
    steps -- q -> g = q + dir_k with g passable, bit k in out(q) and bit k in out(g)"""
    ny, nx = S.shape
    d = np.full((ny, nx), NONE, dtype=np.int64)
    heap = []
    for y, x in zip(*np.nonzero(S)):
        d[y, x] = 0
        heap.append((0, int(x), int(y)))
    heapq.heapify(heap)
    while heap:
        v, x, y = heapq.heappop(heap)
        if v != d[y, x]:
            continue
        for k, ((dx, dy), w) in enumerate(zip(DIRS, COST)):
            gx, gy = x + dx, y + dy
            if not (0 <= gx < nx and 0 <= gy < ny and P[gy, gx]):
                continue
            if not ((int(out[y, x]) >> k) & (int(out[gy, gx]) >> k) & 1):
                continue
            if v + w < d[gy, gx] and v + w <= limit:
                d[gy, gx] = v + w
                heapq.heappush(heap, (v + w, gx, gy))
    return d


def relax_to_fixed_point(S, P, out, limit):
    """the same distances by whole-grid relaxation passes until nothing changes (the plain form)"""
    ny, nx = S.shape
    big = 1 << 30
    d = np.where(S, 0, big).astype(np.int64)
    o = np.zeros((ny + 2, nx + 2), dtype=np.uint8)
    o[1:-1, 1:-1] = out
    while True:
        pad = np.full((ny + 2, nx + 2), big, dtype=np.int64)
        pad[1:-1, 1:-1] = d
        best = d.copy()
        for k, ((dx, dy), w) in enumerate(zip(DIRS, COST)):
            # into g from q = g - dir_k
            dq = pad[1 - dy:1 - dy + ny, 1 - dx:1 - dx + nx]
            oq = o[1 - dy:1 - dy + ny, 1 - dx:1 - dx + nx]
            ok = ((oq >> k) & (out >> k) & 1) != 0
            best = np.minimum(best, np.where(ok, dq + w, big))
        best = np.where(P & (best <= limit), best, d)
        if np.array_equal(best, d):
            break
        d = best
    return np.where(d >= big, NONE, d)


def flow_distance(cls, win, road, moves, r2, hidden=None):
    """(d_flow [ny, nx] uint16, L): 65535 = not reached over allowed steps within L[J-1]"""
    L = RR.reach_units(r2)
    S, P = RR.passable(cls, win, road, hidden)
    d = dijkstra(S, P, moves_over(moves, win), int(L[-1]))
    return d[1:-1, 1:-1].astype(np.uint16), L


def arrival_map_flow(cls, win, road, moves, r2, hidden=None):
    """(A_flow, A_euclid, d_flow, L) with A_flow = max(A_geo(d_flow), A_euclid), 255 the latest"""
    d, L = flow_distance(cls, win, road, moves, r2, hidden)
    A_e, _ = HR.arrival_map(cls, win, road, r2, hidden)
    return np.maximum(RR.arrival_geo(cls, d, L), A_e), A_e, d, L


def sector(yaw_deg):
    """the three directions around a heading that is a multiple of 45 degrees: the byte a straight lane of that heading gets"""
    k = int(round(yaw_deg / 45.0)) % 8
    return (1 << k) | (1 << ((k + 1) % 8)) | (1 << ((k - 1) % 8))
