"""NumPy / heapq statement of the road metric of the hidden-traffic reach forecast (DESIGN.md §5.10 "Road metric"), written
from its definition -- not from the product code: heap Dijkstra over the window grown by one cell, where the device relaxes
tiles in distance bands.

Windows, class bytes, ``road`` and ``hidden`` as in ``ref_hidden_reach``.  Integers only."""
import heapq
import math

import numpy as np

import ref_hidden_reach as HR

NONE = 65535
AXIS, DIAG = 12, 17
STEPS = [(dx, dy, DIAG if dx and dy else AXIS) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]


def reach_units(r2):
    """L[j] = isqrt(169 R2[j])"""
    return np.array([math.isqrt(169 * int(v)) for v in r2], dtype=np.int64)


def passable(cls, win, road, hidden=None):
    """(S, P) over the window grown by one cell, bool [ny + 2, nx + 2]: P = S or road inside the window, P = S outside it"""
    S = HR.sources(cls, win, road, hidden, 1)
    P = S.copy()
    P[1:-1, 1:-1] |= (np.asarray(cls, dtype=np.uint8) & 1) != 0
    return S, P


def dijkstra(S, P, limit):
    """d over the grid of S / P (python ints, NONE = impassable or beyond ``limit``): cheapest 8-connected path from a source
    over passable cells, 12 per axis step and 17 per diagonal step, a diagonal step asking for its two end cells only"""
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
        for dx, dy, w in STEPS:
            qx, qy = x + dx, y + dy
            if 0 <= qx < nx and 0 <= qy < ny and P[qy, qx] and v + w < d[qy, qx] and v + w <= limit:
                d[qy, qx] = v + w
                heapq.heappush(heap, (v + w, qx, qy))
    return d


def relax_to_fixed_point(S, P, limit):
    """the same distances by whole-grid relaxation passes until nothing changes (the plain form)"""
    ny, nx = S.shape
    big = 1 << 30
    d = np.where(S, 0, big).astype(np.int64)
    while True:
        pad = np.full((ny + 2, nx + 2), big, dtype=np.int64)
        pad[1:-1, 1:-1] = d
        best = d.copy()
        for dx, dy, w in STEPS:
            best = np.minimum(best, pad[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] + w)
        best = np.where(P & (best <= limit), best, d)
        if np.array_equal(best, d):
            break
        d = best
    return np.where(d >= big, NONE, d)


def road_distance(cls, win, road, r2, hidden=None):
    """(d [ny, nx] uint16, L): 65535 = impassable or beyond L[J-1]"""
    L = reach_units(r2)
    S, P = passable(cls, win, road, hidden)
    d = dijkstra(S, P, int(L[-1]))
    return d[1:-1, 1:-1].astype(np.uint16), L


def arrival_geo(cls, d, L):
    """A_geo [ny, nx] uint8: min { j : d <= L[j] } on road cells, 255 elsewhere"""
    is_road = (np.asarray(cls, dtype=np.uint8) & 1) != 0
    A = np.full(d.shape, HR.NEVER, dtype=np.uint8)
    dd = d.astype(np.int64)
    for j in range(len(L) - 1, -1, -1):
        A[is_road & (dd != NONE) & (dd <= int(L[j]))] = j
    return A


def arrival_map_road(cls, win, road, r2, hidden=None):
    """(A_road, A_euclid, d, L) with A_road = max(A_geo, A_euclid), 255 the latest"""
    d, L = road_distance(cls, win, road, r2, hidden)
    A_e, _ = HR.arrival_map(cls, win, road, r2, hidden)
    return np.maximum(arrival_geo(cls, d, L), A_e), A_e, d, L
