"""NumPy / heapq statement of the road metric of the occlusion memory (DESIGN.md §5.9 "Road metric"), written from its
definition -- not from the product code: heap Dijkstra over the window grown by n cells, where the device relaxes tiles in LDS.

Windows, class bytes and ``road`` as in ``ref_occlusion_memory``.  Integers only."""
import heapq
import math

import numpy as np

import ref_occlusion_memory as M

AXIS, DIAG = 12, 17
STEPS = [(dx, dy, DIAG if dx and dy else AXIS) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
NONE = 1 << 30


def reach_units(r2):
    """L = isqrt(169 r2)"""
    return math.isqrt(169 * int(r2))


def halo(r2):
    """n = L // 12: the most steps a path of cost <= L can have"""
    return reach_units(r2) // AXIS


def grids(road, prev_h, prev_win, win, grow):
    """(P_{k-1}, Pass) over `win` grown by `grow` cells, bool: Pass = P or the raster's road bit (0 off the raster)"""
    P = M.previous_p(road, prev_h, prev_win, win, grow) != 0
    R = M.previous_p(road, None, None, win, grow) != 0       # (a reset's P is the road bit itself)
    return P, P | R


def dijkstra(P, passable, limit):
    """d over the grid (python ints, NONE = not within `limit`): cheapest 8-connected path from a cell of P over passable
    cells, 12 per axis step and 17 per diagonal step, a diagonal step asking for its two end cells only"""
    ny, nx = P.shape
    d = np.full((ny, nx), NONE, dtype=np.int64)
    d[P] = 0
    # only a source with a passable neighbour that is no source can improve anything: the others need not be popped
    open_ = np.pad(passable & ~P, 1)
    front = np.zeros((ny, nx), dtype=bool)
    for dx, dy, _ in STEPS:
        front |= open_[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    heap = [(0, int(x), int(y)) for y, x in zip(*np.nonzero(P & front))]
    heapq.heapify(heap)
    while heap:
        v, x, y = heapq.heappop(heap)
        if v != d[y, x]:
            continue
        for dx, dy, w in STEPS:
            qx, qy = x + dx, y + dy
            if 0 <= qx < nx and 0 <= qy < ny and passable[qy, qx] and v + w < d[qy, qx] and v + w <= limit:
                d[qy, qx] = v + w
                heapq.heappush(heap, (v + w, qx, qy))
    return d


def relax_to_fixed_point(P, passable, limit):
    """the same distances by whole-grid relaxation passes until nothing changes (the plain form)"""
    ny, nx = P.shape
    d = np.where(P, 0, NONE).astype(np.int64)
    while True:
        pad = np.full((ny + 2, nx + 2), NONE, dtype=np.int64)
        pad[1:-1, 1:-1] = d
        best = d.copy()
        for dx, dy, w in STEPS:
            best = np.minimum(best, pad[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] + w)
        best = np.where(passable & (best <= limit), best, d)
        if np.array_equal(best, d):
            return d
        d = best


def road_distance(win, road, r2, prev_h, prev_win, grow=None):
    """(d [ny, nx] int64 with NONE = beyond L, L); the search runs over the window grown by `grow` cells (None = n)"""
    L = reach_units(r2)
    g = halo(r2) if grow is None else grow
    P, passable = grids(road, prev_h, prev_win, win, g)
    d = dijkstra(P, passable, L)
    ix0, iy0, nx, ny = win
    return d[g:g + ny, g:g + nx], L


def step(cls, win, road, r2, prev_h=None, prev_win=None, grow=None):
    """(H_k [ny, nx] uint8, masked classes) of one step under the road metric; prev_h None = a reset, which is the Euclidean
    memory's reset"""
    if prev_h is None:
        return M.step(cls, win, road, r2)
    cls = np.asarray(cls, dtype=np.uint8)
    H_e, _ = M.step(cls, win, road, r2, prev_h, prev_win)          # the disc test of every occluded cell
    d, L = road_distance(win, road, r2, prev_h, prev_win, grow)
    vis, occ = (cls & 2) != 0, (cls & 4) != 0
    H = np.where(occ & ~vis, (H_e != 0) & (d <= L), H_e != 0).astype(np.uint8)
    out = cls.copy()
    out[occ & (H == 0)] &= np.uint8(0xFB)
    return H, out


class Memory(M.Memory):
    """the host rules of ``ref_occlusion_memory.Memory`` around the road metric's `step`"""

    def advance(self, cls, win, road, timestep):
        r2, reason = self.plan(timestep)
        if reason is None:
            H, out = step(cls, win, road, r2, *self.prev)
        else:
            H, out = step(cls, win, road, 0)
        self.prev, self.explicit = (H, win), False
        if timestep is not None:
            self.t = timestep
        return H, out, reason
