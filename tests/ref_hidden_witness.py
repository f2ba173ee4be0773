"""Plain Python / NumPy statement of the hidden-traffic witnesses (DESIGN.md §5.10 "Witnesses"), written from the definition -- not
from the product code: the extension of the maps to every world-raster cell, the conflict cell, the walk back along ``d``.

Windows are (ix0, iy0, nx, ny) in world-raster cells; ``A`` is the arrival map and ``d`` the road distance of one
``fo_scene_hidden_reach_road`` / ``_flow`` call ([ny, nx]), ``road`` the world road raster [rny, rnx], ``moves`` the map's move
table over the raster or None (every step allowed).  Integers only, apart from the footprint test, which is written out here
from §5.10 point 5: centre (x + wb c, y + wb s), ``|u| <= hl`` and ``|w| <= hw`` with ``u = ex c + ey s``, ``w = ey c - ex s``."""
import math

import numpy as np

NEVER, D_NONE, ANY = 255, 65535, 0xFF
NO_CELL = -2 ** 31
# step k points at k * 45 degrees: E, NE, N, NW, W, SW, S, SE; 12 per axis step, 17 per diagonal one
DIRS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
COST = [17 if dx and dy else 12 for dx, dy in DIRS]


def min_path_cap(r2_last):
    """isqrt(169 R2[J-1]) // 12: no walk over a forecast's maps is longer"""
    return math.isqrt(169 * int(r2_last)) // 12


class Maps:
    """A, d and out extended to every world-raster cell"""

    def __init__(self, A, d, win, road, moves=None):
        self.A, self.d, self.win, self.road = np.asarray(A), np.asarray(d), tuple(int(v) for v in win), np.asarray(road)
        self.moves = None if moves is None else np.asarray(moves)

    def _in_window(self, gx, gy):
        ix0, iy0, nx, ny = self.win
        return 0 <= gx - ix0 < nx and 0 <= gy - iy0 < ny

    def _on_raster(self, gx, gy):
        rny, rnx = self.road.shape
        return 0 <= gx < rnx and 0 <= gy < rny

    def arrival(self, gx, gy):
        if self._in_window(gx, gy):
            return int(self.A[gy - self.win[1], gx - self.win[0]])
        return 0 if self._on_raster(gx, gy) and self.road[gy, gx] else NEVER

    def dist(self, gx, gy):
        if self._in_window(gx, gy):
            return int(self.d[gy - self.win[1], gx - self.win[0]])
        return 0 if self._on_raster(gx, gy) and self.road[gy, gx] else D_NONE

    def out(self, gx, gy):
        if self.moves is not None and self._on_raster(gx, gy):
            return int(self.moves[gy, gx])
        return ANY


def footprint_cells(maps, origin, cs, x, y, c, s, hl, hw, wb):
    """(gx, gy) of every cell of the window's and the raster's bounding box whose centre lies in the rectangle (float64, the
    definition's order of operations); a pose that is not finite has none"""
    cx, cy = x + wb * c, y + wb * s
    if not (math.isfinite(cx) and math.isfinite(cy)):
        return []
    ix0, iy0, nx, ny = maps.win
    rny, rnx = maps.road.shape
    lox, loy, hix, hiy = min(ix0, 0), min(iy0, 0), max(ix0 + nx, rnx) - 1, max(iy0 + ny, rny) - 1
    n = int(math.ceil((hl + hw) / cs)) + 2              # no point of the rectangle is farther than hl + hw from its centre
    bx, by = int(math.floor((cx - origin[0]) / cs)), int(math.floor((cy - origin[1]) / cs))
    gx = np.arange(max(bx - n, lox), min(bx + n, hix) + 1)
    gy = np.arange(max(by - n, loy), min(by + n, hiy) + 1)
    if len(gx) == 0 or len(gy) == 0:
        return []
    GX, GY = np.meshgrid(gx, gy)
    px = origin[0] + (GX.astype(np.float64) + 0.5) * cs
    py = origin[1] + (GY.astype(np.float64) + 0.5) * cs
    ex, ey = px - cx, py - cy
    u = ex * c + ey * s
    w = ey * c - ex * s
    inside = (np.abs(u) <= hl) & (np.abs(w) <= hw)
    return [(int(a), int(b)) for a, b in zip(GX[inside], GY[inside])]


def conflict_cell(maps, cells, k_star):
    """g*: among ``cells`` with A <= k*, the smallest (d, gy, gx); None if there is none"""
    best = None
    for gx, gy in cells:
        if maps.arrival(gx, gy) <= k_star:
            key = (maps.dist(gx, gy), gy, gx)
            if best is None or key < best:
                best = key
    return None if best is None else (best[2], best[1])


def predecessors(maps, c):
    """K of cell c: the directions k whose step INTO c, out of p = c - dir_k, lies on a cheapest path"""
    dc, oc = maps.dist(*c), maps.out(*c)
    K = []
    for k, ((dx, dy), w) in enumerate(zip(DIRS, COST)):
        p = (c[0] - dx, c[1] - dy)
        dp = maps.dist(*p)
        if dp != D_NONE and dp + w == dc and (maps.out(*p) >> k) & (oc >> k) & 1:
            K.append(k)
    return K


def walk(maps, g, path_cap):
    """(steps, src, dirs): from g back along d, keeping straight where it can, else the lowest direction; steps = -2 where a
    cell has no predecessor or the row is full"""
    c, prev, dirs = g, None, []
    while maps.dist(*c) > 0:
        K = predecessors(maps, c)
        if not K or len(dirs) == path_cap:
            return -2, c, dirs
        k = prev if prev in K else min(K)
        prev = k
        dirs.append(k)
        c = (c[0] - DIRS[k][0], c[1] - DIRS[k][1])
    return len(dirs), c, dirs


def witnesses(A, d, win, road, first, origin, cs, x, y, heading, hl, hw, wb, path_cap, moves=None):
    """(cell [M, 2] int32, src [M, 2] int32, steps [M] int32, wdist [M] int32, dirs [M, path_cap] uint8)"""
    maps = Maps(A, d, win, road, moves)
    x, y, heading = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(heading, dtype=np.float64)
    M, T = x.shape
    cell = np.full((M, 2), NO_CELL, dtype=np.int32)
    src = np.full((M, 2), NO_CELL, dtype=np.int32)
    steps = np.full(M, -1, dtype=np.int32)
    wdist = np.full(M, -1, dtype=np.int32)
    dirs = np.full((M, path_cap), 255, dtype=np.uint8)
    for m in range(M):
        k = int(first[m])
        if not 0 <= k < T:
            continue
        g = conflict_cell(maps, footprint_cells(maps, origin, cs, x[m, k], y[m, k], heading[m, k, 0], heading[m, k, 1], hl, hw, wb), k)
        if g is None:                    # a first these maps do not bear out
            steps[m] = -2
            continue
        cell[m], wdist[m] = g, maps.dist(*g)
        steps[m], s, route = walk(maps, g, path_cap)
        src[m] = s
        dirs[m, :len(route)] = route
    return cell, src, steps, wdist, dirs
