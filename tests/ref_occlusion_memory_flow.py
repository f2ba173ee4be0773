"""NumPy / heapq statement of the vehicle layer of the occlusion memory (DESIGN.md §5.9 "Vehicle layer"), written from its
definition -- not from the product code: heap Dijkstra over directed steps on the window grown by n cells, where the device
relaxes tiles in LDS.

Windows, class bytes and ``road`` as in ``ref_occlusion_memory``; the move table ``moves`` (uint8 over the world raster, bit j =
step j may be taken out of the cell, 0xFF off the raster) is an INPUT, as in ``ref_hidden_reach_flow``, whose step rule this
module uses.  The class bytes are the UNMASKED ones of the step (what the stage holds before any memory).  Integers only."""
import numpy as np

import ref_hidden_reach_flow as F
import ref_occlusion_memory as M
import ref_occlusion_memory_road as R

NONE = F.NONE


def flow_distance(win, road, moves, r2, prev_v, prev_win, grow=None):
    """(d_flow [ny, nx] int64 with NONE = not within L over allowed steps, L); the search runs over the window grown by `grow`
    cells (None = n = L // 12)"""
    L = R.reach_units(r2)
    g = R.halo(r2) if grow is None else grow
    PV, passable = R.grids(road, prev_v, prev_win, win, g)
    d = F.dijkstra(PV, passable, F.moves_over(moves, win, g), L)
    ix0, iy0, nx, ny = win
    return d[g:g + ny, g:g + nx], L


def step(cls, win, road, moves, r2, prev_v=None, prev_win=None, grow=None):
    """V_k [ny, nx] uint8 of one step; prev_v None = a reset: (c & 2) ? 0 : (c & 4) ? 1 : (c & 1), which is H of a
    reset step (an occluded cell of the visibility stage is a road cell)"""
    cls = np.asarray(cls, dtype=np.uint8)
    if prev_v is None:
        return np.where(cls & 2, 0, np.where(cls & 4, 1, cls & 1)).astype(np.uint8)
    disc, _ = M.step(cls, win, road, r2, prev_v, prev_win)          # the disc test of every occluded cell, over PV
    d, L = flow_distance(win, road, moves, r2, prev_v, prev_win, grow)
    vis, occ = (cls & 2) != 0, (cls & 4) != 0
    return np.where(occ & ~vis, (disc != 0) & (d <= L), disc != 0).astype(np.uint8)


class Memory(M.Memory):
    """the host rules of ``ref_occlusion_memory.Memory`` (one plan for H and V: the same r2, the same reset reasons) around
    `step`; ``prev`` holds (V, window)"""

    def advance(self, cls, win, road, moves, timestep):
        r2, reason = self.plan(timestep)
        V = step(cls, win, road, moves, r2, *self.prev) if reason is None else step(cls, win, road, moves, 0)
        self.prev, self.explicit = (V, win), False
        if timestep is not None:
            self.t = timestep
        return V, reason
