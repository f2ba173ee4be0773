"""NumPy statement of the occlusion memory, written from its definition -- not from the product code.

Windows are (ix0, iy0, nx, ny) in world-raster cells; class bytes are [ny, nx] uint8 with the bits 1 road, 2 visible,
4 occluded; ``road`` is the world road raster [rny, rnx] (nonzero = road)."""
import math

import numpy as np

MAX_HALO = 32


def reach_r2(v_max, dt_s, margin, cs):
    rho = v_max * dt_s + margin
    return int(math.floor(rho * rho / (cs * cs)))


def offsets(r2):
    """D = {(dx, dy) : dx^2 + dy^2 <= r2}, integers only"""
    h = math.isqrt(r2)
    return [(dx, dy) for dy in range(-h, h + 1) for dx in range(-h, h + 1) if dx * dx + dy * dy <= r2]


def previous_p(road, prev_h, prev_win, win, h):
    """P_{k-1} over the window `win` grown by h cells on every side: H_{k-1} inside the previous window, the road bit
    elsewhere on the raster, 0 off it; prev_h None = a reset (the road bit everywhere)"""
    rny, rnx = road.shape
    ix0, iy0, nx, ny = win
    qx = np.arange(ix0 - h, ix0 + nx + h)
    qy = np.arange(iy0 - h, iy0 + ny + h)
    QX, QY = np.meshgrid(qx, qy)
    on = (QX >= 0) & (QX < rnx) & (QY >= 0) & (QY < rny)
    P = np.zeros(QX.shape, dtype=np.uint8)
    P[on] = road[QY[on], QX[on]] != 0
    if prev_h is not None:
        px0, py0, pnx, pny = prev_win
        inp = (QX >= px0) & (QX < px0 + pnx) & (QY >= py0) & (QY < py0 + pny)
        P[inp] = prev_h[QY[inp] - py0, QX[inp] - px0]
    return P


def step(cls, win, road, r2, prev_h=None, prev_win=None):
    """(H_k [ny, nx] uint8, masked classes) of one step; prev_h None = a reset"""
    cls = np.asarray(cls, dtype=np.uint8)
    ix0, iy0, nx, ny = win
    h = math.isqrt(r2) if prev_h is not None else 0
    P = previous_p(road, prev_h, prev_win, win, h)
    reach = np.zeros((ny, nx), dtype=bool)
    for dx, dy in (offsets(r2) if prev_h is not None else [(0, 0)]):
        reach |= P[h + dy:h + dy + ny, h + dx:h + dx + nx] != 0
    vis, occ, rd = (cls & 2) != 0, (cls & 4) != 0, (cls & 1) != 0
    H = np.where(vis, False, np.where(occ, reach, rd)).astype(np.uint8)
    out = cls.copy()
    out[occ & (H == 0)] &= np.uint8(0xFB)
    return H, out


class Memory:
    """the host rules around `step`: R2 from Δt, the reset reasons"""

    def __init__(self, v_max, dt, cs, margin=None):
        self.v_max, self.dt, self.cs = v_max, dt, cs
        self.margin = math.sqrt(2.0) * cs if margin is None else margin
        self.prev = None      # (H, window)
        self.t = None
        self.explicit = False

    def reset(self):
        self.explicit = True

    def plan(self, timestep):
        if self.explicit:
            return 0, "explicit"
        if self.prev is None:
            return 0, "first"
        if timestep is None or self.t is None or timestep <= self.t:
            return 0, "time"
        r2 = reach_r2(self.v_max, (timestep - self.t) * self.dt, self.margin, self.cs)
        if r2 > MAX_HALO * MAX_HALO:     # sqrt(R2) > MAX_HALO
            return 0, "reach"
        return r2, None

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
