"""The raster window the per-step cell classes live in, and what a step hands back instead of a shapely geometry."""
from dataclasses import dataclass

import numpy as np

from .fan_geometry import VISIBLE


@dataclass
class CellWindow:
    """raster window the per-step cell classes live in: window cell (ix, iy) = world raster cell (ix0+ix, iy0+iy)"""
    x0: float
    y0: float
    cs: float
    ix0: int
    iy0: int
    nx: int
    ny: int

    def centers(self, idx):
        idx = np.asarray(idx)
        ix, iy = idx % self.nx, idx // self.nx
        return np.stack((self.x0 + (self.ix0 + ix + 0.5) * self.cs, self.y0 + (self.iy0 + iy + 0.5) * self.cs), -1)

    def cell_of(self, xy):
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        ix = np.floor((xy[:, 0] - self.x0) / self.cs).astype(np.int64) - self.ix0
        iy = np.floor((xy[:, 1] - self.y0) / self.cs).astype(np.int64) - self.iy0
        ok = (ix >= 0) & (ix < self.nx) & (iy >= 0) & (iy < self.ny)
        return np.where(ok, iy * self.nx + ix, -1)


class VisibleArea:
    """What ``evaluate_scenario`` hands back instead of a shapely geometry: the visible polygon's ring (device
    tensor [n_rays, 2]; for an open fan the ego position closes the polygon) and the per-cell classes."""

    def __init__(self, ego_pos, ring, rng, hit_id, cls, window: CellWindow, full_circle, bit=VISIBLE):
        self.ego_pos = np.asarray(ego_pos, dtype=np.float64)
        self.ring, self.range, self.hit_id, self.cls, self.window = ring, rng, hit_id, cls, window
        self.full_circle = full_circle
        self._bit = bit
        self._ring_h = None

    @property
    def exterior(self):
        """polygon vertices as numpy [n,2] (host copy, lazily)"""
        if self._ring_h is None:
            r = self.ring.cpu().numpy()
            self._ring_h = r if self.full_circle else np.concatenate((self.ego_pos[None], r), axis=0)
        return self._ring_h

    @property
    def area(self):
        """area of the cells of this class (cell count x cell area)"""
        return float(((self.cls & self._bit) != 0).sum().item()) * self.window.cs ** 2

    @property
    def ring_area(self):
        p = self.exterior
        x, y = p[:, 0], p[:, 1]
        return 0.5 * abs(float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)))

    @property
    def is_empty(self):
        return not bool(((self.cls & self._bit) != 0).any().item())

    def mask(self):
        """bool device tensor [ny, nx]"""
        return (self.cls & self._bit) != 0

    def contains(self, xy):
        """class bit of the cell containing each point (bool numpy [n])"""
        idx = self.window.cell_of(xy)
        flat = self.cls.reshape(-1).cpu().numpy()
        out = np.zeros(len(idx), dtype=bool)
        ok = idx >= 0
        out[ok] = (flat[idx[ok]] & self._bit) != 0
        return out
