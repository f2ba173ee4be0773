"""Seeded scenes for the brake clearance's tests (DESIGN.md §5.10 "Brake clearance"), shared by tests/test_hidden_brake_cpu.py --
which holds the checker alone to conditions on them, so that a degenerate scene cannot hide a failure -- and
tests/test_hidden_brake_gpu.py, which runs the same scenes on the device.

The map is the straight two-lane road of tests/test_hidden_reach_gpu._parked_car_scene: lanelets over x in [-10, 70], y in
[-3.5, 3.5], cells of 0.5 m.  Its raster is written down here (no cell centre lies on a lanelet's edge, so there is nothing to
decide): origin (-11, -4.5), 164 x 18 cells, road in rows 2 .. 15 and columns 2 .. 161.  The device test asserts that the model's
own raster is this one."""
import math
from types import SimpleNamespace

import numpy as np

import ref_hidden_reach as HR
import ref_hidden_reach_flow as RF
import ref_hidden_reach_road as RR

CS, ORIGIN = 0.5, (-11.0, -4.5)
RNX, RNY = 164, 18
DT = 0.1
VEH = (4.508, 1.610, 1.4227)          # length, width, wb_rear_axle (BMW 320i)
HL, HW, WB = 0.5 * VEH[0], 0.5 * VEH[1], VEH[2]
ENTRIES = ("fo_scene_hidden_reach", "fo_scene_hidden_reach_road", "fo_scene_hidden_reach_flow")


def road_raster():
    road = np.zeros((RNY, RNX), dtype=np.uint8)
    road[2:16, 2:162] = 1
    return road


def lane_table():
    """the lower lane drives east, the upper one west, everything beside the road is free"""
    moves = np.full((RNY, RNX), RF.ANY, dtype=np.uint8)
    moves[2:9, 2:162] = RF.sector(0)
    moves[9:16, 2:162] = RF.sector(180)
    return moves


def travelled_arc(x, y):
    """be.py's formula, row by row"""
    return np.stack([np.insert(np.cumsum(np.sqrt(np.diff(xr) ** 2 + np.diff(yr) ** 2)), 0, 0) for xr, yr in zip(x, y)]) \
        if len(x) else np.zeros(np.shape(x))


def class_bytes(rng, win, road, blobs, specks=True):
    """class bytes of a window: visible road / visible ground on the raster, nothing known off it; ``blobs`` rectangles of occluded
    cells (the hidden stretches) and a sprinkle of single occluded cells"""
    ix0, iy0, nx, ny = win
    GX, GY = np.meshgrid(np.arange(ix0, ix0 + nx), np.arange(iy0, iy0 + ny))
    on = (GX >= 0) & (GX < RNX) & (GY >= 0) & (GY < RNY)
    is_road = np.zeros((ny, nx), dtype=bool)
    is_road[on] = road[GY[on], GX[on]] != 0
    cls = np.where(is_road, 3, 2).astype(np.uint8)
    cls[~on] = 0
    for _ in range(blobs):
        w, h = int(rng.integers(2, 9)), int(rng.integers(2, 7))
        bx, by = int(rng.integers(0, max(nx - w, 1))), int(rng.integers(0, max(ny - h, 1)))
        sub = cls[by:by + h, bx:bx + w]
        sub[:] = np.where(sub & 1, 5, 4)
    speck = (rng.random((ny, nx)) < 0.003) & specks
    cls[speck] = np.where(cls[speck] & 1, 5, 4)
    return cls


def fan(rng, win, M, T, v_top, ragged):
    """M trajectories of T samples that start in the window's part of the road and drive along it, either way, integrated sample
    by sample; a few stand, a few start beside the road or outside the window"""
    ix0, iy0, nx, ny = win
    x = np.zeros((M, T))
    y = np.zeros((M, T))
    th = np.zeros((M, T))
    v = np.zeros((M, T))
    for m in range(M):
        x0 = ORIGIN[0] + (ix0 + rng.uniform(-4.0, nx + 4.0)) * CS
        y0 = rng.uniform(-3.0, 3.0) if rng.random() < 0.85 else rng.uniform(-9.0, 9.0)
        psi = rng.uniform(-0.12, 0.12) + (math.pi if rng.random() < 0.4 else 0.0)
        kappa = rng.uniform(-0.02, 0.02)
        kind = rng.integers(0, 6)
        v0 = 0.0 if kind == 0 else rng.uniform(0.0, v_top)
        acc = rng.uniform(-3.0, 2.0) if kind >= 3 else 0.0
        px, py = x0, y0
        for k in range(T):
            x[m, k], y[m, k], th[m, k] = px, py, psi
            v[m, k] = min(max(v0 + acc * (k * DT), 0.0), v_top)
            px, py = px + v[m, k] * math.cos(psi) * DT, py + v[m, k] * math.sin(psi) * DT
            psi = psi + kappa * v[m, k] * DT
    lens = rng.integers(-1, T + 2, M).astype(np.int32) if ragged else None
    if ragged and M >= 3:
        lens[:3] = (0, 1, 2)
    return x, y, np.stack((np.cos(th), np.sin(th)), -1), v, lens


WINDOWS = [(-4, -3, 172, 24),         # the whole raster and a rim off it: nothing but the hidden stretches is a source
           (30, -3, 70, 24),          # a part of the road: the road beyond either end is unobserved, A = 0 there
           (120, 6, 60, 20)]          # over the raster's upper right corner


def scene(seed, M, T, entry=0, ragged=False, win=None, a_brake=8.0, v_hidden=None, v_top=None, blobs=None):
    """one seeded scene: window (by the seed: two of three scenes see the whole road), class bytes, reach table, trajectories,
    speeds, arc"""
    rng = np.random.default_rng(seed)
    road = road_raster()
    win = WINDOWS[(0, 1, 0, 2, 0, 0)[seed % 6]] if win is None else win
    whole = win == WINDOWS[0]
    cls = class_bytes(rng, win, road, 2 if blobs is None else blobs, specks=not whole)
    horizon = max(T - 1, 1) * DT
    v_hidden = min(8.0, 24.0 / horizon) if v_hidden is None else v_hidden      # (a reach of at most 48 cells + margin)
    v_top = min(14.0, 45.0 / horizon) if v_top is None else v_top
    r2 = HR.reach_table(v_hidden, DT, math.sqrt(2.0) * CS, CS, T)
    x, y, head, v, lens = fan(rng, win, M, T, v_top, ragged)
    return SimpleNamespace(seed=seed, M=M, T=T, entry=ENTRIES[entry], win=win, cls=cls, hidden=None, r2=r2, x=x, y=y, head=head, v=v,
                           arc=travelled_arc(x, y), lens=lens, a_brake=float(a_brake), dt=DT, road=road, moves=lane_table())


def arrival_and_first(sc):
    """the forecast's map and ``first`` by the forecast's own checkers (CPU)"""
    if sc.entry.endswith("_flow"):
        A = RF.arrival_map_flow(sc.cls, sc.win, sc.road, sc.moves, sc.r2, sc.hidden)[0]
    elif sc.entry.endswith("_road"):
        A = RR.arrival_map_road(sc.cls, sc.win, sc.road, sc.r2, sc.hidden)[0]
    else:
        A = HR.arrival_map(sc.cls, sc.win, sc.road, sc.r2, sc.hidden)[0]
    cells, first, _ = HR.trajectories(A, sc.win, sc.road, ORIGIN, CS, sc.x, sc.y, sc.head, HL, HW, WB, sc.lens)
    return A, cells, first


# the random scenes of both test files: (seed, M, T, entry, ragged).  The workgroup holds 256 / G trajectories, G = the power of two
# >= min(T, 64): 256 at T = 1, 128 at T = 2, 8 at T = 31 and 32, 4 from T = 33 on -- M takes the three values around each
RANDOM_SCENES = [
    (11, 255, 1, 0, False), (12, 256, 1, 1, True), (13, 257, 1, 2, False),
    (21, 127, 2, 1, False), (22, 128, 2, 2, True), (23, 129, 2, 0, False),
    (31, 7, 31, 2, False), (32, 8, 31, 0, True), (33, 9, 31, 1, False), (34, 1, 31, 0, False), (35, 70, 31, 1, True),
    (41, 7, 32, 0, False), (42, 8, 32, 1, False), (43, 9, 32, 2, True),
    (51, 3, 33, 1, False), (52, 4, 33, 2, False), (53, 5, 33, 0, True),
    (61, 3, 64, 2, True), (62, 4, 64, 0, False), (63, 5, 64, 1, False),
    (71, 3, 65, 0, False), (72, 4, 65, 1, True), (73, 5, 65, 2, False),
    (81, 2, 254, 1, False),
]
