"""What the tests of the brake clearance by classes share (DESIGN.md §5.10 "Brake clearance by classes"): the seeded scenes of
tests/hidden_brake_scenes.py with a set of hidden-user speeds, their reach tables, the threshold table and -- by the checkers
alone -- the key map of the scene's forecast and the clearance of its trajectories."""
import math

import numpy as np

import hidden_brake_scenes as SC
import ref_hidden_clearance as HC
import ref_hidden_reach as HR
import ref_hidden_reach_flow as RF
import ref_hidden_reach_road as RR

SPEEDS = (1.5, 4.0, 8.0)              # m/s: a pedestrian, a cyclist, slow urban traffic
MARGIN = math.sqrt(2.0) * SC.CS


def speeds_for(T, speeds=SPEEDS):
    """``speeds`` up to a horizon of 31 samples; beyond it scaled down together, as the scenes scale their own ``v_hidden``, so that
    the fastest reach stays at 48 cells + margin (8 m/s over 25 s would be a reach of 400 cells, beyond the halo cap)"""
    f = min(8.0, 24.0 / (max(T - 1, 1) * SC.DT)) / 8.0
    return tuple(v * f for v in speeds)


def reach_tables(speeds, T, dt=SC.DT, margin=MARGIN, cs=SC.CS):
    return [HR.reach_table(v, dt, margin, cs, T) for v in speeds]


def thresholds(tables):
    """thr [C, T] int64: 169 R2_c[j]"""
    return np.stack([169 * np.asarray(t, dtype=np.int64) for t in tables])


def key_map(sc, r2_cap):
    """the key map behind the scene's forecast: 169 D2, max(169 D2, d^2) along the road, max(169 D2, d_flow^2) along the lanes"""
    if sc.entry.endswith("_flow"):
        key = HC.key_map(sc.cls, sc.win, sc.road, r2_cap, "euclid", sc.hidden)[0]
        S, P = RR.passable(sc.cls, sc.win, sc.road, sc.hidden)
        d = RF.dijkstra(S, P, RF.moves_over(sc.moves, sc.win), math.isqrt(169 * int(r2_cap)))[1:-1, 1:-1]
        near = (key != HC.NONE) & (d != RF.NONE)
        return np.where(near, np.maximum(key, d * d), HC.NONE).astype(np.int64)
    return HC.key_map(sc.cls, sc.win, sc.road, r2_cap, "road" if sc.entry.endswith("_road") else "euclid", sc.hidden)[0]


def class_scene(spec, speeds=SPEEDS, maps=True):
    """the scene of ``spec`` (seed, M, T, entry, ragged) with ``speeds`` (scaled by :func:`speeds_for`), ``tables``, ``thr``,
    ``r2_cap`` = the end of the fastest table and, with ``maps``, ``key`` and ``qmin`` by the checkers"""
    sc = SC.scene(*spec)
    sc.speeds = speeds_for(sc.T, speeds)
    sc.tables = reach_tables(sc.speeds, sc.T)
    sc.thr = thresholds(sc.tables)
    sc.r2_cap = max(int(t[-1]) for t in sc.tables)
    if maps:
        sc.key = key_map(sc, sc.r2_cap)
        sc.qmin = HC.clearance(sc.key, sc.win, sc.road, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, SC.HL, SC.HW, SC.WB, sc.lens)
    return sc
