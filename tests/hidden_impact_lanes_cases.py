"""What tests/test_hidden_impact_lanes_cpu.py and tests/test_hidden_impact_lanes_gpu.py share (DESIGN.md §5.10 "Impact verdict by
approach angle"): the hand-built move tables over the straight road of tests/hidden_brake_scenes.py, the raw-entry scenes of the
device's checker test with their masks and slacks, and the hand scene with the numbers written out -- so that the CPU test can hold the
condition "no open choice in any of them" by the checkers alone."""
import math
from types import SimpleNamespace

import numpy as np

import hidden_brake_scenes as SC
import hidden_impact_cases as IC
import ref_hidden_clearance as HC
import ref_hidden_reach_flow as RF

NONE = HC.NONE


def table(name):
    """a move table [RNY, RNX] over the road raster of tests/hidden_brake_scenes.py, 0xFF off the road"""
    if name == "any":
        return np.full((SC.RNY, SC.RNX), RF.ANY, dtype=np.uint8)
    if name == "lanes":                                     # the lower lane drives east, the upper one west
        return SC.lane_table()
    assert name == "cross"
    # stripes across the road, 5 columns each: north-bound, south-bound, east-bound, two bits alone (nothing central), a crossing of a
    # north and a west lanelet (the union: five bits), west-bound, a north-east lane -- and so on along the road
    stripes = (RF.sector(90), RF.sector(270), RF.sector(0), 0b00000110, RF.sector(90) | RF.sector(180), RF.sector(180), RF.sector(45))
    moves = np.full((SC.RNY, SC.RNX), RF.ANY, dtype=np.uint8)
    for gx in range(2, 162):
        moves[2:16, gx] = stripes[(gx // 5) % len(stripes)]
    return moves


# the raw-entry scenes of the checker test: (scene, C, K, table, dir_mask, heading_slack, B).  scene "tie31": the T = 31 tie scene of
# tests/test_hidden_brake_verdict_gpu.py, five users on three maps; "maps8": the class-and-map-count scene of
# tests/test_hidden_brake_users_gpu.py, class c on map (c + 1) % K.  Masks none, all and mixed -- 0b01010 binds one of the two classes of
# map 0 of "tie31" and leaves the other free, 0b10110101 one and leaves one on every map of "maps8"
RAW_CASES = (
    ("tie31", 5, 3, "lanes", 0b00000, 0.0, 5), ("tie31", 5, 3, "lanes", 0b11111, 0.0, 5), ("tie31", 5, 3, "cross", 0b01010, 0.0, 31),
    ("tie31", 5, 3, "cross", 0b11111, 0.2, 12), ("tie31", 5, 3, "cross", 0b10101, math.pi / 2.0, 3),
    ("maps8", 4, 1, "lanes", 0b1111, 0.0, 5), ("maps8", 4, 2, "cross", 0b0110, 0.0, 31), ("maps8", 5, 2, "cross", 0b11111, 0.0, 5),
    ("maps8", 8, 3, "cross", 0b10110101, 0.0, 31), ("maps8", 8, 3, "lanes", 0b11111111, 0.2, 5), ("maps8", 1, 1, "cross", 0b1, 0.0, 31),
)


def raw_scene(name, C_, K):
    """(scene, keys [K], qmins [K], thr [C, T], map_of [C], r2_caps [K], rows [C, 4], speed_of [C])"""
    import hidden_brake_users_scenes as US
    import test_hidden_brake_users_gpu as UG
    import test_hidden_brake_verdict_gpu as VG
    if name == "tie31":
        sc = VG._scene(VG.TIE_SCENES[31], US.USERS)
        assert C_ == 5 and K == 3
        return sc, sc.keys, sc.qmins, sc.thr, sc.map_of, sc.r2_caps, IC.rows_of(IC.KINDS5), [u[0] for u in sc.users]
    sc, keys, qmins, cap = UG._three_maps()
    return (sc, keys[:K], qmins[:K], sc.thr[:C_], [(c + 1) % K for c in range(C_)], [cap] * K, IC.rows_of(IC.KINDS8[:C_]),
            list(UG.SPEEDS8[:C_]))


# ------------------------------------------------------------------------------------------------ the hand scene
CAR_ROW = tuple(IC.RI.row("Car", 5.76, 2.6, IC.EGO_MASS))
CAR_SPEED = 13.9
COS_67_5 = 0.3826834323650897           # cos 67.5 deg: a north-bound sector seen from an east-bound ego, pdof = 90 deg - 22.5 deg + ...
COS_157_5 = -0.9238795325112867         # cos 157.5 deg: the ego's own lane, from behind


def hand_case(v0, a_brake, wall_x, byte, T=16, dt=0.5, keys_at_wall=(0, 0, 0, 0), thr=0, beside=None, y=-1.75, x0=0.0, win=None):
    """tests/hidden_impact_cases.wall_case -- a straight east-bound candidate at constant speed ``v0`` from ``x0`` towards a wall of cells
    that begins at ``wall_x`` and spans the window's rows: column n of the wall holds the key ``keys_at_wall[n]``; one class with the
    threshold ``thr`` at every sample -- with a move table whose bytes are ``byte`` (one, or one per column of the wall) on the wall's
    columns where they lie on the raster and ``beside`` (default 0xFF) everywhere else"""
    win = SC.WINDOWS[0] if win is None else win
    road = SC.road_raster()
    ix0, iy0, nx, ny = win
    cols = len(keys_at_wall)
    g0 = int(round((wall_x - SC.ORIGIN[0]) / SC.CS))
    key = np.full((ny, nx), NONE, dtype=np.int32)
    for n, k in enumerate(keys_at_wall):
        if 0 <= g0 + n - ix0 < nx:
            key[:, g0 + n - ix0] = k
    x = (x0 + v0 * np.arange(T) * dt)[None, :]
    yy = np.full((1, T), float(y))
    head = np.stack((np.ones((1, T)), np.zeros((1, T))), -1)
    qmin = np.asarray(HC.clearance(key, win, road, SC.ORIGIN, SC.CS, x, yy, head, SC.HL, SC.HW, SC.WB, None))
    moves = np.full((SC.RNY, SC.RNX), RF.ANY if beside is None else beside, dtype=np.uint8)
    for n in range(cols):
        if 0 <= g0 + n < SC.RNX:
            moves[:, g0 + n] = byte if isinstance(byte, int) else byte[n]
    return SimpleNamespace(T=T, win=win, road=road, key=key, qmin=qmin, x=x, y=yy, head=head, v=np.full((1, T), float(v0)),
                           arc=SC.travelled_arc(x, yy), thr=np.full((1, T), int(thr), dtype=np.int32), r2_cap=1, a_brake=float(a_brake),
                           dt=dt, moves=moves, wall_gx=g0)


def cell_centre_x(gx):
    return SC.ORIGIN[0] + (gx + 0.5) * SC.CS


FRONT = SC.WB + SC.HL                    # from the pose to the front edge of an east-bound footprint


def closing_of(u, s, cm):
    return u + s if cm == 1.0 else math.sqrt(max(0.0, u * u + s * s + 2.0 * u * s * cm))


# v0, a_brake, wall_x, B as the first hand case of tests/test_hidden_impact_gpu.py: from b = 0 the ego is hit at sample 2 with 4 m/s left
HAND_U = 4.0
HAND = (
    # name, byte on the wall's cells -> cosine, closing
    ("a north-bound cross lane", RF.sector(90), COS_67_5, math.sqrt(HAND_U * HAND_U + CAR_SPEED * CAR_SPEED + 2.0 * HAND_U * CAR_SPEED * COS_67_5)),
    ("the oncoming lane", RF.sector(180), 1.0, HAND_U + CAR_SPEED),
    ("its own lane, from behind", RF.sector(0), COS_157_5,
     math.sqrt(HAND_U * HAND_U + CAR_SPEED * CAR_SPEED + 2.0 * HAND_U * CAR_SPEED * COS_157_5)),
    ("an off-lane cell", RF.ANY, 1.0, HAND_U + CAR_SPEED),
)
