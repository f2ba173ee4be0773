"""What tests/test_hidden_harm_ladder_lanes_cpu.py and tests/test_hidden_harm_ladder_lanes_gpu.py share (DESIGN.md §5.10 "Harm ladder
by approach angle"): the raw-entry scenes of tests/hidden_impact_lanes_cases.RAW_CASES -- imported, not edited -- as scenes of the
ladder family (a ladder of three levels around the scene's own deceleration), their two limits between the recorded harms, the checker
on a walk, and the hand case with the numbers written out -- so that the CPU test can hold the conditions the device comparison rests
on by the checkers alone."""
import math
from types import SimpleNamespace

import numpy as np

import hidden_brake_scenes as SC
import hidden_impact_lanes_cases as LC
import ref_hidden_brake_harm_ladder as RH
import ref_hidden_brake_harm_ladder_lanes as RHL
import ref_hidden_impact_lanes as RL

RAW_CASES = LC.RAW_CASES


def raw_case(case):
    """RAW_CASES[case] as a scene of the ladder family: what tests/test_hidden_brake_ladder_users_gpu._raw and the raw entry of the device
    test read, and ``moves``, ``mask``, ``slack``, ``rows``, ``speed_of``; the ladder is half, once and twice the scene's deceleration"""
    name, C_, K, tab, mask, slack, B = RAW_CASES[case]
    sc, keys, qmins, thr, map_of, r2_caps, rows, speed_of = LC.raw_scene(name, C_, K)
    return SimpleNamespace(x=sc.x, y=sc.y, head=sc.head, v=sc.v, arc=sc.arc, lens=sc.lens, win=sc.win, dt=sc.dt, keys=list(keys), qmins=list(qmins),
                           thr=np.ascontiguousarray(thr, dtype=np.int32), map_of=list(map_of), r2_caps=list(r2_caps), T=sc.x.shape[1], M=sc.x.shape[0],
                           road=SC.road_raster(), users=tuple((float(s), "road", "any") for s in speed_of),
                           levels=np.array([0.5 * sc.a_brake, sc.a_brake, 2.0 * sc.a_brake]), starts=B, rows=np.asarray(rows, dtype=np.float64),
                           speed_of=[float(s) for s in speed_of], moves=LC.table(tab), mask=mask, slack=slack)


def check(sc, lu, harm_limit, mask=None, slack=None, moves=None, levels=None, finite=None):
    """the checker on a scene and the ladder-users walk ``lu`` of it (brake_first, stop, first)"""
    cos_h, sin_h = RL.host_h(sc.slack if slack is None else slack)
    return RHL.harm_ladder_lanes(sc.keys, sc.win, sc.road, sc.moves if moves is None else moves, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v,
                                 SC.HL, SC.HW, SC.WB, list(sc.levels if levels is None else levels), sc.dt, sc.thr, sc.map_of, sc.starts, sc.rows.tolist(),
                                 sc.speed_of, sc.mask if mask is None else mask, cos_h, sin_h, harm_limit, lu.brake_first, lu.stop, lu.first, sc.lens,
                                 finite)


def limits(hits):
    """the two limits of a scene whose hits have the harms ``hits``: the middles of its two widest gaps between neighbouring distinct
    harms -- each strictly between two recorded harms, with a hit over it and one under it (None: fewer than three distinct harms, the
    scene is no case)"""
    vals = sorted(set(hits))
    if len(vals) < 3:
        return None
    gaps = sorted(((b - a, a) for a, b in zip(vals, vals[1:])), reverse=True)[:2]
    return tuple(sorted(lo + 0.5 * gap for gap, lo in gaps))


# ------------------------------------------------------------------------------------------------ the hand case
# tests/hidden_impact_lanes_cases.hand_case: the ego heads East at 8 m/s towards a wall of cells at 10 m, dt = 0.5, brake start 0, where a
# car at 13.9 m/s may be.  Levels 2 and 4 m/s^2: the poses are 0 4 7.5 and 0 4 7 -- the front is over the wall at sample 2 at both, with
# 8 - 2 * (2 * 0.5) = 6 m/s and 8 - 4 * (2 * 0.5) = 4 m/s left.  With CAR_ROW = (p0, p1):
#   head-on (an off-lane cell, the oncoming lane)   w = 6 + 13.9, 4 + 13.9           harm 0.034616760809621  0.031764897885419
#   a north-bound cross lane, cosine = cos 67.5 deg  w = sqrt(u^2 + 13.9^2 + 2 u 13.9 cm)  harm 0.030713356125559  0.029099514513638
# HAND_LIMIT = 0.030 lies between the two approaches at 4 m/s and below both at 6 m/s: head-on no level suffices (need = 2), from the cross
# lane level 1 does.
HAND_LEVELS = (2.0, 4.0)
HAND_LIMIT = 0.030
HAND_U = (6.0, 4.0)
HAND_HEAD_ON = (0.034616760809621, 0.031764897885419)
HAND_CROSS = (0.030713356125559, 0.029099514513638)


def hand_harm(u, cm):
    """the car's harm at the ego speed ``u`` under the cosine ``cm``, from CAR_ROW and the logistic alone"""
    return RH.logistic(LC.CAR_ROW[0], LC.CAR_ROW[1], LC.closing_of(u, LC.CAR_SPEED, cm))


def hand_case(byte, **kw):
    """the hand scene with the move byte ``byte`` on the wall, as a scene of the ladder family with the car lane-bound"""
    h = LC.hand_case(8.0, 4.0, 10.0, byte, **kw)
    return SimpleNamespace(x=h.x, y=h.y, head=h.head, v=h.v, arc=h.arc, lens=None, win=h.win, dt=h.dt, keys=[h.key], qmins=[h.qmin], thr=h.thr,
                           map_of=[0], r2_caps=[h.r2_cap], T=h.T, M=1, road=h.road, users=((LC.CAR_SPEED, "road", "lanes"),),
                           levels=np.array(HAND_LEVELS), starts=1, rows=np.array([LC.CAR_ROW]), speed_of=[LC.CAR_SPEED], moves=h.moves, mask=1,
                           slack=0.0)


def walk_on_the_host(sc, levels=None):
    """the ladder-users walk of a scene by tests/ref_hidden_brake_ladder_users.py"""
    import ref_hidden_brake_ladder_users as LU
    return LU.ladder_users(sc.keys, sc.win, sc.road, sc.qmins, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB,
                           list(sc.levels if levels is None else levels), sc.starts, sc.dt, sc.thr, sc.map_of, sc.lens)
