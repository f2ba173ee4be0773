"""What tests/test_hidden_harm_ladder_cpu.py and tests/test_hidden_harm_ladder_gpu.py share (DESIGN.md §5.10 "Harm ladder"): the
raw-entry scenes the device is held to the checker on -- scenes of tests/hidden_brake_ladder_users_scenes.py, imported and not
edited, with a kind and a harm row per class -- their three harm limits, the hand case and the non-monotone case.  The CPU test
holds the checker alone to the conditions the device comparison rests on, on every one of them."""
import math
from types import SimpleNamespace

import numpy as np

import hidden_brake_ladder_users_scenes as S
import hidden_impact_cases as IC
import ref_hidden_brake_harm_ladder as RH

# (seed, M, T, ragged, C, layout, L, B) of tests/hidden_brake_ladder_users_scenes.SCENES -- the smallest shapes at which the lane layout
# switches -- both kernel widths, one to three maps, G <= 64, 128 and 256, one round and several
CHECKER_CASES = [
    (124, 3, 31, False, 5, "3", 23, 31),    # the default ladder from every start: Lp = 32, G = 256, 4 rounds; width 8, three maps
    (35, 70, 31, True, 4, "2", 2, 1),       # B = 1, L = 2: G = 2, the rows decide the workgroup; ragged lengths; width 4, two maps
    (32, 3, 31, True, 8, "gap", 33, 1),     # Lp = 64 with 31 padded lanes; eight classes
    (51, 3, 33, True, 4, "3", 2, 33),       # G = 128: a trajectory over two waves, the curve through the exchange
    (54, 3, 33, False, 4, "2", 5, 33),      # Lp = 8, G = 256: 32 starts a round, two rounds, the second with one start
    (21, 70, 2, True, 5, "same", 1, 2),     # T = 2 = B, L = 1: G = 2, 128 trajectories a workgroup; two maps that are one buffer
    (22, 3, 2, False, 8, "3", 64, 1),       # T = 2, B = 1, every lane of a wave a level
]


def pricing(sc):
    """(kinds, rows [C, 4], speed_of [C]) of the classes of a scene: the kinds of tests/hidden_impact_cases.KINDS8 in order, at the
    scene's own (scaled) class speeds"""
    C = len(sc.users)
    return IC.KINDS8[:C], IC.rows_of(IC.KINDS8[:C]), [float(u[0]) for u in sc.users]


def limits(hits):
    """the three limits of a scene whose hits have the harms ``hits``: 0.0, inf and one strictly between two of them (None: the
    scene has fewer than two distinct harms and is no case)"""
    return 0.0, math.inf, RH.between(hits)


def check(sc, lu, harm_limit, levels=None, B=None, finite=None):
    """the checker on a scene and the ladder-users walk ``lu`` of it (brake_first, stop, first: from the device's detail or from
    tests/ref_hidden_brake_ladder_users.py)"""
    _, rows, speed_of = pricing(sc)
    levels = sc.levels if levels is None else levels
    return RH.harm_ladder(lu.brake_first, lu.stop, lu.first, sc.v, list(levels), sc.dt, sc.starts if B is None else B, rows.tolist(), speed_of,
                          harm_limit, sc.lens, finite)


# ------------------------------------------------------------------------------------------------ the hand case
# One candidate at 8 m/s towards the wall of tests/hidden_impact_cases.wall_case at 10 m, dt = 0.5, brake start 0, levels 2 and 4 m/s^2:
#   at 2 m/s^2 the speeds are 8 7 6 .. and the poses 0 4 7.5: the front is over the wall at sample 2, where 8 - 2 * (2 * 0.5) = 6 m/s are left;
#   at 4 m/s^2 the speeds are 8 6 4 2 0 and the poses 0 4 7: the same sample, 8 - 4 * (2 * 0.5) = 4 m/s left;
# both users -- a pedestrian at 2 m/s (class 0) and a car at 6 m/s (class 1) -- wait behind the wall, so both hit at both levels and
# "clear" is reached at neither.  With PED_ROW and CAR_ROW (the rows of KINDS5[0] and KINDS5[4] against IC.EGO_MASS):
#   pedestrian  1 / (1 + exp(3.164 - 0.26951159804844643 * 8)) = 0.26738961171012643  and at w = 6: 0.17553005433799326
#   car         1 / (1 + exp(4.213 + p1 * 12)), p1 = -0.177 * 1093.3 / (1093.3 + m_car): a few percent at both levels
# HAND_LIMIT = 0.2 lies between the pedestrian's two harms: level 0 is over (the pedestrian alone), level 1 is not -> need 1, decel 4.0,
# blocking 0b01, user 0; the ladder verdict on the same inputs says need = 2 = L, "no level".
HAND_LEVELS = (2.0, 4.0)
HAND_LIMIT = 0.2
HAND_KINDS = (IC.KINDS5[0], IC.KINDS5[4])
HAND_SPEED_OF = (2.0, 6.0)
HAND_PED = (0.26738961171012643, 0.17553005433799326)      # the pedestrian's harm at w = 8 and w = 6
HAND_CAR = (0.024615761599242083, 0.022568558271252922)    # the car's at w = 12 and w = 10


def hand_case():
    h = IC.wall_case(8.0, 4.0, 10.0)
    thr = np.zeros((2, h.T), dtype=np.int32)
    return SimpleNamespace(M=1, T=h.T, win=h.win, road=h.road, x=h.x, y=h.y, head=h.head, v=h.v, arc=h.arc, lens=None, dt=h.dt, keys=[h.key],
                           qmins=[h.qmin], thr=thr, map_of=[0, 0], r2_caps=[h.r2_cap], levels=np.array(HAND_LEVELS), starts=1,
                           users=((2.0, "road", "any"), (6.0, "road", "any")), rows=IC.rows_of(HAND_KINDS), speed_of=list(HAND_SPEED_OF))


# ------------------------------------------------------------------------------------------------ the non-monotone case
def non_monotone_case():
    """user 0 of tests/hidden_brake_ladder_users_scenes.hand_scene alone: candidate 0 from brake start 0 passes the band before it is
    reached without braking, lies in it, moving, at 3 m/s^2 and stays short of it at 8 m/s^2 -- hit at the middle level only: harder
    braking is worse there, harm_at is (0, h, 0) with h > 0"""
    sc = S.hand_scene()
    sc.keys, sc.qmins, sc.thr, sc.map_of, sc.r2_caps = sc.keys[:1], sc.qmins[:1], sc.thr[:1], [0], sc.r2_caps[:1]
    sc.users = ((2.0, "road", "any"),)
    sc.rows, sc.speed_of, sc.starts = IC.rows_of(IC.KINDS5[:1]), [2.0], 1
    return sc
