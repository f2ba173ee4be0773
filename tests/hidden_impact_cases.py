"""What tests/test_hidden_impact_cpu.py and tests/test_hidden_impact_gpu.py share: the kinds, speeds and harm rows of the road users of
the raw-entry scenes, and those scenes themselves (the tie scenes of tests/test_hidden_brake_verdict_gpu.py, the class-and-map-count
scene of tests/test_hidden_brake_users_gpu.py and the wall of the hand case), so that the CPU test can hold the condition "no open
choice in any of them" by the checker alone."""
from types import SimpleNamespace

import numpy as np

import hidden_brake_scenes as SC
import ref_hidden_impact as RI

EGO_MASS = 1093.3                                  # kg
# one kind per user of tests/hidden_brake_users_scenes.USERS (1.5, 4.0, 4.0, 4.0, 8.0 m/s), inflated dimensions in m
KINDS5 = (("Pedestrian", 0.36, 0.65), ("Bicycle", 2.8, 2.25), ("Pedestrian", 0.36, 0.65), ("Motorcycle", 2.64, 1.04), ("Car", 5.76, 2.6))
# ... and of SPEEDS8 of tests/test_hidden_brake_users_gpu.py: eight classes, a truck and a bus among them
KINDS8 = KINDS5 + (("Truck", 10.8, 3.25), ("Bus", 14.4, 3.38), ("Taxi", 5.52, 2.47))


def rows_of(kinds, ego_mass=EGO_MASS):
    return np.array([RI.row(k, l, w, ego_mass) for k, l, w in kinds], dtype=np.float64)


def kinds_of(users, all_kinds=KINDS5, all_users=None):
    """the kinds of a selection ``users`` of ``all_users`` (by identity of the triples)"""
    return tuple(all_kinds[all_users.index(u)] for u in users)


# ------------------------------------------------------------------------------------------------ the hand case: a wall of key-0 cells
def wall_case(v0, a_brake, wall_x, T=16, dt=0.5):
    """a straight candidate at constant speed ``v0`` along the lane of tests/hidden_brake_scenes.py towards a wall of key-0 cells that
    begins at ``wall_x`` and spans the road: one class whose thresholds are 0 at every sample, so a pose is hit iff its footprint
    covers a cell of the wall.  dt = 0.5 and dyadic speeds and decelerations: every speed of every manoeuvre is a dyadic number"""
    import ref_hidden_clearance as HC
    win = SC.WINDOWS[0]
    road = SC.road_raster()
    ix0, iy0, nx, ny = win
    NONE = 2 ** 31 - 1
    key = np.full((ny, nx), NONE, dtype=np.int32)
    c0 = int(round((wall_x - SC.ORIGIN[0]) / SC.CS)) - ix0
    key[:, c0:c0 + 4] = 0
    k = np.arange(T) * dt
    x = (v0 * k)[None, :]
    y = np.full((1, T), -1.75)
    head = np.stack((np.ones((1, T)), np.zeros((1, T))), -1)
    v = np.full((1, T), float(v0))
    qmin = np.asarray(HC.clearance(key, win, road, SC.ORIGIN, SC.CS, x, y, head, SC.HL, SC.HW, SC.WB, None))
    return SimpleNamespace(T=T, win=win, road=road, key=key, qmin=qmin, x=x, y=y, head=head, v=v, arc=SC.travelled_arc(x, y),
                           thr=np.zeros((1, T), dtype=np.int32), r2_cap=0, a_brake=float(a_brake), dt=dt)
