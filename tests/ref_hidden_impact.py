"""Plain-Python statement of the hidden-traffic impact verdict (DESIGN.md §5.10 "Impact verdict", include/fo_hip.h
fo_scene_hidden_brake_impact), written from its definition -- not from the product code.  The walk is tests/ref_hidden_brake_users.py's,
taken whole: the stage is defined on what fo_scene_hidden_brake_users writes (``brake_first``, ``stop``, ``first``) and on ``v``.  What is
stated here is steps 1 - 7 -- plain loops over lists -- and the harm rows of the definition."""
import math

import numpy as np

NOT_FINITE = -2
C_SAFE, C_RES0, C_RES1, NC = 12, 14, 15, 16      # FO_C_SAFE, FO_C_RES0, FO_C_RES1, FO_NC (include/fo_hip.h)
OPEN_TOL = 1e-9                                  # the float tolerance of the harm values: a choice between closer harms is open

# the reference's tables by type (metrics/utils/harm_model.py:15-32, 158-190), by lower-case type name
PROTECTED = {"car": True, "truck": True, "bus": True, "bicycle": False, "pedestrian": False, "priorityvehicle": True,
             "parkedvehicle": True, "train": True, "motorcycle": False, "taxi": True, "unknown": False}
COEFF = dict(lr4s_const=-4.457, lr4s_speed=0.177, lr4s_side=0.244, lr4s_rear=-0.431, lr1s_const=-4.591, lr1s_speed=0.185,
             ped_const=3.164, ped_speed=0.288)   # harm_params.json as shipped


def mass(kind, size):
    kind = kind.lower()
    if kind in ("car", "priorityvehicle", "parkedvehicle", "taxi"):
        return -1333.5 + 526.9 * size ** 0.8
    return {"truck": 25000.0, "bus": 13000.0, "bicycle": 90.0, "pedestrian": 75.0, "train": 118800.0, "motorcycle": 250.0}.get(kind, 0.0)


def row(kind, length, width, ego_mass, coeff=COEFF):
    """(p0, p1, p2, p3) of a road user: the reference's harm head-on (dv = v_ego + v_obs) and at the worst area of impact"""
    protected = PROTECTED[kind.lower()]          # (a type without a protection entry has no row: KeyError)
    m_obs = mass(kind, float(length) * float(width))
    split_ego, split_obst = m_obs / (ego_mass + m_obs), ego_mass / (ego_mass + m_obs)
    if protected:
        area = max(0.0, coeff["lr4s_side"], coeff["lr4s_rear"])
        return (-coeff["lr4s_const"] - area, -coeff["lr4s_speed"] * split_obst, -coeff["lr4s_const"] - area, -coeff["lr4s_speed"] * split_ego)
    return (coeff["ped_const"], -coeff["ped_speed"] * split_obst, -coeff["lr1s_const"], -coeff["lr1s_speed"] * split_ego)


def logistic(p_const, p_speed, w):
    return 1.0 / (1.0 + math.exp(p_const + p_speed * w))


def speed_one(first, brake_first, stop, v, a_brake, dt, ends):
    """steps 1 - 3 for one (class, trajectory): ``brake_first``, ``stop``, ``v`` the rows over b / k -> (speed, at)"""
    best, at = -math.inf, -1
    for b in range(ends):
        bf, st = int(brake_first[b]), int(stop[b])
        met = 0 <= first <= b
        if not (met or 0 <= bf < st):                                                   # 1.
            continue
        left = float(v[b]) - a_brake * ((bf - b) * dt)
        u = float(v[first]) if met else (left if left > 0.0 else 0.0)                   # 2. (a NaN speed: fmax's 0)
        if u > best:                                                                    # 3.: ascending b, the lowest start stays
            best, at = u, b
    return (best, at) if at >= 0 else (0.0, -1)


def choose(speed, at, rows, speed_of, finite=True):
    """steps 4 - 6 for one trajectory: (obstacle harm, ego harm, user, open) -- ``open``: the best and the second-best obstacle harm
    differ by less than OPEN_TOL and do not come from the same (row, w)"""
    best, harm, user, cands = -1.0, (0.0, 0.0), -1, []
    for c in range(len(at)):
        if at[c] < 0:
            continue
        w = float(speed[c]) + float(speed_of[c])
        ho, he = logistic(rows[c][0], rows[c][1], w), logistic(rows[c][2], rows[c][3], w)
        cands.append((ho, tuple(float(p) for p in rows[c]), w))
        if ho > best:
            best, harm, user = ho, (ho, he), c
    is_open = False
    if len(cands) > 1 and finite:
        cands.sort(key=lambda t: -t[0])
        (h0, r0, w0), (h1, r1, w1) = cands[0], cands[1]
        is_open = abs(h0 - h1) < OPEN_TOL and (r0, w0) != (r1, w1)
    if not finite:                                                                      # 6.
        harm, user = (1.0, 1.0), NOT_FINITE
    return harm[0], harm[1], user, is_open


def fold_row(cost_row, safe, obst_harm, user, harm_limit):
    """step 7 for one trajectory: (cost row [16] as a list of floats, safe) -> the new pair; nothing but the three columns changes"""
    out = list(cost_row)
    out[C_RES0], out[C_RES1] = float(obst_harm), float(user)
    if obst_harm > harm_limit or user == NOT_FINITE:
        safe, out[C_SAFE] = 0, 0.0
    return out, safe


def impact(brake_first, stop, first, v, a_brake, dt, B, rows, speed_of, lens=None, finite=None):
    """steps 1 - 6 over what fo_scene_hidden_brake_users wrote (``brake_first [C, M, T]``, ``stop [M, T]``, ``first [C, M]``) and
    ``v [M, T]``: (harm [M, 2], user [M], speed [C, M], at [C, M], open cases)"""
    brake_first, stop, first, v = np.asarray(brake_first), np.asarray(stop), np.asarray(first), np.asarray(v, dtype=np.float64)
    C, M, T = brake_first.shape
    harm, user = np.zeros((M, 2)), np.full(M, -1, dtype=np.int32)
    speed, at = np.zeros((C, M)), np.full((C, M), -1, dtype=np.int32)
    n_open = 0
    for m in range(M):
        Lm = T if lens is None else min(max(int(lens[m]), 0), T)
        ends = min(int(B), Lm)
        for c in range(C):
            speed[c, m], at[c, m] = speed_one(int(first[c, m]), brake_first[c, m], stop[m], v[m], float(a_brake), float(dt), ends)
        ho, he, user[m], is_open = choose(speed[:, m].tolist(), at[:, m].tolist(), rows, speed_of, True if finite is None else bool(finite[m]))
        harm[m] = (ho, he)
        n_open += bool(is_open)
    return harm, user, speed, at, n_open


def fold(cost, safe, harm, user, harm_limit):
    """step 7 over cost [M, 16] / safe [M]: copies with the fold applied"""
    cost, safe = np.array(cost, dtype=np.float64), np.array(safe, dtype=np.uint8)
    for m in range(len(safe)):
        out, safe[m] = fold_row(cost[m].tolist(), int(safe[m]), float(harm[m][0]), int(user[m]), harm_limit)
        cost[m] = out
    return cost, safe
