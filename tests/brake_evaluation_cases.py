"""Cases shared by tests/test_brake_evaluation_cpu.py and tests/test_brake_evaluation_gpu.py: brake evaluation (metrics/be.py,
csrc/fo_sweep_be_reduce.hpp) placed where it can go wrong.  NumPy, the two references of tests/ref_brake_evaluation.py and the
synthetic generator only; every builder is cached per process -- treat what it returns as read-only.

touch()          exact-touch cases: a standing agent whose near face sits exactly where the braked ego's front is furthest
                 along at a bisection node, and 2^-40 m to either side, for every node a bracket [0, 5] reaches, three prediction
                 lengths, a faster and a slower ego, agents with swapped dimensions and agents that touch sideways.  All inputs
                 are dyadic; the expected values come from be_exact.
known_answers()  literals: unavoidable collision, an ego at rest, ttc = 0, no collision, no prediction, bracket starts and their
                 half-even rounding, the stop rule next to its threshold, the clamp at the path end, the left knot of a
                 zero-length segment.
shapes()         rotated random geometry from synthetic.make_batch at the smallest and the oddest shapes, with be_float's
                 branch report for every active pair."""
from fractions import Fraction

import numpy as np

import ref_brake_evaluation as R

VEH = (4.5, 1.75, 1.5, 1093.3, 8.0)      # length, width, wb_rear_axle, mass, a_max: dyadic where the brake evaluation reads them
DT = 0.125
T = 31                                    # T - 1 = 30: the longest horizon the queue kernel serves
OFFSETS = (-2.0 ** -40, 0.0, 2.0 ** -40)
AGENT_KEYS = ("pos", "yaw", "v", "cov", "shape", "raw_dims", "type", "len")
METRICS = ("dce", "ttc", "be")
_CACHE = {}


def _cached(fn):
    def wrapper():
        if fn.__name__ not in _CACHE:
            _CACHE[fn.__name__] = fn()
        return _CACHE[fn.__name__]
    wrapper.__name__ = fn.__name__
    wrapper.__doc__ = fn.__doc__
    return wrapper


def agents_dict(rows, Ta):
    """rows: [(pos [Ta, 2] or (x, y), (length, width), len)] -> the agent arrays of MetricSweep.set_agents / the oracle"""
    A = len(rows)
    pos = np.zeros((A, Ta, 2))
    for k, (p, _, _) in enumerate(rows):
        pos[k] = np.asarray(p, dtype=np.float64)          # (a single point is broadcast: a standing agent)
    raw = np.array([r[1] for r in rows], dtype=np.float64).reshape(A, 2)
    return {"pos": pos, "yaw": np.zeros((A, Ta)), "v": np.zeros((A, Ta)), "cov": np.tile(0.1 * np.eye(2), (A, Ta, 1, 1)),
            "shape": raw * 1.25, "raw_dims": raw, "type": np.zeros(A, dtype=np.int32),
            "len": np.array([r[2] for r in rows], dtype=np.int32)}


def straight_rows(v0s, n=T, a=None):
    """ego rows on x = v0 dt i, y = 0, theta = 0, v = v0"""
    v0s = np.asarray(v0s, dtype=np.float64)
    x = v0s[:, None] * DT * np.arange(n)[None, :]
    z = np.zeros_like(x)
    return {"x": x, "y": z.copy(), "theta": z.copy(), "v": np.repeat(v0s[:, None], n, 1), "a": z.copy() if a is None else a}


def row(traj, m):
    return {k: v[m] for k, v in traj.items()}


def agent(agents, k):
    return {"pos": agents["pos"][k], "yaw": agents["yaw"][k], "raw_dims": agents["raw_dims"][k], "len": int(agents["len"][k])}


def exact_expected(traj, agents, veh, dt, rows=None):
    """be_exact on every pair of the given ego rows (all of them by default): decel [rows, A] as floats, NaN for len == 0"""
    rows = range(traj["x"].shape[0]) if rows is None else rows
    out = np.full((len(rows), agents["pos"].shape[0]), np.nan)
    for i, m in enumerate(rows):
        assert not traj["theta"][m].any() and np.ptp(traj["y"][m]) == 0.0
        for k in range(agents["pos"].shape[0]):
            assert not agents["yaw"][k].any()
            d, _ = R.be_exact(traj["x"][m], traj["y"][m, 0], traj["v"][m], traj["a"][m], agents["pos"][k], agents["raw_dims"][k],
                              int(agents["len"][k]), veh, dt)
            if d is not None:
                assert Fraction(float(d)) == d
                out[i, k] = float(d)
    return out


# ------------------------------------------------------------------------------------------------------------- touch
def nodes(depth=6):
    """every candidate a bisection of [0, 5] tests in its first `depth` iterations, 5 k / 2^depth; the stop rule (width < 0.1)
    ends it after the sixth"""
    assert depth <= 6 and 5.0 / 2 ** 5 >= 0.1 > 5.0 / 2 ** 6
    return [Fraction(5 * k, 2 ** depth) for k in range(1, 2 ** depth)]


def furthest(v0, d, n, dt=DT):
    """arc length of the braked ego at its last tested sample n - 1 (speeds [v0, v0, v0 - d dt, ...] >= 0, left Riemann sum)"""
    v0, d, dt = Fraction(v0), Fraction(d), Fraction(dt)
    s = Fraction(0)
    for i in range(n - 1):
        s += (v0 if i == 0 else max(v0 - d * (i - 1) * dt, Fraction(0))) * dt
    return s


def _exactly(q):
    f = float(q)
    assert Fraction(f) == q, f"{q} is not representable"
    return f


@_cached
def touch():
    """{traj [M = 66: even rows the faster, odd rows the slower ego], agents, veh, dt, meta [A], expected [2, A] (rows 0, 1),
    flips}; meta[k] = (ego kind the agent was placed for, node, prediction length, offset index, what).  The faster ego gets
    an agent at every one of the 63 nodes of depth <= 6, the slower ego only at the 15 nodes of depth <= 4 (the exact reference
    is slow); every agent is evaluated against both egos all the same."""
    length, width, wb = (Fraction(q) for q in VEH[:3])
    speeds = (8.0, 4.0)
    rows, meta = [], []
    for kind, v0 in enumerate(speeds):
        dend = Fraction(v0) * Fraction(DT) * (T - 1)
        for L in (T, T // 2, 9):
            for node in nodes(6 if kind == 0 else 4):
                stop = furthest(v0, node, L)
                if stop > dend:
                    continue                                   # the stop point lies beyond the path: the clamp decides, not the node
                shapes = [("square", (0.5, 0.5))]
                if kind == 0 and L == T and node.denominator <= 8:
                    shapes += [("long", (2.0, 0.5)), ("wide", (0.5, 2.0))]
                for what, (al, aw) in shapes:
                    for o, off in enumerate(OFFSETS):
                        centre = stop + wb + length / 2 + Fraction(al) / 2 + Fraction(off)
                        rows.append(((_exactly(centre), 0.0), (al, aw), L))
                        meta.append((kind, float(node), L, o, what))
    # sideways: the agent overlaps the ego's reach lengthwise, its near side exactly at the ego's flank (and 2^-40 m to either side)
    for L in (T, 9):
        for o, off in enumerate(OFFSETS):
            centre = furthest(8.0, Fraction(5, 2), L) + wb + length / 2 + Fraction(1, 4)
            rows.append(((_exactly(centre), _exactly(width / 2 + Fraction(1, 4) + Fraction(off))), (0.5, 0.5), L))
            meta.append((0, 2.5, L, o, "flank"))
    agents = agents_dict(rows, T)
    traj = straight_rows([speeds[m % 2] for m in range(66)])
    expected = exact_expected(traj, agents, VEH, DT, rows=(0, 1))
    flips = 0
    for k, (kind, node, L, o, what) in enumerate(meta):
        if o == 1 and meta[k + 1][:3] == (kind, node, L) and expected[kind, k] != expected[kind, k + 1]:
            flips += 1
    return {"traj": traj, "agents": agents, "veh": VEH, "dt": DT, "meta": meta, "expected": expected, "flips": flips}


# ------------------------------------------------------------------------------------------------------------- known answers
ALL_HIT = 4.921875            # six hits from [0, 5]: 2.5, 3.75, 4.375, 4.6875, 4.84375, 4.921875
ALL_MISS = 0.078125           # six misses


@_cached
def known_answers():
    """{traj, agents, veh, dt, literal [(row, agent, expected decel, what)], exact_rows, expected [M, A]}: `expected` is
    be_exact on the axis-aligned rows and be_float (under be.py:31-62's activity rule) on the one row that turns"""
    n = T
    a = np.zeros((12, n))
    brake = (-4.96, -5.0, -7.5, -1.125, -0.375, -0.625, -1.8, -1.8)
    for i, q in enumerate(brake):
        a[1 + i, 5] = q
    a[9, 5] = 2.0                                                        # accelerating only: the bracket starts at 0
    traj = straight_rows([8.0] * 12, a=a)
    # row 10: the ego at rest; row 11: the path all but ends after eight steps, the speeds say otherwise; a 13th row turns on the spot
    for k in ("x", "v"):
        traj[k][10] = 0.0
    traj["x"][11, 8:] = 8.0 + np.arange(n - 8) / 64.0    # (creeps on: a last segment of some length, which extrapolates)
    traj = {k: np.concatenate((v, np.zeros((1, n)))) for k, v in traj.items()}
    traj["theta"][12, 1:] = 1.5
    front = VEH[2] + VEH[0] / 2                                          # 3.75: the ego's front ahead of its reference point
    i = np.arange(n)
    rows = [((front + 0.5 + 0.25, 0.0), (0.5, 0.5), n),                  # 0: half a metre ahead: no deceleration up to 5 avoids it
            (np.stack((6.0 - 0.25 * i, np.zeros(n)), -1), (0.5, 0.5), n),  # 1: drives into the ego at rest (sample 8)
            ((front + 0.25, 0.0), (0.5, 0.5), n),                        # 2: touches the ego's front at sample 0: ttc = 0
            ((20.0, 6.0), (0.5, 0.5), n),                                # 3: beside the road: no collision
            ((front + 0.75, 0.0), (0.5, 0.5), 0),                        # 4: no prediction
            ((18.3046875, 0.0), (0.5, 0.5), n),                          # 5: the standing agent of the bracket-start table
            # 6, 7: the stop rule next to its threshold: from 1.8 the bracket (4.8, 4.9) is 0.1 + 5e-16 wide (goes on to 4.85),
            # (4.9, 5.0) is 0.1 - 4e-16 wide (stops at the 4.9 just tested); the agents stand where 4.875 / 4.975 would just stop
            ((float(furthest(8.0, Fraction(4.875), n)) + front + 0.25, 0.0), (0.5, 0.5), n),
            ((float(furthest(8.0, Fraction(4.975), n)) + front + 0.25, 0.0), (0.5, 0.5), n),
            # 8: crosses the road behind the end of row 11's path at sample 20: the ego, held at the end of its path whatever
            # the speeds say, is hit at every deceleration; re-sampled past the end it would have gone by
            (np.stack((np.full(n, 11.0), np.where(i >= 20, 0.0, 8.0)), -1), (0.5, 0.5), n),
            # 9: beside the ego that turns on the spot: clear of its first heading, inside its later ones -- a zero-length
            # segment keeps its LEFT knot, so no deceleration ever meets it
            ((VEH[2] * np.cos(1.5), 3.0), (0.5, 0.5), n)]
    agents = agents_dict(rows, n)
    literal = [(0, 0, ALL_HIT, "unavoidable"), (10, 1, ALL_HIT, "ego at rest, driven into"), (0, 2, 0.0, "ttc = 0"),
               (0, 3, 0.0, "no collision"), (0, 4, np.nan, "no prediction"),
               (1, 5, 4.98, "bracket from 4.96"), (2, 5, 5.0, "bracket from 5.0"), (3, 5, 6.25, "bracket from 7.5"),
               (4, 5, 2.5143750000000002, "1.125 rounds to 1.12"),
               (5, 5, 2.4734375, "0.375 rounds to 0.38"), (6, 5, 2.4678125, "0.625 rounds to 0.62"),
               (9, 5, 2.578125, "accelerating only"), (0, 5, 2.578125, "no acceleration"),
               (7, 6, 4.85, "stop rule: 0.1 + 5e-16 goes on"), (8, 7, 4.9, "stop rule: 0.1 - 4e-16 stops"),
               (11, 8, ALL_HIT, "held at the path end"), (12, 9, ALL_MISS, "left knot of a zero-length segment")]
    exact_rows = tuple(range(12))
    expected = np.full((13, len(rows)), np.nan)
    expected[:12] = exact_expected(traj, agents, VEH, DT, rows=exact_rows)
    for k in range(len(rows)):
        expected[12, k] = float_pair(row(traj, 12), agent(agents, k), VEH, DT)[0]
    return {"traj": traj, "agents": agents, "veh": VEH, "dt": DT, "literal": literal, "exact_rows": exact_rows,
            "expected": expected}


def float_pair(traj_row, ag, veh, dt):
    """be.py:31-62 on be_float: (decel, info or None); NaN without a prediction, 0 without a collision at ttc > 0"""
    if ag["len"] <= 0:
        return np.nan, None
    first, gap = R.first_contact(traj_row, ag, veh)
    assert gap > 1e-3, "a gap the reference's millimetre rounding would call a collision"
    if first is None or first == 0 or len(traj_row["x"]) < 2:
        return 0.0, None
    return R.be_float(traj_row, ag, veh, dt)


# ------------------------------------------------------------------------------------------------------------- shapes
SHAPE_DT = 0.1
# (M, A, T, Ta, seed, prediction lengths above Ta): every M of {1, 63, 64, 65, 129} (one lane, one lane short of a tile, a full
# tile, one lane in the last tile, two tiles and one lane), every A of {1, 3, 4, 5, 8, 9, 17} (idle waves in the brake kernel's
# blocks of four agents and in the reduction's eight waves), every T of {2, 3, 8, 9, 31, 33} (33: past the queue kernel's
# horizon) and Ta of {T - 3, T, T + 5} occur
SHAPES = ((1, 17, 31, 31, 1, False), (63, 1, 33, 38, 2, False), (64, 3, 9, 9, 3, False), (65, 4, 8, 5, 4, False),
          (129, 5, 31, 36, 5, False), (65, 8, 3, 3, 6, False), (64, 9, 2, 7, 7, False), (129, 17, 33, 30, 8, False),
          (63, 9, 31, 31, 9, True))


def shape_batch(M, A, T, Ta, seed, over):
    """(traj, agents, agents as the oracle takes them): synthetic.make_batch, the agents drawn into the ego's reach, a third of
    the candidates braking, every other one on a path shorter than its speeds say, some standing for their first step or throughout,
    ragged prediction lengths, all turned by an angle.  `over`: some lengths claim more samples than the table holds -- the library clamps them to Ta
    (fo_agent_rows.hpp), the oracle refuses them and is given the clamped ones"""
    from frenetix_occlusion import synthetic as S
    n = max(T, Ta)
    traj, agents = S.make_batch(M, A, T=n, dt=SHAPE_DT, config_id=100 + seed)
    traj = {k: v[:, :T].copy() for k, v in traj.items()}
    agents = {k: (v[:, :Ta].copy() if k in ("pos", "yaw", "v", "cov") else v.copy()) for k, v in agents.items()}
    p0 = agents["pos"][:, :1, :].copy()
    reach = 1.0 + 9.0 * (T - 1) * SHAPE_DT
    new0 = np.stack((3.0 + (p0[..., 0] - 6.0) / 39.0 * reach, p0[..., 1] * (5.0 / 14.0)), -1)
    agents["pos"] = new0 + (agents["pos"] - p0)
    traj["a"][::3, min(4, T - 1)] = np.minimum(traj["a"][::3, min(4, T - 1)], 0.0) - 1.237
    i = np.arange(T, dtype=np.float64)
    slow = i * (1.0 - 0.5 * i / max(T - 1, 1))           # a path that comes to rest after half the way its first speeds promise:
    for m in range(M):                                   # the constant-deceleration profile runs past its end
        if m % 2 == 1:
            for k in ("x", "y", "theta"):
                traj[k][m] = np.interp(slow, i, traj[k][m])
        if m % 5 == 2:                                  # stands for its first step: a zero-length first segment
            traj["x"][m, 1], traj["y"][m, 1] = traj["x"][m, 0], traj["y"][m, 0]
        if m % 16 == 7:                                  # stands throughout
            traj["x"][m], traj["y"][m], traj["v"][m] = traj["x"][m, 0], traj["y"][m, 0], 0.0
    hi = min(T + 2, Ta)
    pattern = (Ta, 2, Ta, 1, Ta, 0, hi, Ta - 1, Ta)
    agents["len"] = np.array([max(pattern[k % 9], 0) for k in range(A)], dtype=np.int32)
    phi = 0.1 + 0.7 * seed
    c, s = np.cos(phi), np.sin(phi)
    traj["x"], traj["y"] = c * traj["x"] - s * traj["y"], s * traj["x"] + c * traj["y"]
    px, py = agents["pos"][..., 0].copy(), agents["pos"][..., 1].copy()
    agents["pos"][..., 0], agents["pos"][..., 1] = c * px - s * py, s * px + c * py
    traj["theta"] = traj["theta"] + phi
    agents["yaw"] = agents["yaw"] + phi
    oracle_agents = agents
    if over:
        oracle_agents = dict(agents)
        agents = dict(agents)
        agents["len"] = np.where(agents["len"] == Ta, Ta + 1 + np.arange(A) % 3, agents["len"]).astype(np.int32)
    return traj, agents, oracle_agents


def shapes(O):
    """[{shape, traj, agents, veh, dt, ref (the oracle's run), active [M, A], decel (be_float on the active pairs, else the
    oracle's 0 / NaN), min_abs_sep, clamped, zero_segment [M, A]}]"""
    if "shapes" in _CACHE:
        return _CACHE["shapes"]
    from frenetix_occlusion import synthetic as S
    out = []
    for M, A, T, Ta, seed, over in SHAPES:
        traj, agents, oagents = shape_batch(M, A, T, Ta, seed, over)
        ref = O.sweep(traj, oagents, S.VEHICLE_BMW320I, SHAPE_DT, metrics=METRICS, thr={"be": 0.2})
        ttc = ref["pair_f"][..., O.PF["ttc"]]
        active = np.isfinite(ttc) & (ttc > 0) & (T >= 2)
        decel = np.where(active, np.nan, ref["pair_f"][..., O.PF["be_decel"]])
        sep = np.full((M, A), np.inf)
        clamped, zero = np.zeros((M, A), dtype=bool), np.zeros((M, A), dtype=bool)
        for m, k in np.argwhere(active):
            decel[m, k], info = R.be_float(row(traj, m), agent(oagents, k), S.VEHICLE_BMW320I, SHAPE_DT)
            sep[m, k], clamped[m, k], zero[m, k] = info["min_abs_sep"], info["clamped"], info["zero_segment"]
        out.append({"shape": (M, A, T, Ta), "traj": traj, "agents": agents, "veh": S.VEHICLE_BMW320I, "dt": SHAPE_DT, "ref": ref,
                    "active": active, "decel": decel, "min_abs_sep": sep, "clamped": clamped, "zero_segment": zero})
    _CACHE["shapes"] = out
    return out


# ------------------------------------------------------------------------------------------------- the near-touch band
# Where be_float's separating-axis test and the oracle's `quad_distance == 0` may disagree: measured by measure_band on the
# poses of the shape batches (tests/test_brake_evaluation_cpu.py holds the figure), G one decade above.  Inside the band a
# third implementation -- the device's fused arithmetic -- may sit on either side as well.
BAND_MEASURED = 2.220446049250313e-15        # ten ulps of 1.0, none beyond: 1 189 disagreements among 14 605 rectangle pairs at
                                             # measure_band's stride of 3 (what the CPU module runs), 3 553 among 42 672 at stride 1
G = 2.5e-14


def measure_band(O, batches, stride=3):
    """For every `stride`-th active pair: the ego's and the agent's rectangle at the pair's first contact, the agent pushed
    away along the line of centres until the two just touch (bisection on be_float's own separation down to the last bit of
    the shift), then 127 shifts around that point, from 1e-18 m to 9.1e-10 m to either side and 0.  Returns (the largest |sep| at
    which `sep <= 0` and the oracle's `quad_distance == 0` disagree, the number of rectangle pairs tested, the number of
    disagreements)."""
    worst, n, bad = 0.0, 0, 0
    shifts = [0.0]
    for e in range(-18, -9):
        for f in (1.0, 1.7, 2.9, 4.3, 5.9, 7.7, 9.1):
            shifts += [f * 10.0 ** e, -f * 10.0 ** e]
    shifts = np.array(shifts)
    for b in batches:
        veh, traj, ag = b["veh"], b["traj"], b["agents"]
        hlA, hwA, wb = veh[0] / 2, veh[1] / 2, veh[2]
        for m, k in np.argwhere(b["active"])[::stride]:
            i = int(b["ref"]["pair_i"][m, k, O.PI["time_dce"]])
            th, yaw = traj["theta"][m, i], ag["yaw"][k, i]
            cx, cy = traj["x"][m, i] + wb * np.cos(th), traj["y"][m, i] + wb * np.sin(th)
            p = ag["pos"][k, i]
            rl, rw = ag["raw_dims"][k]
            u = p - np.array([cx, cy])
            norm = np.hypot(*u)
            if norm == 0.0:
                continue
            u = u / norm
            sep = lambda lam: float(R._separation(np.array([cx]), np.array([cy]), np.array([th]), hlA, hwA, np.array([p[0] + lam * u[0]]),
                                                  np.array([p[1] + lam * u[1]]), np.array([yaw]), rl / 2, rw / 2)[0])
            lo, hi = 0.0, 1.0
            while sep(hi) <= 0:
                hi *= 2
            if sep(lo) > 0:
                continue                     # (a first contact the millimetre rounding made: nothing to push apart)
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if mid == lo or mid == hi:
                    break
                lo, hi = (mid, hi) if sep(mid) <= 0 else (lo, mid)
            qa = O.rect_vertices(cx, cy, th, veh[0], veh[1])
            for d in shifts:
                lam = lo + d
                s = sep(lam)
                qb = O.rect_vertices(p[0] + lam * u[0], p[1] + lam * u[1], yaw, rl, rw)
                n += 1
                if (s <= 0) != (O.quad_distance(qa, qb) == 0.0):
                    bad += 1
                    worst = max(worst, abs(s))
    return worst, n, bad
