"""The phantom predictions' exact reference (tests/ref_phantom_predictions.py) against the two CPU statements of the same stage -- the C
oracle (fo_oracle_route_predictions, fo_oracle_cv_predictions, fo_oracle_spawn_headings) and the host path
(FOAgentManager._route_prediction, _cv_prediction, _heading_towards_path) -- on the cases of tests/phantom_prediction_cases.py,
and the self-checks of those cases: every kernel form the three scenario fixtures never select is selected here, every decision
that is exact in rationals is exact in float64, and the reference alone leaves no designed case and at most 1 % of the random
slots open.  tests/test_phantom_predictions_gpu.py runs the same cases on the device."""
import os
from fractions import Fraction as Fr
from types import SimpleNamespace

import numpy as np
import pytest

import phantom_prediction_cases as C
import ref_phantom_predictions as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAUNCHES = C.launches()
IDS = [l.name for l in LAUNCHES]
WORST = {"oracle": {}, "host": {}}


def _live(launch):
    return range(launch.n_points * 3)


def _route_of(scene, ll, r):
    a, n = int(scene.first[3 * ll + r]), int(scene.count[3 * ll + r])
    return scene.xy[a:a + n], scene.s[a:a + n]


def _curve_for(launch, scene, ref, i):
    """the curve a derived heading of point i looks at: the centre line of the lanelet the reference found (mode lane_center), else
    the path"""
    lc = int(ref["center_lanelet"][i])
    if lc >= 0 and scene.center_off[lc + 1] - scene.center_off[lc] >= 2:
        return scene.center_xy[scene.center_off[lc]:scene.center_off[lc + 1]]
    return launch.path


# ------------------------------------------------------------------------------------------------ plain float64, the kernels' order
def float64_route(q, s, px, py, spd, T, dt):
    """closest segment, s0, d0, d1 and the samples' arc lengths as the kernels, the oracle and the host path evaluate them"""
    a, e = q[:-1], q[1:] - q[:-1]
    l2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    t = np.clip(((px - a[:, 0]) * e[:, 0] + (py - a[:, 1]) * e[:, 1]) / l2, 0.0, 1.0)
    cx, cy = a[:, 0] + t * e[:, 0], a[:, 1] + t * e[:, 1]
    d2 = (px - cx) * (px - cx) + (py - cy) * (py - cy)
    i = int(np.argmin(d2))
    l = np.sqrt(l2[i])
    s0 = s[i] + t[i] * l
    d0 = ((px - cx[i]) * (-e[i, 1]) + (py - cy[i]) * e[i, 0]) / l
    d1 = -0.5
    if abs(0.0 - d0) < abs(d1 - d0):
        d1 = 0.0
    if abs(0.5 - d0) < abs(d1 - d0):
        d1 = 0.5
    sk = s0 + spd * (np.arange(T, dtype=np.float64) * dt)
    return dict(seg=i, d2=d2, s0=s0, d0=d0, d1=d1, sk=sk, len=int((sk <= s[-1]).sum()))


# ------------------------------------------------------------------------------------------------ self-checks of the cases
def test_the_fixtures_feed_no_zero_length_route_segment():
    """route_polyline removes duplicate vertices, so the kernels' division by the segment length is safe on what the product
    builds (and the cases here feed none either)"""
    from frenetix_occlusion import scenario as S
    for k in (1, 2, 3):
        sc = S.load_geometry_npz(os.path.join(GOLDEN, f"scenario{k}_geometry.npz"))
        tab = S.RouteTable.from_lanelets(sc.lanelets, R=3)
        for a, n in zip(tab.first, tab.count):
            if n >= 2:
                assert np.all(np.hypot(*np.diff(tab.xy[a:a + n], axis=0).T) > 0.0), k
    for scene in (C.long_scene(), C.many_scene(), C.random_block()[0]):
        for a, n in zip(scene.first, scene.count):
            if n >= 2:
                assert np.all(np.diff(scene.s[a:a + n]) > 0.0)


def test_every_untested_form_is_selected():
    """counts over the reference's decisions: the second pass over the segments (winner index >= 64, fetched from another lane),
    routes read from global memory (nv > 256), horizons over 64 samples, more than 64 lanelets, ties, routes that end inside
    the horizon, the late quintic, d0 = +-0.25, sk == s_end, inactive slots"""
    n = dict.fromkeys(("nv>64", "nv>256", "bi>=64", "bi>=64 lane!=0", "bi>=256", "T>64", "T>64 route", "P>64", "tie", "tie same lane",
                       "tie high index in low lane", "len<T", "len=1", "len=T-1", "len=T on the end", "tau>1", "|d0|=0.25", "straight",
                       "heading bi>=64", "heading tie", "n_path>64", "lane_center", "empty route slot", "second ballot group"), 0)
    for l in LAUNCHES:
        ref = C.reference(l)
        scene = C.SCENES[l.map]()
        n["P>64"] += len(scene.polys) > 64
        n["n_path>64"] += len(l.path) > 64
        for i in range(l.n_points):
            h = ref["heading_dec"][i]
            if h is not None:
                n["heading bi>=64"] += h["seg"] >= 64
                n["heading tie"] += len(h["ties"]) > 1 and not h["same_foot"]
            n["lane_center"] += ref["center_lanelet"][i] >= 0
            n["second ballot group"] += max(ref["lanelet"][i], ref["center_lanelet"][i]) >= 64
            for r in range(3):
                d, L = ref["dec"][3 * i + r], int(ref["len"][3 * i + r])
                if d is None:
                    n["empty route slot"] += 1
                    continue
                n["T>64"] += l.T > 64
                if d["form"] == "straight":
                    n["straight"] += 1
                    continue
                t = d["ties"]
                n["nv>64"] += d["nv"] > 64; n["nv>256"] += d["nv"] > 256; n["bi>=64"] += d["seg"] >= 64
                n["bi>=64 lane!=0"] += d["seg"] >= 64 and d["seg"] % 64 != 0; n["bi>=256"] += d["seg"] >= 256
                n["T>64 route"] += l.T > 64 and L > 64
                n["tie"] += len(t) > 1; n["tie same lane"] += len(t) > 1 and t[0] % 64 == t[1] % 64
                n["tie high index in low lane"] += len(t) > 1 and t[1] % 64 < t[0] % 64
                n["len<T"] += L < l.T; n["len=1"] += L == 1 and l.T > 1; n["len=T-1"] += L == l.T - 1
                n["len=T on the end"] += L == l.T and (l.T - 1) in d["exact_k"]
                n["tau>1"] += L > 31 and l.dt >= 0.1 and d["d0"] != d["d1"]
                n["|d0|=0.25"] += d["margins"]["d0"] == 0.0
    assert all(v > 0 for v in n.values()), n
    assert n["nv>256"] >= 6 and n["bi>=64 lane!=0"] >= 10 and n["tie same lane"] >= 4 and n["tie high index in low lane"] >= 2, n
    assert sorted({l.T for l in LAUNCHES}) == [1, 2, 31, 41, 64, 65, 130]
    assert sorted({len(l.path) for l in LAUNCHES if l.map == "LONG"}) == [2, 65, 66, 129, 300]
    assert all(l.n_points < len(l.points) for l in LAUNCHES)              # every launch has slots behind *d_n_points
    # the designed answers
    ref, l = C.reference(LAUNCHES[2]), LAUNCHES[2]
    by = {t: i for i, t in enumerate(l.tags)}
    seg = lambda tag, r=0: ref["dec"][3 * by[tag] + r]["seg"]
    assert (seg("bend tie 63|64"), seg("hairpin tie 8|72"), seg("hairpin tie 9|70"), seg("hairpin tie 198|262")) == (63, 8, 9, 198)
    assert (seg("hairpin seg=72"), seg("hairpin seg=70"), seg("hairpin seg=262"), seg("nv=600 seg=598")) == (72, 70, 262, 598)
    d1 = lambda d: ref["dec"][3 * by[f"d0={d}"]]["d1"]
    assert [d1(d) for d in (-2.0, -0.5, -0.25, 0.0, 0.25, 0.5, 2.0)] == [-0.5, -0.5, -0.5, 0.0, 0.0, 0.5, 0.5]
    assert ref["len"][3 * by["beyond end"]] == 1 and ref["dec"][3 * by["before start"]]["s0"] == 0
    assert ref["yaw0"][by["ped on the curve"]] == 0.0 and ref["yaw0"][by["ped with its own orientation"]] == 1.25
    assert np.pi < ref["yaw0"][by["ped above the path: lower half plane"]] < 2 * np.pi
    assert ref["lanelet"][by["route table [1,0,0]"]] == -1 and ref["len"][3 * by["route table [1,0,0]"]] == l.T
    assert list(ref["len"][3 * by["[129,1,0]"]:3 * by["[129,1,0]"] + 3]) == [l.T, 0, 0]
    many = [x for x in LAUNCHES if x.map == "MANY"][0]
    got = dict(zip(many.tags, np.maximum(C.reference(many)["lanelet"], C.reference(many)["center_lanelet"])[:many.n_points]))
    assert [got[t] for t in ("lanelet 0", "lanelet 63", "lanelet 64", "lanelet 129", "overlap 3|70 -> 3", "overlap 64|100 -> 64",
                             "70 alone", "100 alone", "on none", "ped lane_center 64|100")] == [0, 63, 64, 129, 3, 64, 70, 100, -1, 64]


def test_open_decisions_stay_under_their_caps():
    """no designed case is open; the random block leaves out at most 1 % of its slots (here: none)"""
    n_random = n_open = 0
    for l in LAUNCHES:
        ref = C.reference(l)
        opened = [(l.tags[s // 3], s % 3) for s in _live(l) if ref["status"][s] == "open"]
        if l.designed:
            assert not opened, (l.name, opened)
        else:
            n_random += sum(ref["dec"][s] is not None for s in _live(l))
            n_open += len(opened)
    assert n_random >= 200 and n_open <= 0.01 * n_random, (n_random, n_open)


@pytest.mark.parametrize("launch", LAUNCHES, ids=IDS)
def test_float64_agrees_with_the_rationals(launch):
    """settled and exact decisions: plain float64 takes the reference's segment, d1 and length; where a margin is 0 in rationals
    (a tie of two segments, |d0| = 0.25, a sample exactly on the route's end or on a vertex) float64 gives the rational value
    bit for bit, so the tie is a tie on the device as well"""
    ref, scene = C.reference(launch), C.SCENES[launch.map]()
    n_exact = 0
    for s_ in _live(launch):
        d = ref["dec"][s_]
        if d is None or d["form"] != "route" or ref["status"][s_] == "open":
            continue
        i, r = divmod(s_, 3)
        q, s = _route_of(scene, int(ref["lanelet"][i]), r)
        ti = {C.CAR: 0, C.BIKE: 1}[int(launch.points[i, 0])]
        px, py, spd = launch.points[i, 1], launch.points[i, 2], launch.types["speed"][ti]
        f = float64_route(q, s, px, py, spd, launch.T, launch.dt)
        tag = (launch.name, launch.tags[i], r)
        assert (f["seg"], f["d1"], f["len"]) == (d["seg"], d["d1"], int(ref["len"][s_])), tag
        if ref["status"][s_] != "exact":
            continue
        n_exact += 1
        m = d["margins"]
        if m["d2"] == 0.0:
            for j in d["ties"]:
                assert Fr(float(f["d2"][j])) == d["d2"], (tag, "d2", j)
        if m["d0"] == 0.0:
            assert Fr(float(f["d0"])) == d["d0"] and abs(f["d0"]) == 0.25, (tag, "d0")
        for k in d["exact_k"]:
            assert Fr(float(f["s0"])) == d["s0"], (tag, "s0")
            assert Fr(float(f["sk"][k])) == d["s0"] + Fr(float(spd)) * k * Fr(float(launch.dt)), (tag, "sk", k)
    if launch.map == "LONG":
        assert n_exact > 0


# ------------------------------------------------------------------------------------------------ reference against the C oracle
@pytest.mark.parametrize("launch", LAUNCHES, ids=IDS)
def test_oracle_against_the_reference(oracle, launch):
    ref, scene = C.reference(launch), C.SCENES[launch.map]()
    n, T = launch.n_points, launch.T
    pts = launch.points[:n]
    types = pts[:, 0].astype(np.int32)
    ti = np.where(types == C.CAR, 0, np.where(types == C.BIKE, 1, 2))
    speed = np.asarray(launch.types["speed"])[ti]
    yaw = pts[:, 3].copy()
    for i in range(n):                      # derived headings: fo_oracle_spawn_headings on the curve the reference's lanelet names
        if ref["heading_dec"][i] is not None:
            yaw[i] = oracle.spawn_headings(pts[i:i + 1, 1:3], np.array([C.PED], dtype=np.int32), _curve_for(launch, scene, ref, i))[0]
            dev = abs(yaw[i] - ref["yaw0"][i])
            WORST["oracle"]["yaw0"] = max(WORST["oracle"].get("yaw0", 0.0), dev)
            assert dev <= 1e-12, (launch.name, launch.tags[i], dev)
    pos, yl, vl, cov, ln = oracle.route_predictions(pts[:, 1:3], types, speed, ref["lanelet"][:n], 3, scene.first, scene.count, scene.xy,
                                                    scene.s, yaw, T, launch.dt, C.VAR0, C.FACTOR)
    got = dict(pos=pos, yaw=yl, v=vl, cov=cov.reshape(-1, T, 4), len=ln)
    C.compare(launch, ref, got, "oracle", _live(launch), WORST["oracle"])
    straight = [i for i in range(n) if ref["dec"][3 * i] is not None and ref["dec"][3 * i]["form"] == "straight"]
    if straight:                            # the straight form's own entry point
        p2, y2, v2, c2 = oracle.cv_predictions(pts[straight, 1:3], yaw[straight], speed[straight], T, launch.dt, C.VAR0, C.FACTOR)
        S = len(ref["len"])
        full = dict(pos=np.zeros((S, T, 2)), yaw=np.zeros((S, T)), v=np.zeros((S, T)), cov=np.ones((S, T, 4)), len=np.zeros(S, dtype=np.int32))
        for j, i in enumerate(straight):
            full["pos"][3 * i], full["yaw"][3 * i], full["v"][3 * i], full["cov"][3 * i], full["len"][3 * i] = p2[j], y2[j], v2[j], c2[j].reshape(T, 4), T
            vx = ref["dec"][3 * i]["vxy"]
            if T > 1 and ref["status"][3 * i] != "open":          # the rounded velocity, read off the first step
                assert np.allclose((p2[j, 1] - p2[j, 0]) / launch.dt, vx, rtol=0, atol=1e-9), (launch.tags[i], vx)
        C.compare(launch, ref, full, "oracle cv", [3 * i for i in straight], WORST["oracle"])


# ------------------------------------------------------------------------------------------------ reference against the host path
CFG = {"pedestrian": {"width": 0.5, "length": 0.3, "default_velocity": 1.4}, "bicycle": {"width": 0.9, "length": 2.0, "default_velocity": 5.0},
       "car": {"width": 2.0, "length": 4.8, "default_velocity": 10.0},
       "prediction": {"variance_factor": C.FACTOR, "size_factor_length_s": 1.2, "size_factor_width_s": 1.3, "size_factor_length_l": 1.4,
                      "size_factor_width_l": 2.5}}
NAMES = {C.CAR: "Car", C.BIKE: "Bicycle", C.PED: "Pedestrian"}


@pytest.mark.parametrize("launch", LAUNCHES, ids=IDS)
def test_host_path_against_the_reference(launch):
    """FOAgentManager's own methods on the same routes and curves (the lanelet a point lies on is the reference's decision: the
    host finds it with the same crossing-number test, tests/test_scene_pointwise.py)"""
    pytest.importorskip("torch")
    from frenetix_occlusion.agent import FOAgentManager, PhantomAgent
    ref, scene = C.reference(launch), C.SCENES[launch.map]()
    T = launch.T
    am = FOAgentManager(SimpleNamespace(obstacles=[]), launch.path, CFG, 0, dt=launch.dt, device="cpu")
    horizon = (T - 1 + 0.5) * launch.dt
    S = len(ref["len"])
    got = dict(pos=np.zeros((S, T, 2)), yaw=np.zeros((S, T)), v=np.zeros((S, T)), len=np.zeros(S, dtype=np.int32))
    slots = []
    for i in range(launch.n_points):
        typ = int(launch.points[i, 0])
        ti = {C.CAR: 0, C.BIKE: 1, C.PED: 2}[typ]
        p = launch.points[i, 1:3].copy()
        yaw = float(launch.points[i, 3])
        if ref["heading_dec"][i] is not None:
            yaw = am._heading_towards_path(p, _curve_for(launch, scene, ref, i))
            dev = abs(yaw - ref["yaw0"][i])
            WORST["host"]["yaw0"] = max(WORST["host"].get("yaw0", 0.0), dev)
            assert dev <= 1e-12, (launch.name, launch.tags[i], dev)
        ag = PhantomAgent(1, NAMES[typ], p, yaw, launch.types["speed"][ti], launch.types["raw_l"][ti], launch.types["raw_w"][ti])
        for r in range(3):
            d = ref["dec"][3 * i + r]
            if d is None:
                continue
            if d["form"] == "straight":
                pr = am._cv_prediction(ag, horizon)
            else:
                ag.initial_orientation = float(ref["yaw0"][i])
                pr = am._route_prediction(ag, horizon, _route_of(scene, int(ref["lanelet"][i]), r)[0])
            s_ = 3 * i + r
            L = len(pr["pos_list"])
            got["pos"][s_, :L], got["yaw"][s_, :L], got["v"][s_, :L], got["len"][s_] = pr["pos_list"], pr["orientation_list"], pr["v_list"], L
            slots.append(s_)
            if ref["status"][s_] != "open":
                c = pr["cov_list"].reshape(L, 4)
                assert np.all(c[:, 1:3] == 0.0)
                rel = float(np.abs(c[:, (0, 3)] / ref["cov"][s_, :L][:, (0, 3)] - 1.0).max())
                WORST["host"]["cov"] = max(WORST["host"].get("cov", 0.0), rel)
                assert rel <= C.COV_RTOL
                assert (pr["shape"]["length"], pr["shape"]["width"]) == tuple(ref["shape"][s_])
    C.compare(launch, ref, got, "host", slots, WORST["host"])


def test_worst_deviations_are_those_of_the_design_table(capsys):
    """(runs last in the module) the largest deviations from the reference seen above -- the figures of DESIGN.md's table of the
    prediction stage; printed with -s"""
    for who, w in WORST.items():
        print(who, {k: f"{v:.3g}" for k, v in w.items()})
        for k, v in w.items():
            assert v <= {"pos": 1e-9, "yaw": 1e-12, "v": 1e-12, "yaw0": 1e-12, "cov": 1e-13}[k]
