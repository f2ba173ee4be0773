"""Hidden-traffic brake clearance by road users on the CPU (DESIGN.md §5.10 "Brake clearance by road users"): the checker
tests/ref_hidden_brake_users.py is held to the tie -- row c is tests/ref_hidden_brake_classes.py on the map of class c with the single
threshold row of class c --, to conditions that keep the scenes from being degenerate (the forecasts differ at one speed, so a walk that
read one map for every class fails) and to hand cases for map_of; the host layer runs on CPU tensors, the ctypes mirror and the launch
plan are held to the header and to csrc by a host compiler.  Every comparison is between integers and exact."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_classes_scenes as CS
import hidden_brake_scenes as SC
import hidden_brake_users_scenes as US
import ref_hidden_brake_classes as BCL
import ref_hidden_brake_users as BU
import ref_hidden_clearance as HC
import test_hidden_brake_classes_cpu as CC
import test_hidden_brake_cpu as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = [spec for spec in SC.RANDOM_SCENES if 31 <= spec[2] <= 65]
_cache = {}


def _users(sc, keys=None, qmins=None, thr=None, map_of=None):
    return BU.brake_users(sc.keys if keys is None else keys, sc.win, sc.road, sc.qmins if qmins is None else qmins, SC.ORIGIN, SC.CS, sc.x,
                          sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB, sc.a_brake, sc.dt, sc.thr if thr is None else thr,
                          sc.map_of if map_of is None else map_of, sc.lens)


def _classes(sc, key, qmin, thr):
    return BCL.brake_classes(key, sc.win, sc.road, qmin, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB, sc.a_brake,
                             sc.dt, thr, sc.lens)


def solved(spec):
    """the scene of ``spec`` with the five users of hidden_brake_users_scenes.USERS on their three maps and the users checker's outputs
    -- computed once, shared by the tests below, never changed"""
    if spec not in _cache:
        sc = US.user_scene(spec)
        _cache[spec] = (sc, _users(sc))
    return _cache[spec]


# ------------------------------------------------------------------------------------------------ 1. the tie on the checkers
def test_users_of_the_scenes():
    assert US.maps_of(US.USERS) == ([("road", "any"), ("road", "lanes"), ("euclid", "any")], [0, 1, 0, 2, 1])
    assert len(LONG) == 17 and {spec[2] for spec in LONG} == {31, 32, 33, 64, 65}
    sc = solved(LONG[0])[0]
    assert [u[0] for u in sc.users] == [1.5, 4.0, 4.0, 4.0, 8.0] and len(sc.keys) == len(sc.qmins) == 3
    assert sc.r2_caps == [int(sc.tables[2][-1]), int(sc.tables[4][-1]), int(sc.tables[3][-1])]
    assert all(int(sc.thr[c, -1]) <= 169 * sc.r2_caps[k] for c, k in enumerate(sc.map_of))


@pytest.mark.parametrize("spec", LONG, ids=lambda s: "-".join(str(v) for v in s))
def test_checker_equals_the_classes_checker_row_by_row(spec):
    """the scenes of tests/hidden_brake_scenes.RANDOM_SCENES with 31 <= T <= 65, every one under all three forecasts: row c of every
    output is ref_hidden_brake_classes.brake_classes on (key, qmin) of the map of class c with the single row thr[c]"""
    sc, (bf, st, commit, first) = solved(spec)
    C_ = len(sc.users)
    assert bf.shape == (C_, sc.M, sc.T) and st.shape == (sc.M, sc.T) and commit.shape == first.shape == (C_, sc.M)
    assert all(a.dtype == np.int32 for a in (bf, st, commit, first))
    for c, k in enumerate(sc.map_of):
        bf_c, st_c, commit_c, first_c = _classes(sc, sc.keys[k], sc.qmins[k], sc.thr[c:c + 1])
        assert np.array_equal(bf[c], bf_c[0]), (c, np.argwhere(bf[c] != bf_c[0])[:4].tolist())
        assert np.array_equal(st, st_c), c
        assert np.array_equal(commit[c], commit_c[0]), (c, np.argwhere(commit[c] != commit_c[0])[:4].tolist())
        assert np.array_equal(first[c], first_c[0]), c
        assert np.array_equal(first[c], HC.reach_from_qmin(sc.qmins[k], sc.tables[c])[1]), c


@pytest.mark.parametrize("spec", [LONG[0], LONG[4], LONG[9]], ids=lambda s: "-".join(str(v) for v in s))
def test_one_map_is_the_classes_checker_outright(spec):
    """K = 1: the whole result is ref_hidden_brake_classes' on the same inputs, for each of the three maps in turn"""
    sc = solved(spec)[0]
    for k in range(3):
        cap = 169 * sc.r2_caps[k]
        thr = sc.thr[[c for c in range(len(sc.users)) if int(sc.thr[c, -1]) <= cap]]
        assert len(thr) >= 2
        got = _users(sc, keys=[sc.keys[k]], qmins=[sc.qmins[k]], thr=thr, map_of=[0] * len(thr))
        ref = _classes(sc, sc.keys[k], sc.qmins[k], thr)
        assert all(np.array_equal(g, r) and g.dtype == r.dtype for g, r in zip(got, ref)), k


def test_scenes_are_not_degenerate():
    """by the checker alone.  Users 1, 2 and 3 move at the same 4 m/s along the lanes, along the road and as the crow flies: in scene
    (31, 7, 31) both pairs of forecasts differ in commit AND in brake_first for some candidate, in scene (35, 70, 31) the lanes differ
    from the road for at least 10 candidates (18 when the scenes were written), in scene (52, 4, 33) the road differs from the
    straight line; every kind of commit is there.  A walk that read one map for every class cannot give these rows"""
    _, (bf, _, commit, _) = solved((31, 7, 31, 2, False))
    assert (commit[1] != commit[2]).any() and (bf[1] != bf[2]).any(), "lanes against road"
    assert (commit[2] != commit[3]).any() and (bf[2] != bf[3]).any(), "road against euclid"
    _, (bf, _, commit, _) = solved((35, 70, 31, 1, True))
    print("scene 35:", int((commit[1] != commit[2]).sum()), int((bf[1] != bf[2]).sum()))
    assert (commit[1] != commit[2]).sum() >= 10 and (bf[1] != bf[2]).sum() >= 100
    _, (bf, _, commit, _) = solved((52, 4, 33, 2, False))
    assert (commit[2] != commit[3]).any() and (bf[2] != bf[3]).sum() >= 20
    seen = np.concatenate([solved(spec)[1][2].ravel() for spec in LONG[:5]])
    assert (seen == -1).sum() >= 20 and (seen == 0).sum() >= 20 and (seen > 0).sum() >= 20
    # and the same map under two names gives the same rows: what differs above is the forecast, nothing else
    sc = solved((31, 7, 31, 2, False))[0]
    twice = _users(sc, keys=[sc.keys[0], sc.keys[1], sc.keys[0]], qmins=[sc.qmins[0], sc.qmins[1], sc.qmins[0]], thr=sc.thr[[2, 1, 2]], map_of=[0, 1, 2])
    assert np.array_equal(twice[0][0], twice[0][2]) and np.array_equal(twice[2][0], twice[2][2]) and (twice[0][0] != twice[0][1]).any()


# ------------------------------------------------------------------------------------------------ 2. hand cases
# The hand road of tests/test_hidden_brake_classes_cpu.py: 5 x 60 cells of 1 m, hidden from column 40 on, dt = 0.5 s, no margin; the
# ego holds exactly the cell of column k at x = k + 0.5.  Map A is its Euclidean key map (169 D^2, D cells in front of the stretch).
# Map B is the map of a road whose hidden stretch begins ten columns farther on (column 50): B(k) = A(k - 10).
def _hand_maps(T, speeds, x, y, head):
    tables = CS.reach_tables(speeds, T, CC.H_DT, 0.0, CC.H_CS)
    r2_cap = max(int(t[-1]) for t in tables)
    cls_b = np.full((5, 60), 3, dtype=np.uint8)
    cls_b[:, 50:] = 5
    keys = [HC.key_map(cls, CC.H_WIN, CC.H_ROAD, r2_cap)[0] for cls in (CC.H_CLS, cls_b)]
    qmins = [HC.clearance(k, CC.H_WIN, CC.H_ROAD, CC.H_ORIGIN, CC.H_CS, x, y, head, CC.H_HL, CC.H_HW, CC.H_WB) for k in keys]
    return keys, qmins, CS.thresholds(tables)


def _hand(speeds, map_of, order=(0, 1)):
    """8 m/s from x = 0.5 braking at 4 m/s^2 (the classes test's first hand case) against ``speeds`` on maps (A, B)[order]"""
    v = np.full((1, 10), 8.0)
    x = 0.5 + np.concatenate(([0.0], np.cumsum(v[0, :-1] * CC.H_DT)))[None]
    y = np.full((1, 10), 2.5)
    head = np.zeros((1, 10, 2))
    head[..., 0] = 1.0
    keys, qmins, thr = _hand_maps(10, speeds, x, y, head)
    keys, qmins = [keys[k] for k in order], [qmins[k] for k in order]
    bf, st, commit, first = BU.brake_users(keys, CC.H_WIN, CC.H_ROAD, qmins, CC.H_ORIGIN, CC.H_CS, x, y, head, SC.travelled_arc(x, y), v, CC.H_HL,
                                           CC.H_HW, CC.H_WB, 4.0, CC.H_DT, thr, map_of)
    assert st[0].tolist() == [4, 5, 6, 7, 8, 9, 10, 10, 10, 10]
    return first[:, 0].tolist(), bf[:, 0].tolist(), commit[:, 0].tolist()


# the rows of the classes test's hand case on map A, written down there: 8 m/s and 4 m/s hidden
A8 = (5, [8, 7, 6, 6, 5, 6, 7, 8, 9, -1], 3)
A4 = (7, [-1, -1, -1, 9, 8, 7, 7, 8, 9, -1], 5)
# On map B the stretch begins 10 cells farther on.  The manoeuvre from b is 4, 7, 9 cells beyond column 4 b while it moves and stands 10
# beyond it from sample b + 4 (the classes test's words).
# 8 m/s hidden (4 cells a sample): the candidate is met when 50 - 4 k <= 4 k, first = 7 (22 <= 28).  From b = 0 the ego stands in column
# 10, 40 cells short: never within the horizon.  From b = 1, 2, 3 it stands in columns 14, 18, 22 and is met there at samples 9, 8, 7
# (36 <= 36, 32 <= 32, 28 <= 28) -- standing, not counted.  From b = 4 it is in columns 20, 23, 25 at samples 5, 6, 7: 30 > 20, 27 > 24,
# 25 <= 28: brake_first = 7 < stop = 8, commit = 4.  From b = 5 column 27 at sample 7 (23 <= 28), from b = 6, 7, 8 the first pose.
B8 = (7, [-1, 9, 8, 7, 7, 7, 7, 8, 9, -1], 4)
# 4 m/s hidden (2 cells a sample): first = 9 (50 - 36 = 14 <= 18).  From b <= 4 the ego stands 40 .. 24 cells short (at most 18 are
# reached), from b = 5 it is in column 30 at sample 9 (20 > 18).  From b = 6 columns 28, 31, 33 at samples 7, 8, 9: 22 > 14, 19 > 16,
# 17 <= 18: brake_first = 9 < stop = 10, commit = 6.  From b = 7 column 35 at sample 9 (15 <= 18), from b = 8 column 36.
B4 = (9, [-1, -1, -1, -1, -1, -1, 9, 9, 9, -1], 6)


def test_map_of_permutations_by_hand():
    first, bf, commit = _hand((8.0, 4.0), (0, 0))
    assert (first[0], bf[0], commit[0]) == A8 and (first[1], bf[1], commit[1]) == A4
    first, bf, commit = _hand((8.0, 8.0, 4.0), (1, 0, 1))
    assert (first[1], bf[1], commit[1]) == A8
    assert (first[0], bf[0], commit[0]) == B8
    assert (first[2], bf[2], commit[2]) == B4
    # the same users with the maps handed over the other way round and map_of turned with them: the same rows
    again = _hand((8.0, 8.0, 4.0), (0, 1, 0), order=(1, 0))
    assert again == (first, bf, commit)
    # every class on B, every class on A, and a map no class names
    first, bf, commit = _hand((8.0, 4.0), (1, 1))
    assert (first[0], bf[0], commit[0]) == B8 and (first[1], bf[1], commit[1]) == B4
    first, bf, commit = _hand((4.0, 8.0), (0, 0), order=(0, 1))
    assert (first[0], bf[0], commit[0]) == A4 and (first[1], bf[1], commit[1]) == A8


def test_a_single_map_reader_would_fail_the_hand_case():
    """what separates the maps is in the expectations themselves: the same speed on A and on B has different rows"""
    assert A8 != B8 and A8[2] < B8[2] and A8[0] < B8[0] and A4 != B4 and A4[2] < B4[2]


# ------------------------------------------------------------------------------------------------ 3. the host layer
def _result(torch, users, commit, stop=None, lengths=None):
    from frenetix_occlusion.hidden_traffic import HiddenBrakeUsers
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.int32))
    C_, M = np.shape(commit)
    stop = [[1] * 4] * M if stop is None else stop
    return HiddenBrakeUsers((), tuple(users), tuple(range(C_)), np.zeros((C_, 4), dtype=np.int32), torch.zeros((C_, M, 4), dtype=torch.int32),
                            t(stop), t(commit), t(commit), None, 4.0, 0.1, lengths)


def test_critical_user_and_decided_until():
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import HiddenBrake, HiddenBrakeUsers
    from frenetix_occlusion.sensor_model import HiddenBrakeUsers as exported
    assert exported is HiddenBrakeUsers
    users = ((7.0, "road", "lanes"), (2.0, "road", "any"), (13.9, "road", "lanes"), (2.0, "euclid", "any"))
    commit = [[-1, 3, -1, 0, -1, 5], [-1, 2, 5, -1, -1, -1], [-1, 0, -1, 0, 4, -1], [-1, -1, 1, -1, -1, -1]]
    out = _result(torch, users, commit)
    cu, vc = out.critical_user(), out.critical_speed()
    assert cu.dtype == torch.int64 and cu.tolist() == [-1, 1, 1, 0, 2, 0]       # equal speeds: the lower index, user 1 before user 3
    assert vc.dtype == torch.float64 and vc.tolist() == [float("inf"), 2.0, 2.0, 7.0, 13.9, 7.0]
    only3 = _result(torch, users, [[-1], [-1], [-1], [6]])
    assert only3.critical_user().tolist() == [3] and only3.critical_speed().tolist() == [2.0]
    one = _result(torch, users[:1], [[-1, 0]])
    assert one.critical_user().tolist() == [-1, 0] and one.critical_speed().tolist() == [float("inf"), 7.0]
    stop = [[2, 3, 4, 4], [4, 4, 4, 4], [1, 2, 3, -1]]
    lengths = torch.as_tensor(np.array([4, 9, 3], dtype=np.int32))
    out = _result(torch, users[:1], [[-1, 0, 1]], stop, lengths)
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.int32))
    assert out.decided_until().tolist() == HiddenBrake(None, None, t(stop), None, None, 4.0, 0.1, lengths).decided_until().tolist() == [2, 0, 2]


def test_refusals_and_calls_in_their_order(monkeypatch):
    torch = pytest.importorskip("torch")
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import hidden_traffic
    from frenetix_occlusion.sensor_model import SensorModel
    assert SensorModel.__dict__["hidden_brake_users"] is hidden_traffic.hidden_brake_users
    assert (N.HIDDEN_BRAKE_MAX_MAPS, N.HIDDEN_BRAKE_MAX_CLASSES, N.HIDDEN_BRAKE_MAX_TABLE) == (3, 8, 896)
    monkeypatch.setattr(N, "current_stream", lambda index=None: None)
    passes = []
    plain = hidden_traffic.unit_headings
    monkeypatch.setattr(hidden_traffic, "unit_headings", lambda theta: passes.append(1) or plain(theta))
    z = np.zeros((2, 31))
    kw = dict(vehicle=SC.VEH, dt=0.1)
    bad_v = np.zeros((2, 30))
    ped, cyc, car = (2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes")
    # 1. its own refusals, before the model is looked at and with everything else wrong too: the count, the names, the speeds, the table
    none = SimpleNamespace(window=None, cell_size=SC.CS)
    call = lambda sm, users, x=z, v=bad_v, **more: SensorModel.hidden_brake_users(sm, x, x, x, v, users=users, a_brake=-1.0, **kw, **more)
    for users, text in ((((2.0, "road"),), r"users\[0\] = \(2\.0, 'road'\) is no triple"), ((ped, ("fast", "road", "any")), r"users\[1\] = \('fast', 'road', 'any'\) is no triple"),
                        ((ped, 7.0), r"users\[1\] = 7\.0 is no triple")):
        with pytest.raises(ValueError, match=r"^hidden_brake_users: " + text + r" \(speed, metric, flow\) with a number for the speed$"):
            call(none, users)
    for users in ((), (ped,) * 9, None, 5):
        with pytest.raises(ValueError, match=r"^hidden_brake_users: users must hold 1 \.\. 8 triples \(speed, metric, flow\)$"):
            call(none, users)
    with pytest.raises(ValueError, match=r"^hidden_brake_users: users\[1\]: metric 'manhattan', one of \('euclid', 'road'\) is possible$"):
        call(none, (ped, (float("nan"), "manhattan", "lanes")))
    with pytest.raises(ValueError, match=r"^hidden_brake_users: users\[0\]: flow 'left', one of \('any', 'lanes'\) is possible$"):
        call(none, ((-1.0, "road", "left"),))
    with pytest.raises(ValueError, match=r"^hidden_brake_users: users\[2\]: flow 'lanes' follows the lanes along the road: it needs metric 'road'"):
        call(none, (ped, cyc, (7.0, "euclid", "lanes")))
    for s in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^hidden_brake_users: the users' speeds must be finite and >= 0$"):
            call(none, (ped, (s, "road", "any")))
    long = np.zeros((2, 113))
    with pytest.raises(ValueError, match=r"^hidden_brake_users: 8 users x 113 samples = 904 thresholds, at most 896 are possible"):
        call(none, (ped,) * 8, x=long)
    # 2. then each clearance's, in its words -- the first map's before anything ran, a later one's after the earlier ones ran
    with pytest.raises(RuntimeError, match=r"^hidden_clearance needs the cell classes of a previous launch\(\)$"):
        call(none, (ped, cyc))
    sm = BC._cpu_model(torch)
    with pytest.raises(ValueError, match=r"^hidden_clearance: lengths must be \[M\]$"):
        call(sm, (ped, cyc), lengths=np.zeros(3))
    assert sm.ctx.calls == []
    with pytest.raises(RuntimeError, match=r"^hidden_clearance: flow 'lanes' needs the map's move table"):
        call(sm, (ped, cyc, car))                           # (this model has no lanelets: the second map's clearance refuses)
    assert sm.ctx.calls == ["fo_scene_hidden_clearance"]
    # 3. then v before a_brake, after every clearance ran
    sm = BC._cpu_model(torch)
    sm.lane_moves = object()
    with pytest.raises(ValueError, match=r"^hidden_brake_users: v must be \[M, T\]$"):
        call(sm, (ped, cyc, car))
    assert sm.ctx.calls == ["fo_scene_hidden_clearance", "fo_scene_hidden_clearance_flow"]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^hidden_brake_users: a_brake >= 0 and finite$"):
            SensorModel.hidden_brake_users(sm, z, z, z, z, users=(ped,), a_brake=bad, **kw)
    assert "fo_scene_hidden_brake_users" not in sm.ctx.calls
    # 4. a good call: one clearance per distinct (metric, flow) in order of first appearance, each at the fastest of its users, then the
    # one entry; ONE heading pass; 8 x 112 is accepted
    sm = BC._cpu_model(torch)
    sm.lane_moves = object()
    x = np.cumsum(np.full((2, 112), 0.05), axis=1)
    z = np.zeros((2, 112))
    users = ((4.0, "road", "lanes"), (0.5, "euclid", "any"), (2.0, "road", "any"), (0.0, "road", "lanes"), (1.0, "euclid", "any"),
             (3.0, "road", "any"), (6.0, "road", "lanes"), (0.25, "road", "any"))
    del passes[:]
    out = SensorModel.hidden_brake_users(sm, x, z, z, np.full((2, 112), 0.5), users=users, a_brake=0.0, lengths=np.array([112, 7]), **kw)
    assert sm.ctx.calls == ["fo_scene_hidden_clearance_flow", "fo_scene_hidden_clearance", "fo_scene_hidden_clearance", "fo_scene_hidden_brake_users"]
    assert passes == [1]
    assert isinstance(out, hidden_traffic.HiddenBrakeUsers) and out.users == users and (out.a_brake, out.dt) == (0.0, 0.1)
    assert out.map_of == (0, 1, 2, 0, 1, 2, 0, 2) and isinstance(out.clearances, tuple) and len(out.clearances) == 3
    assert [(c.metric, c.flow) for c in out.clearances] == [("road", "lanes"), ("euclid", "any"), ("road", "any")]
    margin = out.clearances[0].margin
    assert [c.r2_cap for c in out.clearances] == [int(hidden_traffic.hidden_reach_r2(v, 0.1, margin, SC.CS, 112)[-1]) for v in (6.0, 1.0, 3.0)]
    assert all(c.heading is out.clearances[0].heading for c in out.clearances)
    assert out.thr.dtype == np.int32 and np.array_equal(out.thr, hidden_traffic.hidden_brake_thresholds([u[0] for u in users], 0.1, margin, SC.CS, 112))
    assert all(int(out.thr[c, -1]) <= 169 * out.clearances[k].r2_cap for c, k in enumerate(out.map_of))
    assert tuple(out.brake_first.shape) == (8, 2, 112) and tuple(out.stop.shape) == (2, 112)
    assert tuple(out.commit.shape) == tuple(out.first.shape) == (8, 2)
    assert out.brake_first.dtype == out.stop.dtype == out.commit.dtype == out.first.dtype == torch.int32
    assert np.array_equal(out.arc.numpy(), hidden_traffic.travelled_arc(x, z)) and out.lengths.tolist() == [112, 7]
    assert sm._hbu_inputs[1] is out.arc and all(a is b for a, b in zip(sm._hbu_inputs[2], out.clearances)) and sm._hc_inputs[2] is out.clearances[0].heading
    # heading= handed over: no heading pass at all, theta may be None
    del passes[:]
    sm.ctx.calls.clear()
    x, z = x[:, :31], z[:, :31]
    out2 = SensorModel.hidden_brake_users(sm, x, z, None, z, users=(ped, cyc, car), a_brake=2.0, heading=out.clearances[0].heading[:, :31], **kw)
    assert passes == [] and sm.ctx.calls == ["fo_scene_hidden_clearance", "fo_scene_hidden_clearance_flow", "fo_scene_hidden_brake_users"]
    assert out2.map_of == (0, 1, 1) and out2.clearances[1].r2_cap == int(hidden_traffic.hidden_reach_r2(13.9, 0.1, margin, SC.CS, 31)[-1])


def test_interface_defaults():
    pytest.importorskip("torch")
    import inspect
    from frenetix_occlusion.interface import FOInterface
    from frenetix_occlusion.sensor_model import SensorModel
    assert list(inspect.signature(FOInterface.hidden_brake_users).parameters) == ["self", "trajectories", "users", "a_brake", "margin", "inflate"]
    sig = inspect.signature(SensorModel.hidden_brake_users)
    assert list(sig.parameters) == ["self", "x", "y", "theta", "v", "vehicle", "users", "dt", "a_brake", "margin", "inflate", "lengths", "heading"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    seen = {}

    def hidden_brake_users(x, y, theta, v, **kw):
        seen.update(kw, x=x, v=v)
        return "result"
    vp = SimpleNamespace(length=4.508, width=1.61, wb_rear_axle=1.4227, mass=1093.3, a_max=11.5)
    fo = SimpleNamespace(timestep=3, sensor_model=SimpleNamespace(window=object(), hidden_brake_users=hidden_brake_users),
                         occlusion_memory={"v_max": 13.9, "margin": 0.7}, vehicle_params=vp, dt=0.1)
    traj = {k: np.full((2, 5), i, dtype=np.float64) for i, k in enumerate(("x", "y", "theta", "v", "a"))}
    users = ((2.0, "road", "any"), (7.0, "road", "lanes"))
    assert FOInterface.hidden_brake_users(fo, traj, users) == "result"
    assert seen["a_brake"] == 11.5 and seen["users"] is users and seen["margin"] == 0.7 and seen["dt"] == 0.1
    assert seen["vehicle"] == (4.508, 1.61, 1.4227) and seen["inflate"] == 0.0 and "metric" not in seen and "flow" not in seen
    assert seen["v"] is traj["v"] and seen["x"] is traj["x"]
    FOInterface.hidden_brake_users(fo, traj, users[:1], a_brake=4.0, margin=0.0, inflate=0.2)
    assert (seen["a_brake"], seen["users"], seen["margin"], seen["inflate"]) == (4.0, users[:1], 0.0, 0.2)
    fo.timestep = None
    with pytest.raises(RuntimeError, match="^hidden_brake_users needs a previous evaluate_scenario$"):
        FOInterface.hidden_brake_users(fo, traj, users)


# ------------------------------------------------------------------------------------------------ 4. the C side, by a host compiler
def _cc(names):
    return next((c for c in names if shutil.which(c)), None)


def test_native_mirror_has_the_layout_of_the_header(tmp_path):
    """size and the offset of every member of fo_hidden_brake_users_t against what a C compiler makes of include/fo_hip.h; the
    constants; the entry is declared and exported"""
    from frenetix_occlusion import _native as N
    cc = _cc(("gcc", "cc", "clang"))
    if cc is None:
        pytest.skip("no host C compiler")
    fields = [n for n, *_ in N.HiddenBrakeUsers._fields_]
    assert fields == ["M", "T", "d_x", "d_y", "d_heading", "d_len_or_null", "hl", "hw", "wb", "win_ix0", "win_iy0", "win_nx", "win_ny",
                      "K", "C", "d_key", "d_qmin", "r2_cap", "map_of", "d_v", "d_arc", "a_brake", "dt", "h_thr", "d_brake_first", "d_stop",
                      "d_commit", "d_first"]
    arrays = ("d_key", "d_qmin", "r2_cap", "map_of")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fo_hip.h"', 'int main(void) {', 'fo_hidden_brake_users_t p;',
             'printf("%zu %d %d %d\\n", sizeof(fo_hidden_brake_users_t), FO_HIDDEN_BRAKE_MAX_MAPS, FO_HIDDEN_BRAKE_MAX_CLASSES, '
             'FO_HIDDEN_BRAKE_MAX_TABLE);']
    lines += ['printf("%%zu\\n", offsetof(fo_hidden_brake_users_t, %s));' % f for f in fields]
    lines += ['printf("%%zu\\n", sizeof(p.%s));' % f for f in arrays]
    lines += ['return 0; }']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:4] == [C.sizeof(N.HiddenBrakeUsers), N.HIDDEN_BRAKE_MAX_MAPS, N.HIDDEN_BRAKE_MAX_CLASSES, N.HIDDEN_BRAKE_MAX_TABLE] and out[1:4] == [3, 8, 896]
    assert out[4:4 + len(fields)] == [getattr(N.HiddenBrakeUsers, f).offset for f in fields]
    assert out[4 + len(fields):] == [getattr(N.HiddenBrakeUsers, f).size for f in arrays] == [24, 24, 12, 32]
    assert "fo_scene_hidden_brake_users" in N.EXPORTS
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        assert "int fo_scene_hidden_brake_users(fo_ctx *ctx, const fo_hidden_brake_users_t *p, void *stream);" in f.read()


_PLAN_DRIVER = r"""
#include <cstdio>
#include "fo_hip.h"
#include "fo_scene_plan.hpp"
static_assert(BRAKE_USERS_MAX_MAPS == FO_HIDDEN_BRAKE_MAX_MAPS && BRAKE_USERS_MAX_TABLE == FO_HIDDEN_BRAKE_MAX_TABLE, "the plan's limits are the header's");
int main() {
  long long M, T, K, C;
  printf("%zu\n", brake_users_lds_bound());
  while (scanf("%lld %lld %lld %lld", &M, &T, &K, &C) == 4)
    printf("%d %d %zu %zu\n", brake_users_width((int)C), brake_users_blocks((int)M, (int)T), brake_users_lds_bytes((int)T, (int)K, (int)C),
           brake_classes_lds_bytes((int)T, (int)C));
  return 0;
}
"""


def test_launch_plan(tmp_path):
    """the host functions of csrc/fo_scene_plan.hpp behind the launch, built alone with the host compiler: the grid of the brake kernel,
    its six rows plus one int32 row per map and trajectory plus the table in LDS, the compile-time class count 4 or 8; with one map the
    bytes are the classes kernel's; the bound of 64 544 bytes -- T = 254, three maps, a table of 896 entries -- holds for every call and
    lies under 64 KB"""
    cxx = _cc(("g++", "c++", "clang++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "driver.cpp").write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "driver")
    csrc = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"), "-o", exe])
    asked = [(M, T, K, C_) for T in (1, 2, 3, 31, 32, 33, 64, 65, 112, 128, 253, 254) for K in (1, 2, 3) for C_ in range(1, 9) if C_ * T <= 896
             for M in (1, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257, 10000, 2 ** 31 - 1)]
    assert (1, 112, 3, 8) in asked and (1, 254, 3, 3) in asked and (1, 254, 3, 4) not in asked
    out = subprocess.run([exe], input="\n".join("%d %d %d %d" % a for a in asked) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    bound = int(out[0])
    assert bound == 4 * 254 * (48 + 4 * 3) + 4 * 896 == 64544 and bound < 64 * 1024
    worst = 0
    for (M, T, K, C_), line in zip(asked, out[1:]):
        G = 1
        while G < min(T, 64):
            G *= 2
        per = 256 // G
        lds = per * T * (48 + 4 * K) + 4 * C_ * T
        got = [int(v) for v in line.split()]
        assert got[:3] == [4 if C_ <= 4 else 8, -(-M // per), lds], (M, T, K, C_)
        assert lds <= bound and (K != 1 or got[3] == lds)
        worst = max(worst, lds)
    assert worst == 4 * 254 * 60 + 4 * 3 * 254 == 64008          # the largest a call can ask for: C * T <= 896 leaves 3 classes at T = 254
