"""Hidden-traffic brake ladder by road users on the CPU (DESIGN.md §5.10 "Brake ladder by road users"): the checker
tests/ref_hidden_brake_ladder_users.py is held to hand cases whose results are written down -- among them the one the entry exists
for, a level clear of every user that lies above every user's own answer --, to tests/ref_hidden_brake_users.py level by level and to
tests/ref_hidden_brake_ladder.py class by class (the two ties), and to conditions on the scenes the device test reuses; the host layer
runs on CPU tensors with a stand-in for the native call; the ctypes mirror and the launch plan are held to the header and to csrc by a
host compiler.  Every comparison is between integers and exact."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_ladder_users_scenes as S
import hidden_brake_scenes as SC
import ref_hidden_brake_ladder as L
import ref_hidden_brake_ladder_users as LU
import ref_hidden_brake_users as BU
import ref_hidden_clearance as HC
import test_hidden_brake_cpu as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = HC.NONE


# ------------------------------------------------------------------------------------------------ 1. hand cases
# The road of tests/test_hidden_brake_cpu.py: 5 x 60 cells of 1 m, dt = 0.5 s; the ego (1.8 m x 0.8 m about its reference point,
# heading east in row 2) touches column k iff k - 0.4 <= x <= k + 1.4.  The key of a cell is here the SAMPLE at which hidden traffic
# reaches it (NONE = never) and every class has the thresholds thr[j] = j: "key <= thr[j]" reads "reached by sample j".
def _key(reached):
    """a key map: ``reached`` = {(first column, end column): sample}"""
    key = np.full((5, 60), NONE, dtype=np.int64)
    for (lo, hi), j in reached.items():
        key[:, lo:hi] = j
    return key


def _hand(x0, v, levels, keys, map_of, starts=None, lens=None):
    v = np.asarray(v, dtype=np.float64)[None]
    T = v.shape[1]
    x = x0 + np.concatenate(([0.0], np.cumsum(v[0, :-1] * BC.H_DT)))[None]
    y = np.full((1, T), 2.5)
    head = np.zeros((1, T, 2))
    head[..., 0] = 1.0
    lens = None if lens is None else np.array([lens], dtype=np.int32)
    qmins = [HC.clearance(k, BC.H_WIN, BC.H_ROAD, BC.H_ORIGIN, BC.H_CS, x, y, head, BC.H_HL, BC.H_HW, BC.H_WB, lens) for k in keys]
    thr = np.tile(np.arange(T, dtype=np.int64), (len(map_of), 1))
    return LU.ladder_users(keys, BC.H_WIN, BC.H_ROAD, qmins, BC.H_ORIGIN, BC.H_CS, x, y, head, SC.travelled_arc(x, y), v, BC.H_HL, BC.H_HW,
                           BC.H_WB, levels, T if starts is None else starts, BC.H_DT, thr, map_of, lens)


CROSSING = _key({(20, 22): 4})        # test_a_harder_brake_can_be_less_safe's map: columns 20 and 21 are reached at sample 4, nothing else
STRETCH = _key({(30, 60): 0})         # hidden from column 30 on, at once: the ego touches it iff x >= 29.6


def test_the_level_clear_of_every_user_lies_above_every_users_own():
    """What the entry exists for.  8 m/s from x = 10.5, brake start 0, the ladder 0, 3, 8 m/s^2.
    User 0 on CROSSING is tests/test_hidden_brake_ladder_cpu.py's test_a_harder_brake_can_be_less_safe: without braking the ego has
    passed the columns before sample 4, at 3 m/s^2 it is at 22.0 at sample 4 and moves until sample 6, at 8 it stands at 16.5 --
    unclear = no, YES, no; its own required is 0.
    User 1 on STRETCH: without braking the ego is at 30.5 at sample 5 and never stands; at 3 m/s^2 it comes to rest at 23.25, at 8 at
    16.5 -- unclear = YES, no, no; its own required is 1.
    Together: level 0 is unclear for user 1, level 1 for user 0, level 2 is the first one clear of both: required_all = 2, above
    max(0, 1).  The level below it, 1, is blocked by user 0 alone."""
    r = _hand(10.5, [8.0] * 10, [0.0, 3.0, 8.0], [CROSSING, STRETCH], (0, 1))
    assert r.first[:, 0].tolist() == [-1, 5]
    assert r.brake_first[0, 0, 0].tolist() == [-1, 4, -1] and r.brake_first[1, 0, 0].tolist() == [5, -1, -1]
    assert r.stop[0, 0].tolist() == [10, 6, 2]
    assert r.required[:, 0, 0].tolist() == [0, 1] and r.last_unclear[:, 0, 0].tolist() == [1, 0]
    assert r.required_all[0, 0] == 2 > r.required[:, 0, 0].max() and r.last_unclear_all[0, 0] == 1
    assert r.blocking[0, 0] == 0b01
    assert (0, 0) in LU.above_every_user(r, None, 10)
    # not degenerate: each user alone gives its own answer and no more, and a maximum over the users would have said 1
    for c, key in enumerate((CROSSING, STRETCH)):
        alone = _hand(10.5, [8.0] * 10, [0.0, 3.0, 8.0], [key], (0,))
        assert alone.required_all[0, 0] == alone.required[0, 0, 0] == r.required[c, 0, 0] and alone.blocking[0, 0] == (0, 1)[c]
    # the same users the other way round, on maps handed over the other way round: the rows turn with them
    t = _hand(10.5, [8.0] * 10, [0.0, 3.0, 8.0], [CROSSING, STRETCH], (1, 0))
    assert t.required[:, 0, 0].tolist() == [1, 0] and t.required_all[0, 0] == 2 and t.blocking[0, 0] == 0b10
    # later brake starts: from b = 1 (x = 14.5) the ego passes the crossing at any level (18.5, then 21.75 at sample 3 at 3 m/s^2, 25.0 at
    # sample 4), user 0 is clear throughout; from b = 5 on the candidate itself is in the stretch
    assert r.required[0, 0].tolist()[:5] == [0, 0, 0, 0, 0] and r.required[1, 0, 5:].tolist() == [-1] * 5
    # user 1's commit: at 3 m/s^2 from b = 1 (14.5) the ego rests at 27.25, from b = 2 (18.5) it is at 30.0 at sample 6, still moving; at
    # 8 m/s^2 from b = 3 (22.5) it rests at 28.5, from b = 4 (26.5) it is at 30.5 at sample 5, moving
    assert r.commit[0, 0].tolist() == [-1, 0, -1] and r.commit[1, 0].tolist() == [0, 2, 4]


def test_blocking_on_a_hand_table():
    T_, F = True, False
    #           level 0  1   2   3
    unclear = [[T_, T_, F, F],          # class 0
               [F, T_, T_, F],          # class 1
               [T_, F, F, F]]           # class 2
    assert LU.blocking_mask(unclear, 3) == 0b010            # level 2: class 1 alone
    assert LU.blocking_mask(unclear, 2) == 0b011            # (were 2 the answer:) level 1: classes 0 and 1
    assert LU.blocking_mask(unclear, 1) == 0b101            # level 0: classes 0 and 2
    assert LU.blocking_mask(unclear, 0) == 0                # nothing below level 0
    assert LU.blocking_mask(unclear, -1) == 0               # no clear level: the last level, where nobody is unclear here
    assert LU.blocking_mask([[T_, T_], [F, T_], [F, F]], -1) == 0b011
    # through the walk: towards STRETCH at 8 m/s from x = 0.5 (tests/test_hidden_brake_ladder_cpu.py's straight run: required = 0, 0, 0,
    # 0, 1, 2, 3, -1, -1, -1 on the ladder 2, 3.5, 4, 8) with a second user on a map on which nothing is ever reached
    r = _hand(0.5, [8.0] * 10, [2.0, 3.5, 4.0, 8.0], [STRETCH, _key({})], (0, 1, 0))
    assert r.required[0, 0].tolist() == r.required[2, 0].tolist() == r.required_all[0].tolist() == [0, 0, 0, 0, 1, 2, 3, -1, -1, -1]
    assert r.required[1, 0].tolist() == [0] * 10 and r.last_unclear[1, 0].tolist() == [-1] * 10 and r.first[:, 0].tolist() == [8, -1, 8]
    assert r.blocking[0].tolist() == [0, 0, 0, 0, 0b101, 0b101, 0b101, 0b101, 0b101, 0b101]
    assert r.last_unclear_all[0].tolist() == [-1, -1, -1, -1, 0, 1, 2, 3, 3, 3] and r.commit[0, 0].tolist() == [4, 5, 6, 7]
    assert (r.commit[1] == -1).all() and LU.above_every_user(r, None, 10) == []
    # fewer brake starts: the rows are cut, commit keeps what lies below B
    r = _hand(0.5, [8.0] * 10, [2.0, 3.5, 4.0, 8.0], [STRETCH, _key({})], (0, 1, 0), starts=6)
    assert r.required_all[0].tolist() == [0, 0, 0, 0, 1, 2] and r.commit[2, 0].tolist() == [4, 5, -1, -1] and r.stop.shape == (1, 6, 4)


def test_ragged_lengths_mark_no_manoeuvre():
    r = _hand(10.5, [8.0] * 6, [1.0, 4.0], [STRETCH, CROSSING], (0, 1), lens=2)
    assert r.required_all[0].tolist() == [0, 0, -1, -1, -1, -1] and r.last_unclear_all[0].tolist() == [-1] * 6
    assert r.required[:, 0].tolist() == [[0, 0, -1, -1, -1, -1]] * 2 and (r.last_unclear == -1).all() and (r.blocking == 0).all()
    assert r.stop[0].tolist() == [[2, 2], [2, 2]] + [[-1, -1]] * 4 and (r.brake_first == -1).all() and (r.commit == -1).all()
    r = _hand(10.5, [8.0] * 6, [1.0, 4.0], [STRETCH], (0,), lens=0)
    assert (r.required_all == -1).all() and (r.last_unclear_all == -1).all() and (r.blocking == 0).all() and (r.first == -1).all()
    assert LU.kinds(r, np.array([0]), 6)["no_manoeuvre"] == 6


def test_the_candidates_own_first_blocks_every_level():
    """2 m/s from x = 28.5 (tests/test_hidden_brake_ladder_cpu.py's case): user 0's candidate is in STRETCH from sample 2 on and no
    deceleration helps from there; user 1 (nothing ever reached) stays clear -- required_all = -1 and the last level is blocked by
    user 0 alone"""
    r = _hand(28.5, [2.0] * 6, [0.5, 8.0, 1e9], [STRETCH, _key({})], (0, 1))
    assert r.first[:, 0].tolist() == [2, -1]
    assert r.required[0, 0].tolist() == [1, 1, -1, -1, -1, -1] and r.last_unclear[0, 0].tolist() == [0, 0, 2, 2, 2, 2]
    assert r.required_all[0].tolist() == r.required[0, 0].tolist() and r.required[1, 0].tolist() == [0] * 6
    assert r.blocking[0].tolist() == [1] * 6 and r.commit[0, 0].tolist() == [0, 2, 2]


# ------------------------------------------------------------------------------------------------ 2. the two ties
def _cut(commit, starts):
    return np.where(commit < starts, commit, -1)


@pytest.mark.parametrize("spec", S.SCENES, ids=lambda s: "-".join(str(v) for v in s))
def test_every_level_is_the_users_checker(spec):
    """slice l of brake_first and stop, and first, are ref_hidden_brake_users.brake_users at a_brake = levels[l] for b < B, row for
    row; commit[..., l] is its commit where that is < B, else -1"""
    sc, res = S.checked(spec)
    C_, n_levels, nb = len(sc.map_of), len(sc.levels), sc.starts
    assert res.brake_first.shape == (C_, sc.M, nb, n_levels) and res.stop.shape == (sc.M, nb, n_levels) and res.commit.shape == (C_, sc.M, n_levels)
    assert res.required.shape == res.last_unclear.shape == (C_, sc.M, nb) and res.first.shape == (C_, sc.M)
    assert res.required_all.shape == res.last_unclear_all.shape == res.blocking.shape == (sc.M, nb) and all(a.dtype == np.int32 for a in res)
    for n in sorted({0, n_levels // 2, n_levels - 1}):
        bf, st, commit, first = BU.brake_users(sc.keys, sc.win, sc.road, sc.qmins, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW,
                                               SC.WB, float(sc.levels[n]), sc.dt, sc.thr, sc.map_of, sc.lens)
        assert np.array_equal(res.brake_first[..., n], bf[:, :, :nb]) and np.array_equal(res.stop[..., n], st[:, :nb]), n
        assert np.array_equal(res.commit[..., n], _cut(commit, nb)) and np.array_equal(res.first, first), n


@pytest.mark.parametrize("spec", S.SCENES, ids=lambda s: "-".join(str(v) for v in s))
def test_every_class_is_the_ladders_checker(spec):
    """row c of required, last_unclear and commit (and of brake_first; stop whole) is ref_hidden_brake_ladder.ladder on that class's
    arrival map -- the first sample at which the key of its map lies within its threshold row -- with that class's first"""
    sc, res = S.checked(spec)
    for c, k in enumerate(sc.map_of):
        A = S.arrival_of(sc.keys[k], sc.thr[c])
        bf, st, req, lu, cm = L.ladder(A, sc.win, sc.road, res.first[c], SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB,
                                       sc.levels, sc.starts, sc.dt, sc.lens)
        assert np.array_equal(res.required[c], req) and np.array_equal(res.last_unclear[c], lu) and np.array_equal(res.commit[c], cm), c
        assert np.array_equal(res.brake_first[c], bf) and np.array_equal(res.stop, st), c


def test_scenes_are_not_degenerate():
    """by the checker alone, over the scenes the device runs: an interior required_all, one of -1 with a manoeuvre, one of 0, a
    non-monotone pair, a pair whose required_all lies above every user's own, pairs without a manoeuvre; users that differ; every
    value the plan's shapes are to take"""
    tot, differ, masks = {}, 0, set()
    for spec in S.SCENES + ["hand"]:
        sc, res = S.checked(spec)
        for k, n in LU.kinds(res, sc.lens, sc.T).items():
            tot[k] = tot.get(k, 0) + int(n)
        differ += int((res.required != res.required[:1]).any())
        masks |= set(np.unique(res.blocking).tolist())
        L_ = len(sc.levels)
        assert ((res.required_all >= -1) & (res.required_all < L_) & (res.last_unclear_all >= -1) & (res.last_unclear_all < L_)).all()
        own = np.where(res.required < 0, L_, res.required).max(axis=0)                   # no level clear of all lies below a user's own
        assert (np.where(res.required_all < 0, L_, res.required_all) >= own).all()
        assert (res.last_unclear_all == res.last_unclear.max(axis=0)).all()
    print(tot, sorted(masks))
    assert tot["interior"] >= 20 and tot["none"] >= 20 and tot["zero"] >= 20 and tot["non_monotone"] >= 1 and tot["above"] >= 1
    assert tot["no_manoeuvre"] >= 20 and differ >= 3 and len(masks) >= 4
    assert {len(S.scene(*s[:3], s[3], 1, "1", 1, 1).x) for s in S.SCENES} >= {1, 3, 70}
    assert {s[6] for s in S.SCENES} >= {1, 2, 23, 33, 64} and {s[4] for s in S.SCENES} >= {1, 4, 5, 8}
    assert {s[5] for s in S.SCENES} == {"1", "2", "3", "same", "gap"} and {s[2] for s in S.SCENES} == {2, 31, 33, 100, 254}
    assert all({1, T} <= {s[7] for s in S.SCENES if s[2] == T} for T in (2, 31, 33)) and any(s[3] for s in S.SCENES)
    groups = {S.expected_plan(s[2], S.LAYOUTS[s[5]][0], s[4], s[6], s[7])[1] for s in S.SCENES}
    assert groups >= {2, 16, 32, 64, 128, 256}                  # parts of a wave, a wave, two and four waves
    same = S.scene(*next(s for s in S.SCENES if s[5] == "same"))
    assert same.keys[0] is same.keys[1]


def test_the_hand_scene_of_the_device_test():
    """tests/hidden_brake_ladder_users_scenes.hand_scene, the hand case above on the road of the device tests: what its docstring
    derives for candidate 0 from b = 0, and that the case is there for all three candidates"""
    sc, res = S.checked("hand")
    assert res.first.tolist() == [[-1, -1, -1], [24, 23, 26]]
    assert res.required[:, 0, 0].tolist() == [0, 1] and res.last_unclear[:, 0, 0].tolist() == [1, 0]
    assert res.brake_first[0, 0, 0].tolist() == [-1, 20, -1] and res.brake_first[1, 0, 0].tolist() == [24, -1, -1] and res.stop[0, 0].tolist() == [31, 27, 10]
    assert res.required_all[0, 0] == 2 and res.last_unclear_all[0, 0] == 1 and res.blocking[0, 0] == 0b01
    above = LU.above_every_user(res, None, sc.T)
    assert {m for m, _ in above} == {0, 1, 2} and all((m, 0) in above for m in range(3)) and len(above) == 33


# ------------------------------------------------------------------------------------------------ 3. the host layer
def _result(torch, required, last_unclear, required_all, last_unclear_all, blocking, decelerations, detail=False):
    from frenetix_occlusion.hidden_traffic import HiddenBrakeLadderUsers
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.int32))
    C_, M, nb = np.shape(required)
    users = tuple((float(c + 1), "road", "any") for c in range(C_))
    L_ = len(decelerations)
    bf = t(np.arange(C_ * M * nb * L_).reshape(C_, M, nb, L_)) if detail else None
    st = t(np.arange(M * nb * L_).reshape(M, nb, L_)) if detail else None
    return HiddenBrakeLadderUsers((), users, (0,) * C_, np.zeros((C_, 4), dtype=np.int32), np.array(decelerations), t(required), t(last_unclear),
                                  t(np.arange(C_ * M * L_).reshape(C_, M, L_)), t(np.zeros((C_, M))), t(required_all), t(last_unclear_all),
                                  t(blocking), bf, st, None, 0.1)


def test_derived_tables_on_a_hand_table():
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import HiddenBrakeLadderUsers
    from frenetix_occlusion.sensor_model import HiddenBrakeLadderUsers as exported
    assert exported is HiddenBrakeLadderUsers
    #              clear at once | interior, monotone | interior, NOT monotone | no level clear | no manoeuvre
    required = [[[0, 1, 0, -1, -1]], [[0, 2, 1, 0, -1]]]
    last_unclear = [[[-1, 0, 1, 2, -1]], [[-1, 1, 0, 1, -1]]]
    required_all, last_unclear_all, blocking = [[0, 2, 2, -1, -1]], [[-1, 1, 1, 2, -1]], [[0, 0b10, 0b01, 0b01, 0]]
    out = _result(torch, required, last_unclear, required_all, last_unclear_all, blocking, [0.5, 4.0, 11.5], detail=True)
    rd = out.required_deceleration()
    assert rd.dtype == torch.float64 and tuple(rd.shape) == (1, 5)
    assert rd[0, :3].tolist() == [0.5, 11.5, 11.5] and rd[0, 3].item() == float("inf") and np.isnan(rd[0, 4].item())
    r0, r1 = out.required_deceleration(0), out.required_deceleration(user=1)
    assert r0[0, :3].tolist() == [0.5, 4.0, 0.5] and r0[0, 3].item() == float("inf") and np.isnan(r0[0, 4].item())
    assert r1[0, :4].tolist() == [0.5, 11.5, 4.0, 0.5] and np.isnan(r1[0, 4].item())
    btn = out.brake_threat_number(11.5)
    assert btn[0, :3].tolist() == [0.5 / 11.5, 1.0, 1.0] and btn[0, 3].item() == float("inf") and np.isnan(btn[0, 4].item())
    assert out.brake_threat_number(8.0, user=0)[0, :3].tolist() == [0.5 / 8.0, 0.5, 0.5 / 8.0]
    assert out.monotone().dtype == torch.bool and out.monotone()[0].tolist() == [True, True, True, True, True]
    assert out.monotone(0)[0].tolist() == [True, True, False, True, True] and out.monotone(user=1)[0].tolist() == [True, True, True, False, True]
    bu = out.blocking_users()
    assert bu.dtype == torch.bool and tuple(bu.shape) == (2, 1, 5)
    assert bu[0, 0].tolist() == [False, False, True, True, False] and bu[1, 0].tolist() == [False, True, False, False, False]
    bf, st, cm = out.level(1)
    assert tuple(bf.shape) == (2, 1, 5) and tuple(st.shape) == (1, 5) and tuple(cm.shape) == (2, 1)
    assert bf[1, 0, 2].item() == (5 + 2) * 3 + 1 and st[0, 4].item() == 4 * 3 + 1 and cm[:, 0].tolist() == [1, 4]
    plain = _result(torch, required, last_unclear, required_all, last_unclear_all, blocking, [0.5, 4.0, 11.5])
    assert plain.brake_first is None and plain.stop is None
    with pytest.raises(ValueError, match=r"^HiddenBrakeLadderUsers\.level: brake_first and stop were not asked for \(detail=True\)$"):
        plain.level(0)


def test_refusals_and_calls_in_their_order(monkeypatch):
    torch = pytest.importorskip("torch")
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import hidden_traffic
    from frenetix_occlusion.sensor_model import SensorModel
    assert SensorModel.__dict__["hidden_brake_ladder_users"] is hidden_traffic.hidden_brake_ladder_users     # the module function itself
    assert N.HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES == 3584
    monkeypatch.setattr(N, "current_stream", lambda index=None: None)
    passes = []
    plain = hidden_traffic.unit_headings
    monkeypatch.setattr(hidden_traffic, "unit_headings", lambda theta: passes.append(1) or plain(theta))
    z = np.zeros((2, 31))
    kw = dict(vehicle=SC.VEH, dt=0.1)
    bad_v = np.zeros((2, 30))
    ped, cyc, car = (2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes")
    # 1. the users' refusals in hidden_brake_users' words under the new prefix, before the model is looked at and with everything else
    # wrong too
    none = SimpleNamespace(window=None, cell_size=SC.CS)
    call = lambda sm, users, x=z, v=bad_v, decelerations=(), starts=0, **more: SensorModel.hidden_brake_ladder_users(
        sm, x, x, x, v, users=users, decelerations=decelerations, starts=starts, **kw, **more)
    p = r"^hidden_brake_ladder_users: "
    for users, text in ((((2.0, "road"),), r"users\[0\] = \(2\.0, 'road'\) is no triple"), ((ped, ("fast", "road", "any")), r"users\[1\] = \('fast', 'road', 'any'\) is no triple"),
                        ((ped, 7.0), r"users\[1\] = 7\.0 is no triple")):
        with pytest.raises(ValueError, match=p + text + r" \(speed, metric, flow\) with a number for the speed$"):
            call(none, users)
    for users in ((), (ped,) * 9, None, 5):
        with pytest.raises(ValueError, match=p + r"users must hold 1 \.\. 8 triples \(speed, metric, flow\)$"):
            call(none, users)
    with pytest.raises(ValueError, match=p + r"users\[1\]: metric 'manhattan', one of \('euclid', 'road'\) is possible$"):
        call(none, (ped, (float("nan"), "manhattan", "lanes")))
    with pytest.raises(ValueError, match=p + r"users\[0\]: flow 'left', one of \('any', 'lanes'\) is possible$"):
        call(none, ((-1.0, "road", "left"),))
    with pytest.raises(ValueError, match=p + r"users\[2\]: flow 'lanes' follows the lanes along the road: it needs metric 'road'"):
        call(none, (ped, cyc, (7.0, "euclid", "lanes")))
    for s in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=p + r"the users' speeds must be finite and >= 0$"):
            call(none, (ped, (s, "road", "any")))
    with pytest.raises(ValueError, match=p + r"8 users x 113 samples = 904 thresholds, at most 896 are possible"):
        call(none, (ped,) * 8, x=np.zeros((2, 113)))
    # 2. then the ladder's, in hidden_brake_ladder's words
    many = np.linspace(0.0, 13.0, 65)
    for bad in ([], None, 4.0, [1.0, -0.5], [float("nan")], [1.0, float("inf")], many, ["a"], "123", np.ones((1, 3))):
        with pytest.raises(ValueError, match=p + r"decelerations must hold 1 \.\. 64 finite values >= 0$"):
            call(none, (ped,), decelerations=bad)
    for bad in ([2.0, 1.0], [1.0, 1.0]):
        with pytest.raises(ValueError, match=p + r"decelerations must be strictly ascending"):
            call(none, (ped,), decelerations=bad)
    # 3. then the budget, in words that name both counts: 8 x 112 thresholds fill the argument alone, 8 x 100 leave room for 48 levels
    with pytest.raises(ValueError, match=p + r"8 users x 112 samples = 896 thresholds of 4 bytes and 1 decelerations of 8 bytes are 3592 bytes, "
                                             r"at most 3584 are possible"):
        call(none, (ped,) * 8, x=np.zeros((2, 112)), decelerations=[1.0])
    with pytest.raises(ValueError, match=p + r"8 users x 100 samples = 800 thresholds of 4 bytes and 49 decelerations of 8 bytes are 3592 bytes"):
        call(none, (ped,) * 8, x=np.zeros((2, 100)), decelerations=many[:49])
    # 4. then each clearance's, in its words
    with pytest.raises(RuntimeError, match=r"^hidden_clearance needs the cell classes of a previous launch\(\)$"):
        call(none, (ped, cyc), decelerations=[1.0])
    sm = BC._cpu_model(torch)
    with pytest.raises(ValueError, match=r"^hidden_clearance: lengths must be \[M\]$"):
        call(sm, (ped, cyc), decelerations=[1.0], lengths=np.zeros(3))
    assert sm.ctx.calls == []
    with pytest.raises(RuntimeError, match=r"^hidden_clearance: flow 'lanes' needs the map's move table"):
        call(sm, (ped, cyc, car), decelerations=[1.0])        # (this model has no lanelets: the second map's clearance refuses)
    assert sm.ctx.calls == ["fo_scene_hidden_clearance"]
    # 5. then v, then starts
    sm = BC._cpu_model(torch)
    sm.lane_moves = object()
    with pytest.raises(ValueError, match=p + r"v must be \[M, T\]$"):
        call(sm, (ped, cyc, car), decelerations=[1.0])
    assert sm.ctx.calls == ["fo_scene_hidden_clearance", "fo_scene_hidden_clearance_flow"]
    for bad in (0, 32, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match=p + r"starts = .*, an integer in \[1, T = 31\] or None$"):
            call(sm, (ped,), v=z, decelerations=[1.0, 2.0], starts=bad)
    assert "fo_scene_hidden_brake_ladder_users" not in sm.ctx.calls
    # 6. a good call: one clearance per distinct (metric, flow) in order of first appearance, then the ONE entry; one heading pass;
    # 8 x 100 thresholds and 48 levels are accepted; no detail unless asked for
    sm = BC._cpu_model(torch)
    sm.lane_moves = object()
    x = np.cumsum(np.full((2, 100), 0.05), axis=1)
    z = np.zeros((2, 100))
    users = ((4.0, "road", "lanes"), (0.5, "euclid", "any"), (2.0, "road", "any"), (0.0, "road", "lanes"), (1.0, "euclid", "any"),
             (3.0, "road", "any"), (6.0, "road", "lanes"), (0.25, "road", "any"))
    del passes[:]
    out = SensorModel.hidden_brake_ladder_users(sm, x, z, z, np.full((2, 100), 0.5), users=users, decelerations=many[:48], starts=np.int64(7),
                                                lengths=np.array([100, 7]), **kw)
    assert sm.ctx.calls == ["fo_scene_hidden_clearance_flow", "fo_scene_hidden_clearance", "fo_scene_hidden_clearance",
                            "fo_scene_hidden_brake_ladder_users"]
    assert passes == [1]
    assert isinstance(out, hidden_traffic.HiddenBrakeLadderUsers) and out.users == users and out.dt == 0.1
    assert out.map_of == (0, 1, 2, 0, 1, 2, 0, 2) and [(c.metric, c.flow) for c in out.clearances] == [("road", "lanes"), ("euclid", "any"), ("road", "any")]
    margin = out.clearances[0].margin
    assert np.array_equal(out.thr, hidden_traffic.hidden_brake_thresholds([u[0] for u in users], 0.1, margin, SC.CS, 100))
    assert out.decelerations.dtype == np.float64 and np.array_equal(out.decelerations, many[:48])
    assert tuple(out.required.shape) == tuple(out.last_unclear.shape) == (8, 2, 7) and tuple(out.commit.shape) == (8, 2, 48)
    assert tuple(out.first.shape) == (8, 2) and tuple(out.required_all.shape) == tuple(out.last_unclear_all.shape) == tuple(out.blocking.shape) == (2, 7)
    assert all(getattr(out, k).dtype == torch.int32 for k in LU.SUMMARY) and out.brake_first is None and out.stop is None
    assert np.array_equal(out.arc.numpy(), hidden_traffic.travelled_arc(x, z)) and out.lengths.tolist() == [100, 7]
    assert sm._hblu_inputs[1] is out.arc and all(a is b for a, b in zip(sm._hblu_inputs[2], out.clearances))
    # detail, starts = None (T), heading= handed over: no heading pass at all, theta may be None
    del passes[:]
    sm.ctx.calls.clear()
    x, z = x[:, :31], z[:, :31]
    out2 = SensorModel.hidden_brake_ladder_users(sm, x, z, None, z, users=(ped, cyc, car), decelerations=(3.0,), detail=True,
                                                 heading=out.clearances[0].heading[:, :31], **kw)
    assert passes == [] and sm.ctx.calls == ["fo_scene_hidden_clearance", "fo_scene_hidden_clearance_flow", "fo_scene_hidden_brake_ladder_users"]
    assert out2.map_of == (0, 1, 1) and tuple(out2.brake_first.shape) == (3, 2, 31, 1) and tuple(out2.stop.shape) == (2, 31, 1)
    assert out2.brake_first.dtype == out2.stop.dtype == torch.int32 and tuple(out2.required_all.shape) == (2, 31)


def test_interface_defaults_and_signatures():
    pytest.importorskip("torch")
    from frenetix_occlusion.interface import FOInterface
    from frenetix_occlusion.sensor_model import SensorModel
    assert list(inspect.signature(FOInterface.hidden_brake_ladder_users).parameters) == ["self", "trajectories", "users", "decelerations", "starts",
                                                                                         "detail", "margin", "inflate"]
    sig = inspect.signature(SensorModel.hidden_brake_ladder_users)
    assert list(sig.parameters) == ["self", "x", "y", "theta", "v", "vehicle", "users", "dt", "decelerations", "starts", "detail", "margin",
                                    "inflate", "lengths", "heading"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    assert (sig.parameters["starts"].default, sig.parameters["detail"].default, sig.parameters["inflate"].default) == (None, False, 0.0)
    seen = {}

    def hidden_brake_ladder_users(x, y, theta, v, **kw):
        seen.clear()
        seen.update(kw, x=x, v=v)
        return "result"
    vp = SimpleNamespace(length=4.508, width=1.61, wb_rear_axle=1.4227, mass=1093.3, a_max=11.5)
    fo = SimpleNamespace(timestep=3, sensor_model=SimpleNamespace(window=object(), hidden_brake_ladder_users=hidden_brake_ladder_users),
                         occlusion_memory={"v_max": 13.9, "margin": 0.7}, vehicle_params=vp, dt=0.1)
    traj = {k: np.full((2, 5), i, dtype=np.float64) for i, k in enumerate(("x", "y", "theta", "v", "a"))}
    users = ((2.0, "road", "any"), (7.0, "road", "lanes"))
    assert FOInterface.hidden_brake_ladder_users(fo, traj, users) == "result"
    assert seen["decelerations"] == [0.5 * k for k in range(1, 24)] and seen["starts"] is None and seen["detail"] is False
    assert seen["users"] is users and seen["margin"] == 0.7 and seen["dt"] == 0.1 and seen["vehicle"] == (4.508, 1.61, 1.4227)
    assert seen["inflate"] == 0.0 and "metric" not in seen and "flow" not in seen and "v_max" not in seen and "a_brake" not in seen
    assert seen["v"] is traj["v"] and seen["x"] is traj["x"]
    FOInterface.hidden_brake_ladder_users(fo, traj, users[:1], decelerations=[1.0, 2.0], starts=3, detail=True, margin=0.0, inflate=0.2)
    assert (seen["users"], seen["decelerations"], seen["starts"], seen["detail"], seen["margin"], seen["inflate"]) == (users[:1], [1.0, 2.0], 3, True, 0.0, 0.2)
    vp.a_max = 8.2                                              # hidden_brake_ladder's default: a_max itself is appended
    FOInterface.hidden_brake_ladder_users(fo, traj, users)
    assert seen["decelerations"] == [0.5 * k for k in range(1, 17)] + [8.2]
    vp.a_max = 32.5
    with pytest.raises(ValueError, match=r"^hidden_brake_ladder_users: the default ladder .* has more than 64 levels"):
        FOInterface.hidden_brake_ladder_users(fo, traj, users)
    fo.timestep = None
    with pytest.raises(RuntimeError, match="^hidden_brake_ladder_users needs a previous evaluate_scenario$"):
        FOInterface.hidden_brake_ladder_users(fo, traj, users)
    assert "config" not in inspect.getsource(FOInterface.hidden_brake_ladder_users)      # no configuration key


# ------------------------------------------------------------------------------------------------ 4. the C side, by a host compiler
def _cc(names):
    return next((c for c in names if shutil.which(c)), None)


def test_native_mirror_has_the_layout_of_the_header(tmp_path):
    """size and the offset of every member of fo_hidden_brake_ladder_users_t against what a C compiler makes of include/fo_hip.h; the
    constants; the entry is declared and exported"""
    from frenetix_occlusion import _native as N
    cc = _cc(("gcc", "cc", "clang"))
    if cc is None:
        pytest.skip("no host C compiler")
    fields = [n for n, *_ in N.HiddenBrakeLadderUsers._fields_]
    assert fields == ["M", "T", "d_x", "d_y", "d_heading", "d_len_or_null", "hl", "hw", "wb", "win_ix0", "win_iy0", "win_nx", "win_ny",
                      "K", "C", "d_key", "d_qmin", "r2_cap", "map_of", "d_v", "d_arc", "h_levels", "L", "B", "dt", "h_thr", "d_required",
                      "d_last_unclear", "d_commit", "d_first", "d_required_all", "d_last_unclear_all", "d_blocking", "d_brake_first_or_null",
                      "d_stop_or_null"]
    arrays = ("d_key", "d_qmin", "r2_cap", "map_of")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fo_hip.h"', 'int main(void) {', 'fo_hidden_brake_ladder_users_t p;',
             'printf("%zu %d %d %d %d %d\\n", sizeof(fo_hidden_brake_ladder_users_t), FO_HIDDEN_BRAKE_MAX_MAPS, FO_HIDDEN_BRAKE_MAX_CLASSES, '
             'FO_HIDDEN_BRAKE_MAX_TABLE, FO_HIDDEN_BRAKE_MAX_LEVELS, FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES);']
    lines += ['printf("%%zu\\n", offsetof(fo_hidden_brake_ladder_users_t, %s));' % f for f in fields]
    lines += ['printf("%%zu\\n", sizeof(p.%s));' % f for f in arrays]
    lines += ['return 0; }']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:6] == [C.sizeof(N.HiddenBrakeLadderUsers), N.HIDDEN_BRAKE_MAX_MAPS, N.HIDDEN_BRAKE_MAX_CLASSES, N.HIDDEN_BRAKE_MAX_TABLE,
                       N.HIDDEN_BRAKE_MAX_LEVELS, N.HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES] and out[1:6] == [3, 8, 896, 64, 3584]
    assert out[6:6 + len(fields)] == [getattr(N.HiddenBrakeLadderUsers, f).offset for f in fields]
    assert out[6 + len(fields):] == [getattr(N.HiddenBrakeLadderUsers, f).size for f in arrays] == [24, 24, 12, 32]
    assert "fo_scene_hidden_brake_ladder_users" in N.EXPORTS
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        header = f.read()
    assert "int fo_scene_hidden_brake_ladder_users(fo_ctx *ctx, const fo_hidden_brake_ladder_users_t *p, void *stream);" in header
    assert "#define FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES 3584" in header


_PLAN_DRIVER = r"""
#include <cstdio>
#include "fo_hip.h"
#include "fo_scene_plan.hpp"
static_assert(BRAKE_LADDER_USERS_MAX_ARG_BYTES == FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES && BRAKE_LADDER_USERS_MAX_CLASSES == FO_HIDDEN_BRAKE_MAX_CLASSES &&
              BRAKE_USERS_MAX_MAPS == FO_HIDDEN_BRAKE_MAX_MAPS, "the plan's limits are the header's");
int main() {
  long long M, T, K, C, L, B;
  printf("%zu %d %d\n", brake_ladder_users_lds_bound(), HB_THREADS, BRAKE_LADDER_ROWS_BYTES);
  // every (T, K, C, L, B) a call can have: the largest LDS size, and whether the plan ever breaks one of its own rules
  size_t worst = 0;
  long long broken = 0, n = 0;
  for (int t = 1; t <= 254; ++t)
    for (int k = 1; k <= FO_HIDDEN_BRAKE_MAX_MAPS; ++k)
      for (int l = 1; l <= FO_HIDDEN_BRAKE_MAX_LEVELS; ++l)
        for (int b = 1; b <= t; ++b) {
          const int Lp = brake_ladder_users_width(l), G = brake_ladder_users_group(t, k, l, b), per = brake_ladder_users_per_block(t, k, l, b);
          const size_t rows = (size_t)per * t * (48 + 4 * k);
          broken += !(Lp >= l && Lp <= 64 && (Lp & (Lp - 1)) == 0 && G >= Lp && G <= HB_THREADS && (G & (G - 1)) == 0 && per * G == HB_THREADS &&
                      (G >= b * Lp || G == HB_THREADS) && (per == 1 || rows <= (size_t)BRAKE_LADDER_ROWS_BYTES));
          for (int c = 1; c <= FO_HIDDEN_BRAKE_MAX_CLASSES; ++c) {
            if (c * t > FO_HIDDEN_BRAKE_MAX_TABLE || 4 * c * t + 8 * l > FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES) continue;
            const size_t lds = brake_ladder_users_lds_bytes(t, k, c, l, b);
            broken += lds != rows + (size_t)4 * c * t + (size_t)4 * c * HB_THREADS;
            worst = lds > worst ? lds : worst;
            ++n;
          }
        }
  printf("%zu %lld %lld\n", worst, broken, n);
  while (scanf("%lld %lld %lld %lld %lld %lld", &M, &T, &K, &C, &L, &B) == 6)
    printf("%d %d %d %d %zu\n", brake_ladder_users_width((int)L), brake_ladder_users_group((int)T, (int)K, (int)L, (int)B),
           brake_ladder_users_per_block((int)T, (int)K, (int)L, (int)B), brake_ladder_users_blocks((int)M, (int)T, (int)K, (int)L, (int)B),
           brake_ladder_users_lds_bytes((int)T, (int)K, (int)C, (int)L, (int)B));
  return 0;
}
"""


def test_launch_plan(tmp_path):
    """the host functions of csrc/fo_scene_plan.hpp behind the launch (built alone with the host compiler) against their Python
    restatement tests/hidden_brake_ladder_users_scenes.expected_plan at the switch points: L around every power of two, B Lp around
    every power of two up to 256, T around the horizons at which the 32 KB of rows halve the trajectories of a workgroup (at K = 3,
    60 T per <= 32 768: T = 2 | 3, 4 | 5, 8 | 9, 17 | 18, 34 | 35, 68 | 69, 136 | 137).  The LDS size of EVERY admissible
    (T, K, C, L, B) is derived, not sampled: the driver walks them all, reports the largest size and any broken rule; the largest
    stays under brake_ladder_users_lds_bound() = 44 544 bytes, and that under the 64 KB of a workgroup"""
    cxx = _cc(("g++", "c++", "clang++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "driver.cpp").write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "driver")
    csrc = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"), "-o", exe])
    Ts = (1, 2, 3, 4, 5, 8, 9, 17, 18, 31, 33, 34, 35, 68, 69, 112, 136, 137, 254)
    Ls = (1, 2, 3, 4, 5, 8, 9, 16, 17, 23, 32, 33, 63, 64)
    ok = lambda T, C_, L_: C_ * T <= 896 and 4 * C_ * T + 8 * L_ <= 3584
    asked = []
    for T in Ts:
        for K in (1, 2, 3):
            for L_ in Ls:
                Lp = S.expected_plan(T, K, 1, L_, 1)[0]
                Bs = {1, T, (T + 1) // 2} | {b for g in (64, 128, 256) for b in (g // Lp - 1, g // Lp, g // Lp + 1)}
                for Bn in sorted(b for b in Bs if 1 <= b <= T):
                    per = S.expected_plan(T, K, 1, L_, Bn)[2]
                    for C_ in (c for c in (1, 3, 4, 5, 8) if ok(T, c, L_)):
                        asked += [(M, T, K, C_, L_, Bn) for M in sorted({0, 1, per - 1, per, per + 1, 10000, 2 ** 31 - 1} - {-1})]
    assert any(q[1:] == (31, 2, 3, 23, 31) for q in asked) and any(q[1] == 254 and q[3] == 1 for q in asked)
    out = subprocess.run([exe], input="\n".join("%d %d %d %d %d %d" % q for q in asked) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    bound, threads, rows = (int(v) for v in out[0].split())
    assert (bound, threads, rows) == (32768 + 3584 + 8 * 256 * 4, 256, 32768) and bound == 44544 < 64 * 1024
    worst, broken, n = (int(v) for v in out[1].split())
    assert broken == 0 and n > 10 ** 6 and worst <= bound
    # the same maximum by the restatement, over the classes the plan distinguishes: T, K, Lp and min(B Lp, 256) rounded up to a power of
    # two -- with the largest C the limits leave at the smallest L of that width
    derived = 0
    for T in range(1, 255):
        for Lp in (1, 2, 4, 8, 16, 32, 64):
            L_ = Lp // 2 + 1
            C_ = max(c for c in range(1, 9) if ok(T, c, L_))
            for K in (1, 2, 3):
                derived = max(derived, max(S.expected_plan(T, K, C_, L_, Bn)[3] for Bn in sorted({min(2 ** e, T) for e in range(9)})))
    assert worst == derived
    groups = set()
    for (M, T, K, C_, L_, Bn), line in zip(asked, out[2:]):
        Lp, G, per, lds = S.expected_plan(T, K, C_, L_, Bn)
        assert [int(v) for v in line.split()] == [Lp, G, per, -(-M // per), lds], (M, T, K, C_, L_, Bn)
        groups.add(G)
    assert groups == {1, 2, 4, 8, 16, 32, 64, 128, 256}
    # the default call: 31 samples, 23 levels, every start, two maps, three users -- a trajectory per workgroup, 5.2 KB
    assert S.expected_plan(31, 2, 3, 23, 31) == (32, 256, 1, 31 * 56 + 4 * 3 * 31 + 4 * 3 * 256)
