"""Hidden-traffic harm ladder by approach angle on the device (fo_scene_hidden_brake_harm_ladder_lanes,
SensorModel.hidden_brake_harm_ladder_lanes, FOInterface.hidden_brake_harm_ladder_lanes, PlanningStep(hidden_harm_ladder_lanes_verdict=);
DESIGN.md §5.10 "Harm ladder by approach angle"): the tie to fo_scene_hidden_brake_harm_ladder of the same library on the same device
inputs wherever nothing is known, bit for bit, on the smallest shapes at which the lane layout switches; the plain statement
tests/ref_hidden_brake_harm_ladder_lanes.py on the walk fo_scene_hidden_brake_ladder_users writes on the same device inputs, on hand-built
move tables; fo_scene_hidden_brake_impact_lanes per level; a hand case with the numbers written out; the edges of the hit; the fold on the
cost rows a real planning step left; the step with and without the stage; pre-filled outputs; the refusals.  Integers and decel are
compared exactly, harms to 1e-9 -- the scenes hold no open comparison (tests/test_hidden_harm_ladder_lanes_cpu.py).  Every test runs
under a time limit of its own that ends the process; no test provokes a fault."""
import ctypes as C
import faulthandler
import math
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_ladder_scenes as LS
import hidden_brake_scenes as SC
import hidden_harm_ladder_lanes_cases as HLC
import hidden_impact_cases as IC
import hidden_impact_lanes_cases as LC
import ref_hidden_brake_harm_ladder as RH
import ref_hidden_impact_lanes as RL
import ref_hidden_reach_flow as RF
import rule_refusal_cases as RC
import test_hidden_brake_ladder_users_gpu as LUG
import test_hidden_brake_ladder_verdict_gpu as LVG
import test_hidden_brake_users_gpu as UG
import test_hidden_brake_verdict_gpu as VG
import test_hidden_harm_ladder_gpu as HG
import test_hidden_impact_lanes_gpu as ILG
import test_hidden_reach_flow_gpu as FG
import test_hidden_reach_gpu as T
from test_hidden_brake_ladder_verdict_cpu import expected_plan
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
STEP_LIMIT = 240
TOL = 1e-9
PATTERN = HG.PATTERN
NORTH, WEST, EAST = RF.sector(90), RF.sector(180), RF.sector(0)
LANE_USERS, STEP_KINDS, LEVELS5 = ILG.LANE_USERS, ILG.STEP_KINDS, HG.LEVELS5


@pytest.fixture(autouse=True)
def _time_limit(request):
    faulthandler.dump_traceback_later(getattr(request.module, request.function.__name__ + "_limit", STEP_LIMIT), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw(torch, sm, sc, levels, B, harm_limit, mask, slack=0.0, rows=None, speed_of=None, a_limit=np.inf, keys=None, qmins=None, thr=None,
         map_of=None, r2_caps=None, finite=None, cost=None, safe=None, drop=(), drop_map=(), **over):
    """fo_scene_hidden_brake_harm_ladder_lanes on scene ``sc`` (or on edited data of it) against the move table the context holds; the
    arguments of tests/test_hidden_harm_ladder_gpu._raw, and ``mask`` (dir_mask) and ``slack`` (cos_h and sin_h are the host's of 22.5 deg
    + slack); every byte of the output buffers is pre-filled with PATTERN.  Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    dev = sm.device
    sent = {}

    def up(a, dt):
        if a is None:
            return None
        if id(a) not in sent:
            sent[id(a)] = torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
        return sent[id(a)]
    pick = lambda given, own: getattr(sc, own) if given is None else given
    keys, qmins, thr, map_of, r2_caps = pick(keys, "keys"), pick(qmins, "qmins"), pick(thr, "thr"), pick(map_of, "map_of"), pick(r2_caps, "r2_caps")
    M, Tn = sc.x.shape
    thr = np.ascontiguousarray(thr, dtype=np.int32)
    levels = np.ascontiguousarray(levels, dtype=np.float64)
    Cn, Kn, Ln = thr.shape[0], len(keys), len(levels)
    if rows is None:
        rows, speed_of = IC.rows_of(IC.KINDS8[:Cn]), [float(u[0]) for u in sc.users[:Cn]]
    tx, ty, th, tv, ta = (up(a, np.float64) for a in (sc.x, sc.y, sc.head, sc.v, sc.arc))
    dk, dq, tl = [up(k, np.int32) for k in keys], [up(q, np.int32) for q in qmins], up(sc.lens, np.int32)
    tf, tc, ts = up(finite, np.uint8), up(cost, np.float64), up(safe, np.uint8)
    trow = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float64).reshape(Cn, 4)).to(dev)
    tsp = torch.as_tensor(np.ascontiguousarray(speed_of, dtype=np.float64)).to(dev)

    def filled(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(PATTERN)
        return t
    i32, f64 = torch.int32, torch.float64
    out = SimpleNamespace(need=filled((M,), i32), at=filled((M,), i32), blocking=filled((M,), i32), user=filled((M,), i32),
                          need_of=filled((Cn, M), i32), first=filled((Cn, M), i32), decel=filled((M,), f64),
                          harm_at=filled((M, Ln), f64), user_at=filled((M, Ln), i32))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    pad = lambda vals, n, fill: (list(vals) + [fill] * n)[:n]
    ptrs = dict(d_key=pad([p(t) for t in dk], 3, None), d_qmin=pad([p(t) for t in dq], 3, None))
    for name, k in drop_map:
        ptrs[name][k] = None
    win = sc.win
    cos_h, sin_h = RL.host_h(slack)
    kw = dict(M=over.pop("count", M), T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=HL, hw=HW, wb=WB, win_ix0=win[0],
              win_iy0=win[1], win_nx=win[2], win_ny=win[3], K=Kn, C=Cn, d_key=(C.c_void_p * 3)(*ptrs["d_key"]), d_qmin=(C.c_void_p * 3)(*ptrs["d_qmin"]),
              r2_cap=(C.c_int32 * 3)(*pad([int(r) for r in r2_caps], 3, -5)), map_of=(C.c_int32 * 8)(*pad([int(k) for k in map_of], 8, 99)),
              d_v=p(tv), d_arc=p(ta), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), L=Ln, B=int(B), dt=float(sc.dt),
              h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), a_limit=float(a_limit), d_finite_or_null=p(tf), d_cost_or_null=p(tc),
              d_safe_or_null=p(ts), d_need=p(out.need), d_at=p(out.at), d_blocking=p(out.blocking), d_user=p(out.user), d_decel=p(out.decel),
              d_need_of=p(out.need_of), d_first=p(out.first), d_speed_of=p(tsp), d_harm_rows=p(trow), harm_limit=float(harm_limit),
              d_harm_at=p(out.harm_at), d_user_at=p(out.user_at), dir_mask=int(mask), cos_h=cos_h, sin_h=sin_h)
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeHarmLadderLanes(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_harm_ladder_lanes(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    res = SimpleNamespace(**{k: _np(getattr(out, k)) for k in RH.OUTPUTS})
    res.cost, res.safe = (None if tc is None else _np(tc)), (None if ts is None else _np(ts))
    return rc, msg, res


def _moves(sm, moves):
    from frenetix_occlusion import _native as N
    assert FG._set_moves(sm, moves) == N.FO_OK


def _bitwise(got, want, what, names=RH.OUTPUTS):
    for name in names:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:4].tolist())


# ------------------------------------------------------------------------------------------------ 1. the tie (a)
def _tie(torch, sm, sc, levels, B, limit, what, **edited):
    """the three ways of knowing nothing -- no lane-bound class, a table of 0xFF alone, heading_slack = pi -- against the head-on entry on
    the same device inputs: all nine outputs and the folded rows bit for bit"""
    M = sc.x.shape[0]
    rng = np.random.default_rng(M * 131 + B)
    cost0, safe0 = rng.random((M, 16)), (np.arange(M) % 3 != 0).astype(np.uint8)
    a_limit = float(levels[len(levels) // 2])
    rc, msg, ref = HG._raw(torch, sm, sc, levels, B, limit, a_limit=a_limit, cost=cost0, safe=safe0, **edited)
    assert rc == 0, (what, msg)
    every = (1 << len(edited.get("thr", sc.thr))) - 1
    for name, table, mask, slack in (("dir_mask = 0", "cross", 0, 0.0), ("a table of 0xFF", "any", every, 0.0), ("slack = pi", "cross", every, math.pi)):
        _moves(sm, LC.table(table))
        rc, msg, out = _raw(torch, sm, sc, levels, B, limit, mask, slack, a_limit=a_limit, cost=cost0, safe=safe0, **edited)
        assert rc == 0, (what, name, msg)
        HG._assert_written(out, (what, name))
        _bitwise(out, ref, (what, name))
        assert out.cost.tobytes() == ref.cost.tobytes() and np.array_equal(out.safe, ref.safe), (what, name)
    return ref


TIE_LADDERS = (1, 2, 23, 33, 64)


@pytest.mark.parametrize("T_", sorted(HG.TIE_SCENES))
def test_tie_to_the_head_on_entry_at_every_form_of_the_plan(torch_cuda, T_):
    """T in {1, 2, 31, 65} x L in {1, 2, 23, 33, 64} x B in {1, 2, 5, T} with M at per_block - 1 and per_block + 1 on the scene's FIRST rows
    (lengths 0, 1, 2 lead them) and at per_block on its LAST rows: consequence (a) bit for bit on all nine outputs and the folded rows,
    the three ways -- G = 64, 128 and 256, one round and two, five users on three maps"""
    torch = torch_cuda
    sm, road = UG._parked()
    sc = LVG._scene(HG.TIE_SCENES[T_])
    assert np.array_equal(road, sc.road) and len(sc.keys) == 3
    groups, rounds, hit = set(), set(), 0
    for L in TIE_LADDERS:
        levels = LS.levels_of(L)
        for B in sorted({b for b in (1, 2, 5, T_) if b <= T_}):
            Lp, G, per, _, _ = expected_plan(T_, 3, 5, L, B, sc.M)
            groups.add(G)
            rounds.add(-(-B * Lp // G))
            for lo, hi in sorted({(0, max(per - 1, 1)), (0, per + 1), (sc.M - per, sc.M)}):
                assert 0 <= lo < hi <= sc.M
                ref = _tie(torch, sm, HG._cut(sc, lo, hi), levels, B, 0.1, (T_, L, B, lo, hi))
                hit += int((ref.harm_at > 0).sum())
    assert T_ < 31 or ({64, 128, 256} <= groups and {1, 2} <= rounds and hit > 0), (groups, rounds, hit)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C_", [1, 4, 5, 8])
def test_tie_over_class_and_map_counts(torch_cuda, C_, K):
    """C in {1, 4, 5, 8} x K in {1, 2, 3}: all six instantiations, class c on map (c + 1) % K -- and, with K >= 2, maps that are the very
    same BUFFER; at limit 0 the shared outputs are the ladder verdict's as well"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc = LVG._scene((232, 20, 31, True, 8, "3", 1, 1))
    edited = dict(keys=sc.keys[:K], qmins=sc.qmins[:K], map_of=[(c + 1) % K for c in range(C_)], r2_caps=sc.r2_caps[:K], thr=sc.thr[:C_])
    for L, B, limit in ((23, 5, 0.1), (2, 31, 0.3), (1, 1, 0.0)):
        _tie(torch, sm, sc, LS.levels_of(L), B, limit, (C_, K, L, B), **edited)
    ref = _tie(torch, sm, sc, LS.levels_of(5), 5, 0.0, (C_, K, "limit 0"), **edited)
    rc, msg, lv = LVG._raw(torch, sm, sc, LS.levels_of(5), 5, **edited)
    assert rc == 0, msg
    _bitwise(ref, lv, (C_, K, "the ladder verdict"), RH.SHARED)
    if K >= 2:
        same = dict(edited, keys=[sc.keys[0]] * K, qmins=[sc.qmins[0]] * K)
        _tie(torch, sm, sc, LS.levels_of(5), 5, 0.1, (C_, K, "one buffer"), **same)


# ------------------------------------------------------------------------------------------------ 2. the checker
def _walk(torch, sm, sc, levels=None, B=None):
    rc, msg, lu = LUG._raw(torch, sm, sc, detail=True, levels=np.asarray(sc.levels if levels is None else levels, dtype=np.float64),
                           B=sc.starts if B is None else B)
    assert rc == 0, msg
    return lu


def _checked(torch, sm, sc, limit, what, lu=None, finite=None):
    """the entry on a scene of tests/hidden_harm_ladder_lanes_cases.py against the checker on the device's own walk: integers exactly, decel
    bit for bit, harm_at to 1e-9; returns (outputs, checker's, worst harm difference)"""
    _moves(sm, sc.moves)
    lu = _walk(torch, sm, sc) if lu is None else lu
    want = HLC.check(sc, lu, limit, finite=finite)
    hits = np.array(want["hits"])
    assert want["closest"] >= RH.OPEN_TOL and (not hits.size or np.abs(hits - limit).min() >= RH.OPEN_TOL), what
    rc, msg, out = _raw(torch, sm, sc, sc.levels, sc.starts, limit, sc.mask, sc.slack, rows=sc.rows, speed_of=sc.speed_of, finite=finite)
    assert rc == 0, (what, msg)
    HG._assert_written(out, what)
    return out, want, HG._assert_checker(out, want, what)


@pytest.mark.parametrize("case", range(len(HLC.RAW_CASES)))
def test_checker_on_the_raw_scenes_with_hand_built_move_tables(torch_cuda, case):
    """tests/hidden_impact_lanes_cases.RAW_CASES as scenes of the ladder family -- masks none, all and mixed (a lane-bound and a free class
    on one map), the lane table and the striped one, slacks 0, 0.2 and pi / 2, three levels -- at the two limits between the scene's own
    harms: integers exactly, decel bit for bit, harm_at to 1e-9; and never above the head-on entry on the same inputs (b)"""
    torch = torch_cuda
    sm, road = UG._parked()
    sc = HLC.raw_case(case)
    assert np.array_equal(road, sc.road)
    _moves(sm, sc.moves)
    lu = _walk(torch, sm, sc)
    lims = HLC.limits(HLC.check(sc, lu, 0.0)["hits"])
    assert lims is not None
    worst = 0.0
    for limit in lims:
        out, want, diff = _checked(torch, sm, sc, limit, (HLC.RAW_CASES[case], limit), lu=lu)
        worst = max(worst, diff)
        rc, msg, head = HG._raw(torch, sm, sc, sc.levels, sc.starts, limit, rows=sc.rows, speed_of=sc.speed_of)
        assert rc == 0, msg
        assert (out.harm_at <= head.harm_at).all() and (out.need <= head.need).all() and (out.need_of <= head.need_of).all()
        assert np.array_equal(out.first, head.first)
        if sc.mask == 0:
            _bitwise(out, head, HLC.RAW_CASES[case])
    print(f"{HLC.RAW_CASES[case]}: worst |harm_at - checker| = {worst:.3e} over {len(want['hits'])} hits, limits {lims[0]:.6f} {lims[1]:.6f}; "
          f"{int((out.harm_at < head.harm_at).sum())} (m, l) below head-on, need lowered at {int((out.need < head.need).sum())} candidates")


def test_each_level_is_the_impact_verdict_by_approach_angle_at_that_deceleration(torch_cuda):
    """(c): harm_at[:, l] is the obstacle harm of fo_scene_hidden_brake_impact_lanes at a_brake = levels[l] and the same B on the same
    inputs, to 1e-9, and user_at its user exactly (no two classes tie: tests/test_hidden_harm_ladder_lanes_cpu.py)"""
    torch = torch_cuda
    sm, _ = UG._parked()
    worst, users, below = 0.0, set(), 0
    for case in (1, 3, 8, 9):
        sc = HLC.raw_case(case)
        _moves(sm, sc.moves)
        rc, msg, out = _raw(torch, sm, sc, sc.levels, sc.starts, 0.1, sc.mask, sc.slack, rows=sc.rows, speed_of=sc.speed_of)
        assert rc == 0, msg
        for l, level in enumerate(sc.levels):
            rc, msg, iv = ILG._raw_lanes(torch, sm, sc.win, sc.r2_caps, sc.keys, sc.qmins, sc.x, sc.y, sc.head, sc.v, sc.arc, float(level), sc.dt,
                                         sc.thr, sc.map_of, sc.starts, sc.rows, sc.speed_of, sc.mask, sc.slack, lens=sc.lens)
            assert rc == 0, msg
            diff = float(np.abs(out.harm_at[:, l] - iv.harm[:, 0]).max())
            assert diff <= TOL and np.array_equal(out.user_at[:, l], iv.user), (case, l, diff)
            worst, users, below = max(worst, diff), users | set(iv.user.tolist()), below + int((iv.cosine < 1.0).sum())
    print(f"worst |harm_at - impact verdict's obstacle harm| = {worst:.3e}; users {sorted(users)}; {below} priced below head-on")
    assert len(users) >= 3 and below > 0


def test_never_above_head_on_on_scenario_1(torch_cuda, tmp_path):
    """(b) on scenario 1 with its own lane_move_raster and the three README users through FOInterface: harm_at, need and decel are never
    above the head-on call's, first is its first; with heading_slack = pi every output is that call's; the defaults are the sibling's"""
    torch = torch_cuda
    import test_hidden_witness_gpu as WG
    from frenetix_occlusion import synthetic as SY
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    ego, yaw = WG._drive(fo, sc, 3)
    traj = SY.make_trajectories(64, 31, WG.DT, seed=WG.SEED, ego_pos=ego, ego_yaw=yaw)
    users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
    assert fo.sensor_model.lane_moves is not None
    head = fo.hidden_brake_harm_ladder(traj, users, starts=5)
    lanes = fo.hidden_brake_harm_ladder_lanes(traj, users, starts=5)
    wide = fo.hidden_brake_harm_ladder_lanes(traj, users, starts=5, heading_slack=math.pi)
    torch.cuda.synchronize()
    assert lanes.approach == "lanes" and lanes.heading_slack == 0.0 and head.approach == "head_on" and wide.heading_slack == math.pi
    assert lanes.kinds == head.kinds and lanes.harm_limit == head.harm_limit and lanes.levels.tolist() == head.levels.tolist() and lanes.a_limit == head.a_limit
    assert (_np(lanes.harm_at) <= _np(head.harm_at)).all() and (_np(lanes.need) <= _np(head.need)).all() and (_np(lanes.decel) <= _np(head.decel)).all()
    assert (_np(lanes.need_of) <= _np(head.need_of)).all() and torch.equal(lanes.first, head.first)
    assert torch.equal(lanes.need_of[0], head.need_of[0])                  # the pedestrian is not lane-bound
    for name in RH.OUTPUTS:
        assert torch.equal(getattr(wide, name), getattr(head, name)), name
    print(f"scenario 1: {int((_np(lanes.harm_at) < _np(head.harm_at)).sum())} of {lanes.harm_at.numel()} (m, l) below head-on, need lowered at "
          f"{int((_np(lanes.need) < _np(head.need)).sum())} of 64 candidates")


# ------------------------------------------------------------------------------------------------ 3. the hand case
def test_hand_case_with_known_numbers(torch_cuda):
    """a car at 13.9 m/s against an east-bound ego that brakes from 8 m/s at 2 and at 4 m/s^2 (dt 0.5): the wall at 10 m is hit at sample 2
    with 6 m/s and 4 m/s left.  Head-on the harms are 0.034616760809621 and 0.031764897885419, from a north-bound cross lane (cosine = cos
    67.5 deg) 0.030713356125559 and 0.029099514513638.  With harm_limit = 0.030 the head-on entry says need = 2, "no level"; this stage
    says need = 1 from the cross lane, and 2 from the oncoming lane and from an off-lane cell"""
    torch = torch_cuda
    sm, road = UG._parked()
    for byte, need, harm_at in ((NORTH, 1, HLC.HAND_CROSS), (WEST, 2, HLC.HAND_HEAD_ON), (RF.ANY, 2, HLC.HAND_HEAD_ON)):
        h = HLC.hand_case(byte)
        assert np.array_equal(road, h.road)
        out, want, _ = _checked(torch, sm, h, HLC.HAND_LIMIT, ("hand", byte))
        assert (out.need.tolist(), out.at.tolist(), out.first.tolist(), out.user_at.tolist()) == ([need], [0], [[2]], [[0, 0]]), (byte, out.need)
        assert out.decel.tolist() == [4.0 if need == 1 else math.inf] and out.user.tolist() == [0] and out.blocking.tolist() == [1]
        assert np.abs(out.harm_at[0] - np.array(harm_at)).max() <= TOL, (byte, out.harm_at.tolist())
        rc, msg, head = HG._raw(torch, sm, h, h.levels, 1, HLC.HAND_LIMIT, rows=h.rows, speed_of=h.speed_of)
        assert rc == 0 and head.need.tolist() == [2] and np.abs(head.harm_at[0] - np.array(HLC.HAND_HEAD_ON)).max() <= TOL, msg
    assert abs(HLC.HAND_CROSS[1] - HLC.hand_harm(4.0, LC.COS_67_5)) <= 1e-14 and abs(HLC.HAND_HEAD_ON[0] - HLC.hand_harm(6.0, 1.0)) <= 1e-14


# ------------------------------------------------------------------------------------------------ 4. the edges
def test_the_met_case_against_a_manoeuvre_hit_of_the_same_class(torch_cuda):
    """the wall at 14 m: the candidate itself reaches it at sample 3 at 8 m/s -- the starts b >= 3 are MET there, at every level, at one
    harm --, the starts 1 and 2 hit it on their manoeuvres at less, start 0 at 4 m/s^2 stops short: the curve holds the met harm at
    cos 67.5 deg with B = 6, and the manoeuvres' with B = 3"""
    torch = torch_cuda
    sm, _ = UG._parked()
    w = LC.hand_case(8.0, 4.0, 14.0, NORTH)
    h = HLC.hand_case(NORTH)
    h.keys, h.qmins, h.moves = [w.key], [w.qmin], w.moves
    met = HLC.hand_harm(8.0, LC.COS_67_5)
    h.starts = 6
    out, want, _ = _checked(torch, sm, h, 0.02, "met, B = 6")
    assert out.first.tolist() == [[3]] and np.abs(out.harm_at[0] - met).max() <= TOL and (want["ho"][0, 0, 3:] == want["ho"][0, 0, 3, 0]).all()
    h.starts = 3
    out, want, _ = _checked(torch, sm, h, 0.02, "met, B = 3")
    assert (out.harm_at[0] < met).all() and (out.harm_at[0] > 0).all()
    h.mask = 0                                                             # the same car, free: the met harm is head-on
    h.starts = 6
    out, _, _ = _checked(torch, sm, h, 0.02, "met, free")
    assert np.abs(out.harm_at[0] - HLC.hand_harm(8.0, 1.0)).max() <= TOL


def test_two_classes_first_hit_at_one_pose_on_different_maps(torch_cuda):
    """class 0 on map 0, whose wall is the first column (a north-bound lane); class 1 on map 1, whose wall is the second column (the
    oncoming lane): both are first hit at the same pose, each priced by the cells of its own map"""
    torch = torch_cuda
    sm, _ = UG._parked()
    a = LC.hand_case(8.0, 4.0, 10.0, (NORTH, WEST, WEST, WEST), keys_at_wall=(0, LC.NONE, LC.NONE, LC.NONE), x0=0.25)
    b = LC.hand_case(8.0, 4.0, 10.0, (NORTH, WEST, WEST, WEST), keys_at_wall=(LC.NONE, 0, LC.NONE, LC.NONE), x0=0.25)
    for map_of, first, second in (([0, 1], a, b), ([1, 0], b, a)):
        h = HLC.hand_case(NORTH)
        h.x, h.arc, h.keys, h.qmins, h.moves, h.map_of, h.r2_caps = a.x, a.arc, [first.key, second.key], [first.qmin, second.qmin], a.moves, map_of, [1, 1]
        h.thr, h.rows, h.speed_of, h.mask = np.zeros((2, h.T), dtype=np.int32), np.array([LC.CAR_ROW, LC.CAR_ROW]), [LC.CAR_SPEED, 7.0], 0b11
        out, want, _ = _checked(torch, sm, h, 0.02, ("two maps", map_of))
        ho = want["ho"][:, 0, 0, 1]                                       # at 4 m/s^2: 4 m/s left
        assert abs(ho[0] - HLC.hand_harm(4.0, LC.COS_67_5)) <= 1e-12 and abs(ho[1] - RH.logistic(LC.CAR_ROW[0], LC.CAR_ROW[1], 4.0 + 7.0)) <= 1e-12
        assert abs(out.harm_at[0, 1] - max(ho)) <= TOL


def test_a_hit_at_the_last_moving_sample_counts_and_one_at_the_stop_does_not(torch_cuda):
    """braking from 8 m/s at 4 m/s^2 the ego stands from sample 4 on (poses 0 4 7 9 10 10 ...): a wall first covered at sample 3 = st - 1 is
    hit with 2 m/s left and priced by its lane; one first covered at sample 4 = st meets a standing ego: no hit at that level"""
    torch = torch_cuda
    sm, _ = UG._parked()
    for wall_x, hit in ((12.0, True), (13.0, False)):
        w = LC.hand_case(8.0, 4.0, wall_x, NORTH)
        h = HLC.hand_case(NORTH)
        h.keys, h.qmins, h.moves, h.levels = [w.key], [w.qmin], w.moves, np.array([4.0, 8.0])
        out, want, _ = _checked(torch, sm, h, 0.02, ("the stop", wall_x))
        if hit:
            assert abs(out.harm_at[0, 0] - HLC.hand_harm(2.0, LC.COS_67_5)) <= TOL and out.user_at[0, 0] == 0
        else:
            assert out.harm_at[0, 0] == 0.0 and out.user_at[0, 0] == -1 and out.need.tolist() == [0]


def test_a_hit_cell_off_the_raster_and_a_byte_without_a_central_direction(torch_cuda):
    """the rim of the whole-raster window beyond the raster's east end holds key 0: off the raster, 0xFF whatever the table says beside it
    -- head-on; the same key on the raster's last columns reads the table; a byte of two bits has no central direction and says nothing"""
    torch = torch_cuda
    sm, _ = UG._parked()
    end = SC.ORIGIN[0] + SC.RNX * SC.CS
    for wall_x, byte, cm in ((end, NORTH, 1.0), (end - 2.0, NORTH, LC.COS_67_5), (10.0, 0b00000110, 1.0), (10.0, NORTH | WEST, 1.0)):
        w = LC.hand_case(8.0, 4.0, wall_x, byte, beside=NORTH if wall_x > 10.0 else None, x0=wall_x - 10.0)
        h = HLC.hand_case(NORTH)
        h.x, h.arc, h.keys, h.qmins, h.moves = w.x, w.arc, [w.key], [w.qmin], w.moves
        out, _, _ = _checked(torch, sm, h, 0.02, ("off the raster", wall_x, byte))
        assert np.abs(out.harm_at[0] - np.array([HLC.hand_harm(6.0, cm), HLC.hand_harm(4.0, cm)])).max() <= TOL, (wall_x, byte, out.harm_at)


# ------------------------------------------------------------------------------------------------ 5. the fold and the step
def _hl(**over):
    kw = dict(vehicle=VG.VEH3, ego_mass=RC.VEH[3], users=LANE_USERS, kinds=STEP_KINDS, dt=0.1, levels=LEVELS5, starts=5, harm_limit=0.1, a_limit=4.0,
              heading_slack=0.1)
    kw.update(over)
    return kw


def _step_then_stage(torch, k, tr=None, **over):
    """a plain PlanningStep.run, its cost / safe copied, then the stage by its own call (on ``tr`` where given): (before, after, result)"""
    from frenetix_occlusion.step import PlanningStep
    tr = k.tr if tr is None else tr
    out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced").run(k.sc.ego, k.sc.yaw, k.sc.v)
    assert not hasattr(out, "hidden_harm_ladder_lanes_verdict")
    before = (out.cost.clone(), out.safe.clone())
    hl = k.sm.hidden_brake_harm_ladder_lanes(*tr[:4], cost=out.cost, safe=out.safe, **_hl(**over))
    torch.cuda.synchronize()
    return (_np(before[0]), _np(before[1])), (_np(out.cost), _np(out.safe)), hl


def _device_checker(torch, k, hl):
    """the stage through the Python layer against the checker on the very device data it walked on, held to the no-open-choice condition"""
    w = k.sm.window
    sc = SimpleNamespace(x=_np(k.tr[0]), y=_np(k.tr[1]), head=_np(hl.poses.heading), v=_np(k.tr[3]), arc=_np(hl.poses.arc), lens=None,
                         win=(w.ix0, w.iy0, w.nx, w.ny), dt=0.1, keys=[_np(c.key) for c in hl.clearances], qmins=[_np(c.qmin) for c in hl.clearances],
                         thr=hl.thr, map_of=hl.map_of, r2_caps=[c.r2_cap for c in hl.clearances], levels=hl.levels, starts=hl.starts, T=RC.T)
    lu = _walk(torch, k.sm, sc)
    import ref_hidden_brake_harm_ladder_lanes as RHL
    cos_h, sin_h = RL.host_h(hl.heading_slack)
    want = RHL.harm_ladder_lanes(sc.keys, sc.win, k.sm.road_raster(), k.sm.lane_moves, tuple(k.sm.raster_origin), k.sm.cell_size, sc.x, sc.y, sc.head,
                                 sc.arc, sc.v, HL, HW, WB, list(hl.levels), 0.1, hl.thr, hl.map_of, hl.starts, hl.rows.tolist(), hl.speed_of.tolist(),
                                 0b110, cos_h, sin_h, hl.harm_limit, lu.brake_first, lu.stop, lu.first, None, _np(hl.poses.finite))
    assert want["closest"] >= RH.OPEN_TOL and (not want["hits"] or np.abs(np.array(want["hits"]) - hl.harm_limit).min() >= RH.OPEN_TOL)
    return HG._assert_checker(SimpleNamespace(**{n: _np(getattr(hl, n)) for n in RH.OUTPUTS}), want, "the Python layer"), want


def test_fold_on_the_rows_of_a_real_step(torch_cuda):
    """clean rows: the fold is the checker's on what the stage wrote, at a_limit finite and inf; the stage itself is the checker on the
    device data it walked on; never above the head-on stage, and that stage with heading_slack = pi"""
    torch = torch_cuda
    k = VG._stack(torch)
    assert k.sm.lane_moves is not None
    before, after, hl = _step_then_stage(torch, k)
    assert before[1].any()
    HG._assert_fold(before, after, hl, 4.0)
    worst, want = _device_checker(torch, k, hl)
    assert hl.approach == "lanes" and hl.heading_slack == 0.1 and hl.starts == 5 and hl.harm_limit == 0.1 and hl.levels.tolist() == LEVELS5
    head = k.sm.hidden_brake_harm_ladder(*k.tr[:4], **{key: v for key, v in _hl().items() if key != "heading_slack"})
    torch.cuda.synchronize()
    assert (_np(hl.harm_at) <= _np(head.harm_at)).all() and (_np(hl.need) <= _np(head.need)).all() and torch.equal(hl.first, head.first)
    print(f"step rows: need {sorted(set(_np(hl.need).tolist()))}, worst |harm_at - checker| {worst:.3e}, {int((_np(hl.harm_at) < _np(head.harm_at)).sum())} "
          f"(m, l) below head-on, need lowered at {int((_np(hl.need) < _np(head.need)).sum())} candidates")
    before, after, hl2 = _step_then_stage(torch, k, a_limit=math.inf)
    HG._assert_fold(before, after, hl2, math.inf)
    assert np.array_equal(after[1], np.where(_np(hl2.need) == 5, 0, before[1]))
    _, _, wide = _step_then_stage(torch, k, heading_slack=math.pi)
    for name in RH.OUTPUTS:
        assert torch.equal(getattr(wide, name), getattr(head, name)), name


def test_a_refused_step_and_a_non_finite_candidate(torch_cuda):
    """a refused step (NaN costs) stays unsafe and gets the two columns; a NaN, an inf and a -inf pose fail closed -- need = L, user = -2,
    decel = inf, harm_at = 1.0 -- even at harm_limit = a_limit = inf"""
    torch = torch_cuda
    import test_rule_refusal_gpu as RG
    k = VG._stack(torch, RG.REFUSING_CELL)
    before, after, hl = _step_then_stage(torch, k)
    RG.assert_refused(SimpleNamespace(cost=torch.as_tensor(before[0]), safe=torch.as_tensor(before[1])))
    HG._assert_fold(before, after, hl, 4.0)
    assert not after[1].any() and after[0][:, RH.C_RES0].tobytes() == _np(hl.decel).tobytes()
    k = VG._stack(torch)
    tr = [t.clone() for t in k.tr]
    tr[0][3, 7], tr[2][11, 0], tr[3][40, 15] = float("nan"), float("inf"), float("-inf")
    before, after, hl = _step_then_stage(torch, k, tr=tr, harm_limit=math.inf, a_limit=math.inf)
    HG._assert_fold(before, after, hl, math.inf)
    need, user, decel, harm_at, user_at = (_np(getattr(hl, n)) for n in ("need", "user", "decel", "harm_at", "user_at"))
    for m in (3, 11, 40):
        assert (need[m], user[m], decel[m], after[1][m], after[0][m, RH.C_SAFE], after[0][m, RH.C_RES1]) == (5, -2, np.inf, 0, 0.0, -2.0), m
        assert harm_at[m].tolist() == [1.0] * 5 and user_at[m].tolist() == [-2] * 5
    rest = [m for m in range(RC.M) if m not in (3, 11, 40)]
    assert (user[rest] >= -1).all() and np.array_equal(after[1][rest], before[1][rest]) and (need[rest] <= 0).all()


def test_step_with_the_stage_is_the_call_and_a_step_without_it_is_unchanged(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion.step import PlanningStep
    k = VG._stack(torch)
    plain, staged, hl = _step_then_stage(torch, k)
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_lanes_verdict=_hl())
    for _ in range(2):                                              # (a second run folds into fresh rows, not into folded ones)
        out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
        torch.cuda.synchronize()
        assert _np(out.cost).tobytes() == staged[0].tobytes() and np.array_equal(_np(out.safe), staged[1])
        for name in RH.OUTPUTS:
            assert torch.equal(getattr(out.hidden_harm_ladder_lanes_verdict, name), getattr(hl, name)), name
        assert out.hidden_harm_ladder_lanes_verdict.approach == "lanes" and not hasattr(out, "hidden_harm_ladder_verdict")
    out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_lanes_verdict=None).run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert not hasattr(out, "hidden_harm_ladder_lanes_verdict") and _np(out.cost).tobytes() == plain[0].tobytes() and np.array_equal(_np(out.safe), plain[1])
    for two in (dict(hidden_verdict=VG._hv()), dict(hidden_ladder_verdict=LVG._lv()), dict(hidden_impact_verdict=ILG._iv()),
                dict(hidden_harm_ladder_verdict=HG._hl())):
        with pytest.raises(ValueError, match="same two reserved cost columns"):
            PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_lanes_verdict=_hl(), **two)
    with pytest.raises(ValueError, match="hidden_harm_ladder_lanes_verdict"):
        PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_lanes_verdict=dict(users=LANE_USERS))


_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import torch
import rule_refusal_cases as RC
import test_hidden_harm_ladder_lanes_gpu as LG
from frenetix_occlusion.step import PlanningStep
k = RC.stack(torch, RC.turn_scene(0.5))
opt = dict(hidden_harm_ladder_lanes_verdict=LG._hl()) if sys.argv[1] == "with" else dict()
out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", **opt).run(k.sc.ego, k.sc.yaw, k.sc.v)
torch.cuda.synchronize()
print("child ok", hasattr(out, "hidden_harm_ladder_lanes_verdict"))
'''


def test_a_step_without_the_option_launches_no_kernel_of_the_new_name(torch_cuda, tmp_path, monkeypatch):
    """a planning step without the option launches no hidden-traffic kernel at all; the same step with it launches the new kernel once --
    and not its head-on sibling -- and everything the plain step launches"""
    import re
    monkeypatch.setattr(HG, "_TRACE_CHILD", _TRACE_CHILD)
    without = HG._kernel_names(tmp_path, "without")
    assert "fo_grid_kernel" in without
    for name in ("fo_hr_", "fo_hc_", "fo_hidden_poses_kernel"):
        assert name not in without, name
    with_ = HG._kernel_names(tmp_path, "with")
    assert sum("fo_hr_brake_harm_ladder_lanes_kernel" in line for line in with_.splitlines()) == 1
    assert "fo_hidden_poses_kernel" in with_ and "fo_hr_brake_harm_ladder_kernel" not in with_ and "fo_hr_brake_impact_lanes_kernel" not in with_
    names = lambda text: set(re.findall(r"fo_\w+_kernel", text))
    assert names(without) and names(without) <= names(with_), sorted(names(without) - names(with_))


# ------------------------------------------------------------------------------------------------ 6. every byte is written
def test_every_byte_of_every_output_is_written(torch_cuda):
    """the outputs are pre-filled with 0xA5: after a call no element holds it, at M below, at and above a multiple of the trajectories per
    workgroup, with one wave per trajectory and with four, with and without lengths and finite flags, every class lane-bound"""
    torch = torch_cuda
    sm, _ = UG._parked()
    _moves(sm, LC.table("cross"))
    sc = LVG._scene(HG.TIE_SCENES[31])
    for L, B in ((5, 5), (23, 9)):
        levels = LS.levels_of(L)
        per = expected_plan(31, 3, 5, L, B, sc.M)[2]
        for M in sorted({1, max(per - 1, 1), per, per + 1, sc.M}):
            for ragged, finite in ((False, None), (True, np.arange(M, dtype=np.uint8) % 2)):
                cut = HG._cut(sc, 0, M)
                if not ragged:
                    cut.lens = None
                rc, msg, out = _raw(torch, sm, cut, levels, B, 0.1, 0b11111, finite=finite)
                assert rc == 0, msg
                HG._assert_written(out, (L, B, M, ragged))
                assert not HG._untouched(out)
                if finite is not None:
                    closed = finite == 0
                    assert (out.user[closed] == -2).all() and (out.harm_at[closed] == 1.0).all() and (out.user_at[closed] == -2).all()
                    assert (out.need[closed] == L).all() and (out.user[~closed] >= -1).all() and (out.user_at[~closed] >= -1).all()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_in_their_order_leave_everything_alone(torch_cuda):
    """the harm ladder's list in its order, then dir_mask, cos_h / sin_h and, FO_E_STATE, no move table with a lane-bound class: each
    refusal alone and paired with the next, of which the earlier one is named"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, _ = UG._parked()
    _moves(sm, LC.table("cross"))
    sc = LVG._scene((233, 2, 31, False, 2, "2", 1, 1))
    cap = sc.r2_caps[0]
    cost0, safe0 = np.full((2, 16), 0.5), np.ones(2, dtype=np.uint8)
    levels = [1.0, 4.0, 8.0]

    def call(levels=levels, B=5, cost=cost0, safe=safe0, harm_limit=0.1, mask=0b11, slack=0.0, **kw):
        kw.setdefault("finite", np.ones(2, dtype=np.uint8))
        kw.setdefault("a_limit", 4.0)
        return _raw(torch, sm, sc, levels, B, harm_limit, mask, slack, cost=cost, safe=safe, **kw)

    def refused(what, code=N.FO_E_ARG, **kw):
        rc, msg, out = call(**kw)
        assert rc == code and msg.startswith("fo_scene_hidden_brake_harm_ladder_lanes:") and what in msg, (what, rc, msg)
        assert HG._untouched(out), what                                                 # nothing was launched: every byte of the pattern stands
        assert (out.cost is None or (out.cost == 0.5).all()) and (out.safe is None or (out.safe == 1).all()), what

    rc, msg, out = call()
    assert rc == N.FO_OK and (out.cost[:, 14:] != 0.5).all(), msg
    HG._assert_written(out, "served")
    order = [("K = 0", dict(K=0)), ("C = 9", dict(C=9)), ("h_thr", dict(h_thr=None)), ("window", dict(win_nx=0)), ("r2_cap[0]", dict(r2_caps=[-1, cap])),
             ("map_of[1] = 2", dict(map_of=(0, 2))), ("M = -1", dict(count=-1)), ("L = 0", dict(L=0)), ("h_levels [L]", dict(h_levels=None)),
             ("h_levels[1]", dict(levels=[1.0, float("nan"), 8.0])), ("strictly ascending", dict(levels=[1.0, 1.0, 8.0])), ("dt", dict(dt=0.0)),
             ("a_limit", dict(a_limit=float("nan"))), ("T = 255", dict(T=255)), ("B = 0", dict(B=0)),
             ("decreases", dict(thr=np.array([[5, 4] + [9] * 29, [9] * 31]))), ("d_x", dict(drop=("d_y",))),
             ("d_key[1]", dict(drop_map=(("d_qmin", 1),))), ("d_v", dict(drop=("d_arc",))), ("d_need", dict(drop=("d_decel",))),
             ("go together", dict(cost=None)), ("half extents", dict(hl=-0.1)), ("d_speed_of", dict(d_speed_of=None)),
             ("d_harm_rows", dict(d_harm_rows=None)), ("harm_limit", dict(harm_limit=float("nan"))), ("dir_mask", dict(mask=0b100)),
             ("cos_h", dict(cos_h=1.5))]
    for what, kw in order:
        refused(what, **kw)
    for (what, kw), (_, later) in zip(order, order[1:]):            # of two faults the one earlier in the order is named
        if set(kw) & set(later) or {"levels", "L", "h_levels"} >= set(kw) | set(later):
            continue
        refused(what, **dict(kw, **later))
    refused("dir_mask", mask=0x80000000)
    for bad in (float("nan"), float("inf"), -1.0000001):
        refused("cos_h", cos_h=bad)
        refused("cos_h", sin_h=bad)
    refused("harm_limit", harm_limit=-0.5, mask=0b100)
    for name in ("d_need", "d_at", "d_blocking", "d_user", "d_decel", "d_need_of", "d_first", "d_harm_at", "d_user_at"):
        refused("d_need", drop=(name,))
    assert FG._set_moves(sm, None) == N.FO_OK                                            # no move table
    refused("move table", code=N.FO_E_STATE)
    refused("cos_h", cos_h=float("nan"))                                                # ... behind the two argument refusals
    rc, msg, out = call(mask=0)                                                         # ... and nobody reads it without a lane-bound class
    assert rc == N.FO_OK, msg
    HG._assert_written(out, "no table, no lane-bound class")
    rc, msg, out = call(count=0, harm_limit=float("nan"), mask=0b100)                   # M = 0: FO_OK, nothing launched, nothing looked at behind it
    assert rc == N.FO_OK and HG._untouched(out)
    _moves(sm, LC.table("cross"))
    ctx = N.Context(0)                                                                  # a context without a map
    assert ctx._lib.fo_scene_hidden_brake_harm_ladder_lanes(ctx._h, C.byref(N.HiddenBrakeHarmLadderLanes()), None) == N.FO_E_STATE


def test_refusals_of_the_python_layer(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    k.sm.launch(k.sc.ego, k.sc.yaw)
    call = lambda **over: k.sm.hidden_brake_harm_ladder_lanes(*k.tr[:4], **_hl(**over))
    cost = torch.zeros((RC.M, 16), dtype=torch.float64, device=k.sm.device)
    safe = torch.ones((RC.M,), dtype=torch.uint8, device=k.sm.device)
    for bad in (dict(heading_slack=-0.1), dict(heading_slack=float("nan")), dict(heading_slack=float("inf")), dict(heading_slack="wide"),
                dict(starts=0), dict(starts=17), dict(harm_limit=-1.0), dict(a_limit=float("nan")), dict(levels=[2.0, 1.0]),
                dict(levels=None, a_limit=math.inf), dict(kinds=STEP_KINDS[:2]), dict(ego_mass=0.0), dict(cost=cost), dict(safe=safe), dict(users=())):
        with pytest.raises(ValueError, match="hidden_brake_harm_ladder_lanes"):
            call(**bad)
    with pytest.raises(TypeError):
        call(approach="lanes")
    moves, k.sm.lane_moves = k.sm.lane_moves, None
    try:
        with pytest.raises(ValueError, match="lane_moves"):
            call()
        call(users=tuple((s, m, "any") for s, m, _ in LANE_USERS))     # nobody is lane-bound: served without a table
    finally:
        k.sm.lane_moves = moves
    assert (cost == 0).all() and (safe == 1).all()
    hl = call(cost=cost, safe=safe, heading_slack=4.0)                 # h >= pi: head-on for everybody
    head = k.sm.hidden_brake_harm_ladder(*k.tr[:4], **{key: v for key, v in _hl().items() if key != "heading_slack"})
    torch.cuda.synchronize()
    for name in RH.OUTPUTS:
        assert torch.equal(getattr(hl, name), getattr(head, name)), name
    assert torch.equal(cost[:, RH.C_RES0], hl.decel)
