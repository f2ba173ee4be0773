"""Hidden-traffic harm ladder on the device (fo_scene_hidden_brake_harm_ladder, SensorModel.hidden_brake_harm_ladder,
FOInterface.hidden_brake_harm_ladder, PlanningStep(hidden_harm_ladder_verdict=); DESIGN.md §5.10 "Harm ladder"): the tie to
fo_scene_hidden_brake_ladder_verdict at harm_limit = 0 on the smallest shapes at which the lane layout switches, the consequences of
the definition on the same shapes, the plain statement tests/ref_hidden_brake_harm_ladder.py on the walk
fo_scene_hidden_brake_ladder_users writes on the same device inputs, fo_scene_hidden_brake_impact per level, a hand case with the
numbers written out, a non-monotone case, the fold on the cost rows a real planning step left, the step with and without the stage,
the interface's defaults, pre-filled outputs, the refusals.  Integers and decel are compared exactly, harms to 1e-9 -- the scenes hold
no open comparison (tests/test_hidden_harm_ladder_cpu.py).  Every test runs under a time limit of its own that ends the process (a hung
kernel cannot be waited out from Python); no test provokes a fault."""
import faulthandler
import glob
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_ladder_scenes as LS
import hidden_brake_ladder_users_scenes as S
import hidden_brake_scenes as SC
import hidden_harm_ladder_cases as HC
import hidden_impact_cases as IC
import ref_hidden_brake_harm_ladder as RH
import rule_refusal_cases as RC
import test_hidden_brake_ladder_users_gpu as LUG
import test_hidden_brake_ladder_verdict_gpu as LVG
import test_hidden_brake_users_gpu as UG
import test_hidden_brake_verdict_gpu as VG
import test_hidden_impact_gpu as IG
import test_hidden_reach_gpu as T
from test_hidden_brake_ladder_verdict_cpu import expected_plan
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
STEP_LIMIT = 240          # seconds a test may take before the process is ended with every thread's traceback
TOL = 1e-9                # the family's float tolerance (README, "GPU vs oracle")
PATTERN = 0xA5            # the byte every output buffer is filled with before a call
PAT_I32 = int(np.frombuffer(bytes([PATTERN] * 4), dtype=np.int32)[0])
PAT_F64 = float(np.frombuffer(bytes([PATTERN] * 8), dtype=np.float64)[0])
INT_OUTPUTS, F64_OUTPUTS = ("need", "at", "blocking", "user", "need_of", "first", "user_at"), ("decel", "harm_at")
USERS, VEH3 = VG.USERS, RC.VEH[:3]
STEP_KINDS = IG.STEP_KINDS
LEVELS5 = LVG.LEVELS5
MID = 0.5                 # a limit between 0 and inf for the monotony of need in the limit (no comparison with a checker rests on it)


@pytest.fixture(autouse=True)
def _time_limit(request):
    faulthandler.dump_traceback_later(getattr(request.module, request.function.__name__ + "_limit", STEP_LIMIT), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw(torch, sm, sc, levels, B, harm_limit, rows=None, speed_of=None, a_limit=np.inf, keys=None, qmins=None, thr=None, map_of=None,
         r2_caps=None, finite=None, cost=None, safe=None, drop=(), drop_map=(), **over):
    """fo_scene_hidden_brake_harm_ladder on scene ``sc`` (or on edited data of it); every byte of the output buffers is pre-filled with
    PATTERN.  Arrays that are the same object go up once: two such maps are the same buffer.  ``rows`` / ``speed_of``: None = those of
    tests/hidden_harm_ladder_cases.pricing.  ``cost`` / ``safe``: host arrays, uploaded and returned as the call left them; ``drop`` /
    ``drop_map`` / ``over`` as in tests/test_hidden_brake_ladder_verdict_gpu._raw.  Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
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
    # (not through up(): that keys on the identity of arrays the caller holds, and these two are made here)
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
    kw = dict(M=over.pop("count", M), T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=HL, hw=HW, wb=WB, win_ix0=win[0],
              win_iy0=win[1], win_nx=win[2], win_ny=win[3], K=Kn, C=Cn, d_key=(C.c_void_p * 3)(*ptrs["d_key"]), d_qmin=(C.c_void_p * 3)(*ptrs["d_qmin"]),
              r2_cap=(C.c_int32 * 3)(*pad([int(r) for r in r2_caps], 3, -5)), map_of=(C.c_int32 * 8)(*pad([int(k) for k in map_of], 8, 99)),
              d_v=p(tv), d_arc=p(ta), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), L=Ln, B=int(B), dt=float(sc.dt),
              h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), a_limit=float(a_limit), d_finite_or_null=p(tf), d_cost_or_null=p(tc),
              d_safe_or_null=p(ts), d_need=p(out.need), d_at=p(out.at), d_blocking=p(out.blocking), d_user=p(out.user), d_decel=p(out.decel),
              d_need_of=p(out.need_of), d_first=p(out.first), d_speed_of=p(tsp), d_harm_rows=p(trow), harm_limit=float(harm_limit),
              d_harm_at=p(out.harm_at), d_user_at=p(out.user_at))
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeHarmLadder(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_harm_ladder(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    res = SimpleNamespace(**{k: _np(getattr(out, k)) for k in RH.OUTPUTS})
    res.cost, res.safe = (None if tc is None else _np(tc)), (None if ts is None else _np(ts))
    return rc, msg, res


def _untouched(out):
    """every output still holds the pattern in every byte"""
    return all((getattr(out, k).view(np.uint8) == PATTERN).all() for k in RH.OUTPUTS)


def _assert_written(out, what):
    """no element of any output still holds the pattern (no result is the pattern's number: an int32 below -10^9, a float64 of
    magnitude 10^-127)"""
    for k in INT_OUTPUTS:
        assert (getattr(out, k) != PAT_I32).all(), (what, k)
    for k in F64_OUTPUTS:
        assert (getattr(out, k) != PAT_F64).all(), (what, k)


def _cut(sc, lo, hi):
    """rows [lo, hi) of a scene's candidates: a scene of its own on the same maps"""
    cut = lambda a: None if a is None else np.ascontiguousarray(a[lo:hi])
    return SimpleNamespace(x=cut(sc.x), y=cut(sc.y), head=cut(sc.head), v=cut(sc.v), arc=cut(sc.arc), lens=cut(sc.lens), win=sc.win, dt=sc.dt,
                           keys=sc.keys, qmins=[cut(q) for q in sc.qmins], thr=sc.thr, map_of=sc.map_of, r2_caps=sc.r2_caps, users=sc.users,
                           T=sc.T, M=hi - lo)


def _ends(sc, B):
    lens = np.full(sc.x.shape[0], sc.T) if sc.lens is None else np.clip(sc.lens, 0, sc.T)
    return np.minimum(lens, B)


def _consequences(torch, sm, sc, levels, B, what, **edited):
    """(a), (b), (d) on one scene: at harm_limit = 0 the seven shared outputs and the folded rows are
    fo_scene_hidden_brake_ladder_verdict's bit for bit; at +inf need = 0 wherever there is a manoeuvre; need never rises with the limit
    and never exceeds the ladder verdict's; the curve does not depend on the limit"""
    M = sc.x.shape[0]
    rng = np.random.default_rng(M * 131 + B)
    cost0, safe0 = rng.random((M, 16)), (np.arange(M) % 3 != 0).astype(np.uint8)
    a_limit = float(levels[len(levels) // 2])
    rc, msg, lv = LVG._raw(torch, sm, sc, levels, B, a_limit=a_limit, cost=cost0, safe=safe0, **edited)
    assert rc == 0, (what, msg)
    outs = {}
    for limit in (0.0, MID, math.inf):
        rc, msg, outs[limit] = _raw(torch, sm, sc, levels, B, limit, a_limit=a_limit, cost=cost0, safe=safe0, **edited)
        assert rc == 0, (what, limit, msg)
        _assert_written(outs[limit], (what, limit))
    zero, mid, inf = outs[0.0], outs[MID], outs[math.inf]
    for name in RH.SHARED:                                                              # (a)
        got, want = getattr(zero, name), getattr(lv, name)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, name, np.argwhere(got != want)[:4].tolist())
    assert zero.cost.tobytes() == lv.cost.tobytes() and np.array_equal(zero.safe, lv.safe), what
    ends = _ends(sc, B)
    assert np.array_equal(inf.need, np.where(ends > 0, 0, -1)), what                    # (b)
    assert (inf.need <= mid.need).all() and (mid.need <= zero.need).all() and (inf.need_of <= mid.need_of).all(), what    # (d)
    for o in (mid, inf):
        assert o.harm_at.tobytes() == zero.harm_at.tobytes() and np.array_equal(o.user_at, zero.user_at) and np.array_equal(o.first, zero.first), what
    L = len(levels)                                                                     # (c), in the device's own arithmetic
    below = mid.harm_at <= MID
    lowest = np.where(below.any(axis=1), below.argmax(axis=1), L)
    asked = mid.need >= 0
    assert (mid.need[asked] <= lowest[asked]).all() and (mid.harm_at[mid.need == L] > MID).all(), what
    assert ((zero.user_at == -1) == (zero.harm_at == 0.0)).all() and (zero.harm_at[ends == 0] == 0.0).all() and (zero.harm_at < 1.0).all(), what
    return zero, mid


# ------------------------------------------------------------------------------------------------ 1. the tie and the consequences
# (seed, M, T, ragged, C, layout, L, B) of tests/hidden_brake_ladder_users_scenes.scene: those of the ladder verdict's tie at T = 1, 2, 31 and
# one at T = 65 -- M is at least the largest per_block + 1 of the plan at that T (8 at T = 65: the rows decide)
TIE_SCENES = {1: LVG.TIE_SCENES[1], 2: LVG.TIE_SCENES[2], 31: LVG.TIE_SCENES[31], 65: (265, 12, 65, True, 5, "3", 1, 1)}
LADDERS = (1, 2, 23, 32, 33, 64)


def _tie_starts(T_, L):
    """B in {1, 2, 5, T}; with L = 23 (Lp = 32) also 3 and 9: G = 64 / 128 / 256 / 256 in two rounds at B = 2 / 3 / 5 / 9"""
    return sorted({b for b in (1, 2, 5, T_) + ((3, 9) if L == 23 else ()) if b <= T_})


@pytest.mark.parametrize("T_", sorted(TIE_SCENES))
def test_limit_zero_is_the_ladder_verdict_at_every_form_of_the_plan(torch_cuda, T_):
    """T in {1, 2, 31, 65} x L in {1, 2, 23, 32, 33, 64} x B in {1, 2, 5, T} (3 and 9 at L = 23) with M at per_block - 1 and per_block + 1 on the
    scene's FIRST rows (lengths 0, 1, 2 lead them) and at per_block on its LAST rows: consequence (a) bit for bit on all seven shared
    outputs and the folded rows, and (b), (c), (d) on the same calls -- G from 1 to 256, one round and several, five users on three maps"""
    torch = torch_cuda
    sm, road = UG._parked()
    sc = LVG._scene(TIE_SCENES[T_])
    assert np.array_equal(road, sc.road) and len(sc.keys) == 3 and sc.lens[:3].tolist() == [0, 1, 2]
    groups, moved, hit = set(), 0, 0
    for L in LADDERS:
        levels = LS.levels_of(L)
        for B in _tie_starts(T_, L):
            _, G, per, _, _ = expected_plan(T_, 3, 5, L, B, sc.M)
            groups.add(G)
            for lo, hi in sorted({(0, max(per - 1, 1)), (0, per + 1), (sc.M - per, sc.M)}):
                assert 0 <= lo < hi <= sc.M
                zero, mid = _consequences(torch, sm, _cut(sc, lo, hi), levels, B, (T_, L, B, lo, hi))
                moved, hit = moved + int((mid.need < zero.need).sum()), hit + int((zero.harm_at > 0).sum())
    assert groups == {1: {1, 2, 32, 64}, 2: {1, 2, 4, 32, 64, 128}}.get(T_, {1, 2, 4, 8, 16, 32, 64, 128, 256})
    print(f"T = {T_}: {hit} (trajectory, level) pairs with a hit, need lowered by the limit {MID} at {moved} candidates")
    assert T_ < 31 or (hit > 0 and moved > 0)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C_", [1, 4, 5, 8])
def test_limit_zero_is_the_ladder_verdict_over_class_and_map_counts(torch_cuda, C_, K):
    """C in {1, 4, 5, 8} x K in {1, 2, 3}: all six instantiations, widths with classes that are not there, class c on map (c + 1) % K --
    and, with K >= 2, maps that are the very same BUFFER"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc = LVG._scene((232, 20, 31, True, 8, "3", 1, 1))
    edited = dict(keys=sc.keys[:K], qmins=sc.qmins[:K], map_of=[(c + 1) % K for c in range(C_)], r2_caps=sc.r2_caps[:K], thr=sc.thr[:C_])
    seen = set()
    for L, B in ((23, 5), (2, 31), (1, 1)):
        zero, mid = _consequences(torch, sm, sc, LS.levels_of(L), B, (C_, K, L, B), **edited)
        seen |= set(zero.user_at.ravel().tolist()) | set(zero.user.tolist())
        assert (zero.blocking < (1 << C_)).all() and (zero.user_at < C_).all()
    assert -1 in seen and len(seen) >= 2
    if K >= 2:
        same = dict(edited, keys=[sc.keys[0]] * K, qmins=[sc.qmins[0]] * K)
        _consequences(torch, sm, sc, LS.levels_of(5), 5, (C_, K, "one buffer"), **same)


# ------------------------------------------------------------------------------------------------ 2. the checker
def _walk(torch, sm, sc, levels, B, **edited):
    """fo_scene_hidden_brake_ladder_users with its detail on the scene: brake_first, stop and first, what the stage is defined on"""
    rc, msg, lu = LUG._raw(torch, sm, sc, detail=True, levels=np.asarray(levels, dtype=np.float64), B=B, **edited)
    assert rc == 0, msg
    return lu


def _assert_checker(out, want, what):
    """integers exactly, decel bit for bit, harm_at to 1e-9; returns the worst harm difference"""
    for name in INT_OUTPUTS:
        got, w = getattr(out, name), want[name]
        assert got.dtype == np.int32 and got.shape == w.shape and np.array_equal(got, w), (what, name, np.argwhere(got != w)[:4].tolist())
    assert out.decel.dtype == np.float64 and out.decel.tobytes() == want["decel"].tobytes(), (what, "decel")
    worst = float(np.abs(out.harm_at - want["harm_at"]).max()) if want["harm_at"].size else 0.0
    assert out.harm_at.dtype == np.float64 and out.harm_at.shape == want["harm_at"].shape and worst <= TOL, (what, "harm_at", worst)
    return worst


@pytest.mark.parametrize("spec", HC.CHECKER_CASES, ids=lambda s: "-".join(str(v) for v in s))
def test_checker_on_the_walk_of_the_ladder_users_entry(torch_cuda, spec):
    """every raw-entry case at its three limits -- 0, inf and the one strictly between two of the scene's own harms -- against the plain
    statement on what fo_scene_hidden_brake_ladder_users writes on the same device inputs: integers exactly, decel bit for bit, harm_at
    to 1e-9"""
    torch = torch_cuda
    sm, road = UG._parked()
    sc = S.scene(*spec)
    assert np.array_equal(road, sc.road)
    lu = _walk(torch, sm, sc, sc.levels, sc.starts)
    hits = HC.check(sc, lu, 0.0)["hits"]
    worst = 0.0
    for limit in HC.limits(hits):
        assert limit is not None and np.abs(np.array(hits) - limit).min() >= RH.OPEN_TOL
        want = HC.check(sc, lu, limit)
        assert want["closest"] >= RH.OPEN_TOL
        rc, msg, out = _raw(torch, sm, sc, sc.levels, sc.starts, limit)
        assert rc == 0, msg
        _assert_written(out, (spec, limit))
        worst = max(worst, _assert_checker(out, want, (spec, limit)))
    print(f"{spec}: worst |harm_at - checker| = {worst:.3e} over {len(hits)} hits, in-between limit {HC.limits(hits)[2]:.6f}")


def test_each_level_is_the_impact_verdict_at_that_deceleration(torch_cuda):
    """(e): harm_at[:, l] is the obstacle harm of fo_scene_hidden_brake_impact at a_brake = levels[l] on the same inputs, to 1e-9, and
    user_at its user exactly (the scenes hold no open choice) -- on 23 levels from every start, on ragged lengths, on a trajectory over
    two waves"""
    torch = torch_cuda
    sm, _ = UG._parked()
    worst, users = 0.0, set()
    for spec in (HC.CHECKER_CASES[0], HC.CHECKER_CASES[1], HC.CHECKER_CASES[3], HC.CHECKER_CASES[4]):
        sc = S.scene(*spec)
        _, rows, speed_of = HC.pricing(sc)
        rc, msg, out = _raw(torch, sm, sc, sc.levels, sc.starts, 0.1)
        assert rc == 0, msg
        for l, level in enumerate(sc.levels):
            rc, msg, iv = IG._raw_impact(torch, sm, sc.win, sc.r2_caps, sc.keys, sc.qmins, sc.x, sc.y, sc.head, sc.v, sc.arc, float(level), sc.dt,
                                         sc.thr, sc.map_of, sc.starts, rows, speed_of, lens=sc.lens)
            assert rc == 0, msg
            diff = float(np.abs(out.harm_at[:, l] - iv.harm[:, 0]).max())
            assert diff <= TOL and np.array_equal(out.user_at[:, l], iv.user), (spec, l, diff)
            worst, users = max(worst, diff), users | set(iv.user.tolist())
    print(f"worst |harm_at - impact verdict's obstacle harm| = {worst:.3e}; users {sorted(users)}")
    assert len(users) >= 3


# ------------------------------------------------------------------------------------------------ 3. cases with known numbers
def test_hand_case_with_known_numbers(torch_cuda):
    """tests/hidden_harm_ladder_cases.hand_case: one candidate, levels 2 and 4 m/s^2, a pedestrian and a car behind a wall.  Both levels
    are hit moving, so the ladder verdict says "no level"; the pedestrian's harm is 0.2674 at 2 m/s^2 and 0.1755 at 4 m/s^2, the car's a
    few percent: with harm_limit = 0.2 this stage says level 1, 4 m/s^2, kept from level 0 by the pedestrian"""
    torch = torch_cuda
    sm, road = UG._parked()
    h = HC.hand_case()
    assert np.array_equal(road, h.road)
    rc, msg, lv = LVG._raw(torch, sm, h, h.levels, 1)
    assert rc == 0, msg
    assert (lv.need.tolist(), lv.decel.tolist(), lv.blocking.tolist()) == ([2], [math.inf], [0b11])                 # "no level"
    rc, msg, out = _raw(torch, sm, h, h.levels, 1, HC.HAND_LIMIT, rows=h.rows, speed_of=h.speed_of)
    assert rc == 0, msg
    assert (out.need.tolist(), out.at.tolist(), out.blocking.tolist(), out.user.tolist(), out.decel.tolist()) == ([1], [0], [0b01], [0], [4.0])
    assert out.need_of.tolist() == [[1], [0]] and out.first.tolist() == [[2], [2]] and out.user_at.tolist() == [[0, 0]]
    assert abs(out.harm_at[0, 0] - HC.HAND_PED[0]) <= TOL and abs(out.harm_at[0, 1] - HC.HAND_PED[1]) <= TOL, out.harm_at.tolist()
    assert abs(HC.HAND_PED[1] - 1.0 / (1.0 + math.exp(3.164 - 0.26951159804844643 * 6.0))) <= 1e-15            # the formula, not the digits
    # the car alone: its harm stays below the limit at both levels -> level 0 suffices, though it is hit
    rc, msg, car = _raw(torch, sm, h, h.levels, 1, HC.HAND_LIMIT, rows=h.rows[1:], speed_of=h.speed_of[1:], thr=h.thr[1:], map_of=[0])
    assert rc == 0 and (car.need.tolist(), car.decel.tolist(), car.user.tolist()) == ([0], [2.0], [-1]), msg
    assert abs(car.harm_at[0, 0] - HC.HAND_CAR[0]) <= TOL and abs(car.harm_at[0, 1] - HC.HAND_CAR[1]) <= TOL


def test_harder_braking_is_not_always_safer(torch_cuda):
    """tests/hidden_harm_ladder_cases.non_monotone_case: hit at the middle level only -- harm_at is (0, h, 0), .monotone() is False, and
    need is the FIRST sufficient level, 0"""
    torch = torch_cuda
    from frenetix_occlusion.hidden_traffic import HiddenBrakeHarmLadder
    sm, _ = UG._parked()
    n = HC.non_monotone_case()
    rc, msg, out = _raw(torch, sm, n, n.levels, 1, 0.05, rows=n.rows, speed_of=n.speed_of)
    assert rc == 0, msg
    assert out.harm_at[0, 0] == 0.0 < out.harm_at[0, 1] and out.harm_at[0, 2] == 0.0 and out.user_at[0].tolist() == [-1, 0, -1]
    assert out.harm_at[0, 1] > 0.05 and out.need[0] == 0 and out.decel[0] == 0.0
    res = HiddenBrakeHarmLadder(**{k: torch.as_tensor(getattr(out, k)) for k in RH.OUTPUTS}, levels=n.levels, starts=1, harm_limit=0.05,
                                a_limit=math.inf, rows=n.rows, speed_of=np.array(n.speed_of))
    assert res.monotone().tolist() == [False, False, False]
    levels, harm_at, user_at = res.harm_curve()
    assert levels is n.levels and harm_at is res.harm_at and user_at is res.user_at


# ------------------------------------------------------------------------------------------------ 4. the fold on the device
def _hl(**over):
    kw = dict(vehicle=VEH3, ego_mass=RC.VEH[3], users=USERS, kinds=STEP_KINDS, dt=0.1, levels=LEVELS5, starts=5, harm_limit=0.1, a_limit=4.0)
    kw.update(over)
    return kw


def _step_then_stage(torch, k, tr=None, **over):
    """a plain PlanningStep.run, its cost / safe copied, then the stage by its own call (on ``tr`` where given): (before, after, result)"""
    from frenetix_occlusion.step import PlanningStep
    tr = k.tr if tr is None else tr
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced")
    out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    assert not hasattr(out, "hidden_harm_ladder_verdict")
    before = (out.cost.clone(), out.safe.clone())
    hl = k.sm.hidden_brake_harm_ladder(*tr[:4], cost=out.cost, safe=out.safe, **_hl(**over))
    torch.cuda.synchronize()
    return (_np(before[0]), _np(before[1])), (_np(out.cost), _np(out.safe)), hl


def _assert_fold(before, after, hl, a_limit):
    cost0, safe0 = before
    cost1, safe1 = after
    need, user, decel = _np(hl.need), _np(hl.user), _np(hl.decel)
    want_cost, want_safe = RH.fold(cost0, safe0, need, user, decel, len(hl.levels), a_limit)
    assert cost1.tobytes() == want_cost.tobytes() and np.array_equal(safe1, want_safe)
    others = [c for c in range(16) if c not in (RH.C_SAFE, RH.C_RES0, RH.C_RES1)]
    assert cost1[:, others].tobytes() == cost0[:, others].tobytes()             # bit-identical, NaNs included
    assert (safe1 <= safe0).all()                                               # only ever 1 -> 0
    assert cost1[:, RH.C_RES0].tobytes() == decel.tobytes() and np.array_equal(cost1[:, RH.C_RES1], user.astype(np.float64))
    assert np.array_equal(decel, np.where(need < 0, 0.0, np.append(hl.levels, np.inf)[np.clip(need, 0, len(hl.levels))]))


def _device_tie(torch, k, hl, x=None, v=None):
    """the tie through the Python layer: the ladder-users entry with its detail on the very device data the stage walked on, then the
    checker -- held to the no-open-comparison condition on what it reads back"""
    w = k.sm.window
    x, y, v = (_np(k.tr[0]) if x is None else x), _np(k.tr[1]), (_np(k.tr[3]) if v is None else v)
    sc = SimpleNamespace(x=x, y=y, head=_np(hl.poses.heading), v=v, arc=_np(hl.poses.arc), lens=None, win=(w.ix0, w.iy0, w.nx, w.ny), dt=0.1,
                         keys=[_np(c.key) for c in hl.clearances], qmins=[_np(c.qmin) for c in hl.clearances], thr=hl.thr, map_of=hl.map_of,
                         r2_caps=[c.r2_cap for c in hl.clearances], levels=hl.levels, starts=hl.starts, T=RC.T)
    lu = _walk(torch, k.sm, sc, hl.levels, hl.starts)
    rows = IC.rows_of(STEP_KINDS, RC.VEH[3])
    assert np.abs(hl.rows - rows).max() <= 1e-15 and hl.speed_of.tolist() == [u[0] for u in USERS]
    want = RH.harm_ladder(lu.brake_first, lu.stop, lu.first, v, list(hl.levels), 0.1, hl.starts, hl.rows.tolist(), hl.speed_of.tolist(), hl.harm_limit,
                          None, _np(hl.poses.finite))
    assert want["closest"] >= RH.OPEN_TOL and (not want["hits"] or np.abs(np.array(want["hits"]) - hl.harm_limit).min() >= RH.OPEN_TOL)
    return _assert_checker(SimpleNamespace(**{n: _np(getattr(hl, n)) for n in RH.OUTPUTS}), want, "the Python layer"), want


def test_fold_on_the_rows_of_a_real_step(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    before, after, hl = _step_then_stage(torch, k)
    assert before[1].any() and not np.isnan(before[0][:, :12]).all()
    _assert_fold(before, after, hl, 4.0)
    worst, want = _device_tie(torch, k, hl)
    assert hl.starts == 5 and hl.harm_limit == 0.1 and hl.a_limit == 4.0 and hl.map_of == (0, 1, 0) and hl.levels.tolist() == LEVELS5
    assert torch.equal(hl.critical_user(), hl.user.to(torch.int64)) and hl.required_deceleration() is hl.decel
    assert torch.equal(hl.brake_threat_number(8.0), hl.decel / 8.0)
    need, harm_at = _np(hl.need), _np(hl.harm_at)
    print(f"step rows: need {sorted(set(need.tolist()))}, harm_at min {harm_at.min():.4f} max {harm_at.max():.4f}, worst |harm_at - checker| "
          f"{worst:.3e}, monotone {int(_np(hl.monotone()).sum())} of {len(need)}")
    assert (harm_at > 0.0).any() and (harm_at < 1.0).all()
    # the ladder verdict on the same rows never asks for less, and asks for more somewhere: the stage is finite where "clear" is not
    lv = k.sm.hidden_brake_ladder_verdict(*k.tr[:4], **LVG._lv())
    torch.cuda.synchronize()
    assert (need <= _np(lv.need)).all() and torch.equal(hl.first, lv.first)
    print(f"need below the ladder verdict's at {int((need < _np(lv.need)).sum())} of {len(need)} candidates")
    # a_limit = +inf takes safety only where no level suffices; harm_limit = 0 is the ladder verdict, folded rows included
    before, after, hl2 = _step_then_stage(torch, k, a_limit=math.inf)
    _assert_fold(before, after, hl2, math.inf)
    assert np.array_equal(after[1], np.where(_np(hl2.need) == 5, 0, before[1]))
    for name in RH.OUTPUTS:
        assert torch.equal(getattr(hl2, name), getattr(hl, name)), name
    before, after, hl0 = _step_then_stage(torch, k, harm_limit=0.0)
    for name in RH.SHARED:
        assert torch.equal(getattr(hl0, name), getattr(lv, name)), name
    _assert_fold(before, after, hl0, 4.0)


def test_a_refused_step_stays_unsafe_and_gets_the_two_columns(torch_cuda):
    torch = torch_cuda
    import test_rule_refusal_gpu as RG
    k = VG._stack(torch, RG.REFUSING_CELL)
    before, after, hl = _step_then_stage(torch, k)
    RG.assert_refused(SimpleNamespace(cost=torch.as_tensor(before[0]), safe=torch.as_tensor(before[1])))
    _assert_fold(before, after, hl, 4.0)
    assert not after[1].any() and (after[0][:, RH.C_SAFE] == 0.0).all()
    others = [c for c in range(14) if c != RH.C_SAFE]
    assert np.isnan(after[0][:, others]).all() and after[0][:, RH.C_RES0].tobytes() == _np(hl.decel).tobytes()


def test_a_non_finite_candidate_fails_closed(torch_cuda):
    """a NaN, an inf and a -inf in x, theta and v of three candidates as the stage sees them: need = L, at = 0, blocking = 0, user = -2,
    decel = inf, harm_at = 1.0 and user_at = -2 at every level, and the flag is lost even at harm_limit = a_limit = inf, which take
    nothing else away"""
    torch = torch_cuda
    k = VG._stack(torch)
    tr = [t.clone() for t in k.tr]
    tr[0][3, 7], tr[2][11, 0], tr[3][40, 15] = float("nan"), float("inf"), float("-inf")
    before, after, hl = _step_then_stage(torch, k, tr=tr, harm_limit=math.inf, a_limit=math.inf)
    _assert_fold(before, after, hl, math.inf)
    need, at, blocking, user, decel, harm_at, user_at = (_np(getattr(hl, n)) for n in ("need", "at", "blocking", "user", "decel", "harm_at", "user_at"))
    for m in (3, 11, 40):
        assert (need[m], at[m], blocking[m], user[m], decel[m], after[1][m], after[0][m, RH.C_SAFE], after[0][m, RH.C_RES1]) == (5, 0, 0, -2, np.inf, 0, 0.0, -2.0), m
        assert harm_at[m].tolist() == [1.0] * 5 and user_at[m].tolist() == [-2] * 5 and after[0][m, RH.C_RES0] == np.inf
    rest = [m for m in range(RC.M) if m not in (3, 11, 40)]
    assert _np(hl.poses.finite).sum() == RC.M - 3 and (user[rest] >= -1).all() and (user_at[rest] >= -1).all() and np.array_equal(after[1][rest], before[1][rest])
    assert (need[rest] <= 0).all()


# ------------------------------------------------------------------------------------------------ 5. the planning step
def test_step_with_the_stage_is_the_stage_by_stage_calls(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion.step import PlanningStep
    k = VG._stack(torch)
    plain, staged, hl = _step_then_stage(torch, k)
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_verdict=_hl())
    for _ in range(2):                                              # (a second run folds into fresh rows, not into folded ones)
        out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
        torch.cuda.synchronize()
        assert _np(out.cost).tobytes() == staged[0].tobytes() and np.array_equal(_np(out.safe), staged[1])
        for name in RH.OUTPUTS:
            assert torch.equal(getattr(out.hidden_harm_ladder_verdict, name), getattr(hl, name)), name
    assert (_np(hl.harm_at) > 0.0).any()
    # None: no such attribute, and cost / safe are the step's
    out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_verdict=None).run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert not hasattr(out, "hidden_harm_ladder_verdict") and _np(out.cost).tobytes() == plain[0].tobytes() and np.array_equal(_np(out.safe), plain[1])
    for two in (dict(hidden_verdict=VG._hv()), dict(hidden_ladder_verdict=LVG._lv()), dict(hidden_impact_verdict=IG._iv())):
        with pytest.raises(ValueError, match="same two reserved cost columns"):
            PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_verdict=_hl(), **two)
    with pytest.raises(ValueError, match="hidden_harm_ladder_verdict"):
        PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_harm_ladder_verdict=dict(users=USERS))


_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import torch
import rule_refusal_cases as RC
import test_hidden_harm_ladder_gpu as HG
from frenetix_occlusion.step import PlanningStep
k = RC.stack(torch, RC.turn_scene(0.5))
opt = dict(hidden_harm_ladder_verdict=HG._hl()) if sys.argv[1] == "with" else dict()
out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", **opt).run(k.sc.ego, k.sc.yaw, k.sc.v)
torch.cuda.synchronize()
print("child ok", hasattr(out, "hidden_harm_ladder_verdict"))
'''


def _kernel_names(tmp_path, mode):
    """the kernel names of one planning step in a process of its own, taken the way tests/test_hidden_reach_gpu._kernel_names takes them"""
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"), tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + mode)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), mode],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and f"child ok {mode == 'with'}" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    return "\n".join(open(f).read() for f in files)


def test_a_step_without_the_option_launches_no_hidden_traffic_kernel(torch_cuda, tmp_path):
    """a planning step without the option launches no kernel of the hidden-traffic family at all -- neither the new one nor the pose
    preparation and clearances in front of it; the same step with it launches the new kernel once, and everything the plain step launches"""
    without = _kernel_names(tmp_path, "without")
    assert "fo_grid_kernel" in without
    for name in ("fo_hr_", "fo_hc_", "fo_hidden_poses_kernel"):
        assert name not in without, name
    with_ = _kernel_names(tmp_path, "with")
    assert sum("fo_hr_brake_harm_ladder_kernel" in line for line in with_.splitlines()) == 1
    assert "fo_hidden_poses_kernel" in with_ and "fo_hr_brake_ladder_verdict_kernel" not in with_ and "fo_hr_brake_impact_kernel" not in with_
    names = lambda text: set(re.findall(r"fo_\w+_kernel", text))
    assert names(without) and names(without) <= names(with_), sorted(names(without) - names(with_))


def test_through_the_interface(torch_cuda, tmp_path):
    """FOInterface.hidden_brake_harm_ladder on scenario 1: harm_limit from the configuration's metric_thresholds.harm, the levels 0.5, 1.0,
    ... up to a_max and a_limit = a_max, the default kinds by ascending speed with the dimensions of the agent manager's phantoms -- the
    sensor model's call with all of that spelled out, bit for bit"""
    torch = torch_cuda
    import test_hidden_witness_gpu as WG
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.hidden_traffic import default_brake_ladder
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    ego, yaw = WG._drive(fo, sc, 3)
    traj = SY.make_trajectories(64, 31, WG.DT, seed=WG.SEED, ego_pos=ego, ego_yaw=yaw)
    users = ((13.9, "road", "lanes"), (2.0, "road", "any"), (7.0, "road", "lanes"))       # not in order of speed on purpose
    hl = fo.hidden_brake_harm_ladder(traj, users, starts=5)
    want_kinds = (fo.phantom_kind("Car"), fo.phantom_kind("Pedestrian"), fo.phantom_kind("Bicycle"))
    limit = fo.config["metrics"]["metric_thresholds"]["harm"]
    veh = SY.VEHICLE_BMW320I
    assert hl.kinds == want_kinds and hl.harm_limit == (math.inf if limit is None else float(limit)) and hl.starts == 5 and hl.a_limit == veh[4]
    assert hl.levels.tolist() == default_brake_ladder(veh[4], "test") and len(hl.levels) == 23
    ref = fo.sensor_model.hidden_brake_harm_ladder(traj["x"], traj["y"], traj["theta"], traj["v"], vehicle=veh[:3], ego_mass=veh[3], users=users,
                                                   kinds=want_kinds, dt=WG.DT, levels=default_brake_ladder(veh[4], "test"), starts=5,
                                                   harm_limit=hl.harm_limit, a_limit=veh[4], margin=fo.occlusion_memory["margin"])
    torch.cuda.synchronize()
    for name in RH.OUTPUTS:
        assert torch.equal(getattr(hl, name), getattr(ref, name)), name
    assert np.abs(hl.rows - IC.rows_of(want_kinds, veh[3])).max() <= 1e-15 and tuple(hl.harm_at.shape) == (64, 23)
    named = fo.hidden_brake_harm_ladder(traj, users, kinds=("Car", "Pedestrian", want_kinds[2]), harm_limit=0.5, levels=[2.0, 8.0], starts=5, a_limit=4.0)
    assert named.kinds == want_kinds and named.harm_limit == 0.5 and named.levels.tolist() == [2.0, 8.0] and named.a_limit == 4.0
    with pytest.raises(ValueError, match="kinds is required"):
        fo.hidden_brake_harm_ladder(traj, users[:2])


# ------------------------------------------------------------------------------------------------ 6. every byte is written
def test_every_byte_of_every_output_is_written(torch_cuda):
    """the outputs are pre-filled with a byte pattern: after a call no element holds it, at M below, at and above a multiple of the
    trajectories per workgroup, with one wave per trajectory and with four, with and without lengths and finite flags"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc = LVG._scene(TIE_SCENES[31])
    for L, B in ((5, 5), (23, 9)):
        levels = LS.levels_of(L)
        per = expected_plan(31, 3, 5, L, B, sc.M)[2]
        for M in sorted({1, max(per - 1, 1), per, per + 1, sc.M}):
            for ragged, finite in ((False, None), (True, np.arange(M, dtype=np.uint8) % 2)):
                cut = _cut(sc, 0, M)
                if not ragged:
                    cut.lens = None
                rc, msg, out = _raw(torch, sm, cut, levels, B, 0.1, finite=finite)
                assert rc == 0, msg
                _assert_written(out, (L, B, M, ragged))
                assert not _untouched(out)
                if finite is not None:
                    closed = finite == 0
                    assert (out.user[closed] == -2).all() and (out.harm_at[closed] == 1.0).all() and (out.user_at[closed] == -2).all()
                    assert (out.need[closed] == L).all() and (out.user[~closed] >= -1).all() and (out.user_at[~closed] >= -1).all()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_in_their_order_leave_everything_alone(torch_cuda):
    """the ladder verdict's list in its order, then no d_speed_of, no d_harm_rows, harm_limit negative or NaN"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, _ = UG._parked()
    sc = LVG._scene((233, 2, 31, False, 2, "2", 1, 1))
    cap = sc.r2_caps[0]
    cost0, safe0 = np.full((2, 16), 0.5), np.ones(2, dtype=np.uint8)
    levels = [1.0, 4.0, 8.0]

    def call(levels=levels, B=5, cost=cost0, safe=safe0, harm_limit=0.1, **kw):
        kw.setdefault("finite", np.ones(2, dtype=np.uint8))
        kw.setdefault("a_limit", 4.0)
        return _raw(torch, sm, sc, levels, B, harm_limit, cost=cost, safe=safe, **kw)

    def refused(what, **kw):
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_harm_ladder:") and what in msg, (what, rc, msg)
        assert _untouched(out), what                                                    # nothing was launched: every byte of the pattern stands
        assert (out.cost is None or (out.cost == 0.5).all()) and (out.safe is None or (out.safe == 1).all()), what

    rc, msg, out = call()
    assert rc == N.FO_OK and (out.cost[:, 14:] != 0.5).all(), msg
    _assert_written(out, "served")
    order = [("K = 0", dict(K=0)), ("C = 9", dict(C=9)), ("h_thr", dict(h_thr=None)), ("window", dict(win_nx=0)), ("r2_cap[0]", dict(r2_caps=[-1, cap])),
             ("map_of[1] = 2", dict(map_of=(0, 2))), ("M = -1", dict(count=-1)), ("L = 0", dict(L=0)), ("h_levels [L]", dict(h_levels=None)),
             ("h_levels[1]", dict(levels=[1.0, float("nan"), 8.0])), ("strictly ascending", dict(levels=[1.0, 1.0, 8.0])), ("dt", dict(dt=0.0)),
             ("a_limit", dict(a_limit=float("nan"))), ("T = 255", dict(T=255)), ("B = 0", dict(B=0)),
             ("decreases", dict(thr=np.array([[5, 4] + [9] * 29, [9] * 31]))), ("d_x", dict(drop=("d_y",))),
             ("d_key[1]", dict(drop_map=(("d_qmin", 1),))), ("d_v", dict(drop=("d_arc",))), ("d_need", dict(drop=("d_decel",))),
             ("go together", dict(cost=None)), ("half extents", dict(hl=-0.1)), ("d_speed_of", dict(d_speed_of=None)),
             ("d_harm_rows", dict(d_harm_rows=None)), ("harm_limit", dict(harm_limit=float("nan")))]
    for what, kw in order:
        refused(what, **kw)
    for (what, kw), (_, later) in zip(order, order[1:]):            # of two faults the one earlier in the order is named
        if set(kw) & set(later) or {"levels", "L", "h_levels"} >= set(kw) | set(later):
            continue
        refused(what, **dict(kw, **later))
    refused("harm_limit", harm_limit=-0.5)
    refused("a_limit", a_limit=-0.5)
    refused("L = 65", L=65)
    refused("B = 32", B=32)
    refused("FO_HIDDEN_BRAKE_MAX_TABLE", C=8, T=113, map_of=(0,) * 8)
    refused("FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES", C=8, T=100, L=49, map_of=(0,) * 8, levels=np.linspace(0.5, 11.5, 49))
    for name in ("d_need", "d_at", "d_blocking", "d_user", "d_decel", "d_need_of", "d_first", "d_harm_at", "d_user_at"):
        refused("d_need", drop=(name,))
    refused("go together", safe=None)
    rc, msg, out = call(cost=None, safe=None, finite=None, a_limit=math.inf, harm_limit=math.inf)     # neither, no finite flags, no limits: served
    assert rc == N.FO_OK and (out.need <= 0).all(), msg
    _assert_written(out, "no limits")
    rc, msg, out = call(count=0, harm_limit=float("nan"))                               # M = 0: FO_OK, nothing launched, nothing looked at behind it
    assert rc == N.FO_OK and _untouched(out)
    ctx = N.Context(0)                                                                  # a context without a map
    assert ctx._lib.fo_scene_hidden_brake_harm_ladder(ctx._h, C.byref(N.HiddenBrakeHarmLadder()), None) == N.FO_E_STATE


def test_refusals_of_the_python_layer(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    k.sm.launch(k.sc.ego, k.sc.yaw)
    call = lambda **over: k.sm.hidden_brake_harm_ladder(*k.tr[:4], **_hl(**over))
    cost = torch.zeros((RC.M, 16), dtype=torch.float64, device=k.sm.device)
    safe = torch.ones((RC.M,), dtype=torch.uint8, device=k.sm.device)
    for bad in (dict(starts=0), dict(starts=17), dict(starts=2.0), dict(harm_limit=-1.0), dict(harm_limit=float("nan")), dict(harm_limit=None),
                dict(a_limit=-1.0), dict(a_limit=float("nan")), dict(levels=[]), dict(levels=[2.0, 1.0]), dict(levels=None, a_limit=math.inf),
                dict(kinds=STEP_KINDS[:2]), dict(kinds=(("Building", 1.0, 1.0),) * 3), dict(kinds=("Car",) * 3), dict(ego_mass=0.0),
                dict(ego_mass="heavy"), dict(coeff=dict(lr4s_const=1.0)), dict(cost=cost), dict(safe=safe), dict(cost=cost[:5], safe=safe),
                dict(users=())):
        with pytest.raises(ValueError, match="hidden_brake_harm_ladder"):
            call(**bad)
    with pytest.raises(TypeError):
        call(approach="lanes")                                                          # head-on only: there is no such keyword
    assert (cost == 0).all() and (safe == 1).all()
    hl = call(cost=cost, safe=safe, starts=None, levels=None, a_limit=8.0)              # the default ladder runs up to a_limit
    torch.cuda.synchronize()
    assert hl.starts == RC.T and hl.levels.tolist() == [0.5 * (n + 1) for n in range(16)] and torch.equal(cost[:, RH.C_RES0], hl.decel)
