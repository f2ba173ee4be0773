"""Hidden-traffic ladder verdict on the device (fo_scene_hidden_brake_ladder_verdict, PlanningStep(hidden_ladder_verdict=); DESIGN.md
§5.10 "Ladder verdict"): the tie to fo_scene_hidden_brake_ladder_users of the same library on the same device inputs through the fold
of tests/ref_hidden_brake_ladder_verdict.py at every form of the launch plan, the tie to the fail-safe verdict at one level, the fold
on cost rows a real planning step left, the step with the stage, the refusals.  Integers are exact and decel is bit-equal to
levels[need]: all comparisons are ``==``.  Every test runs under a time limit of its own that ends the process (a hung kernel cannot
be waited out from Python); no test provokes a fault."""
import faulthandler
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_ladder_scenes as LS
import hidden_brake_ladder_users_scenes as S
import hidden_brake_scenes as SC
import ref_hidden_brake_ladder_verdict as LV
import rule_refusal_cases as RC
import test_hidden_brake_ladder_users_gpu as LUG
import test_hidden_brake_users_gpu as UG
import test_hidden_brake_verdict_gpu as VG
import test_hidden_reach_gpu as T
from test_hidden_brake_ladder_verdict_cpu import expected_plan
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
SENTINEL = -7             # no int32 output ever holds it; decel is pre-filled with -7.0, which no deceleration is
STEP_LIMIT = 240          # seconds a test may take before the process is ended with every thread's traceback
RANKS_LIMIT = 200         # ... and the worker processes of the sharded test
USERS = VG.USERS          # of the step tests: two maps, three classes
VEH3 = RC.VEH[:3]
LEVELS5 = [1.0, 2.5, 4.0, 6.0, 8.0]


@pytest.fixture(autouse=True)
def _time_limit(request):
    faulthandler.dump_traceback_later(getattr(request.module, request.function.__name__ + "_limit", STEP_LIMIT), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw(torch, sm, sc, levels, B, M=None, a_limit=np.inf, keys=None, qmins=None, thr=None, map_of=None, r2_caps=None, finite=None,
         cost=None, safe=None, x=None, drop=(), drop_map=(), **over):
    """fo_scene_hidden_brake_ladder_verdict on the first ``M`` trajectories of scene ``sc`` (or on edited data of it); the output buffers
    are pre-filled with SENTINEL.  Arrays that are the same object go up once: two such maps are the same buffer.  ``cost`` / ``safe``:
    host arrays, uploaded and returned as the call left them; ``drop`` / ``drop_map`` / ``over`` as in
    tests/test_hidden_brake_ladder_users_gpu._raw (``count``: the structure's M where it is not the number of rows handed over).
    Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    sent = {}

    def up(a, dt, rows=False):
        if a is None:
            return None
        if id(a) not in sent:
            sent[id(a)] = torch.as_tensor(np.ascontiguousarray(a[:M] if rows else a, dtype=dt)).to(dev)
        return sent[id(a)]
    pick = lambda given, own: getattr(sc, own) if given is None else given
    keys, qmins, thr, map_of, r2_caps = pick(keys, "keys"), pick(qmins, "qmins"), pick(thr, "thr"), pick(map_of, "map_of"), pick(r2_caps, "r2_caps")
    M = sc.x.shape[0] if M is None else M
    Tn = sc.x.shape[1]
    thr = np.ascontiguousarray(thr, dtype=np.int32)
    levels = np.ascontiguousarray(levels, dtype=np.float64)
    Cn, Kn, Ln = thr.shape[0], len(keys), len(levels)
    tx, ty, th, tv, ta = (up(a, np.float64, True) for a in (pick(x, "x"), sc.y, sc.head, sc.v, sc.arc))
    dk, dq, tl = [up(k, np.int32) for k in keys], [up(q, np.int32, True) for q in qmins], up(sc.lens, np.int32, True)
    tf, tc, ts = up(finite, np.uint8), up(cost, np.float64), up(safe, np.uint8)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=dev)
    out = SimpleNamespace(need=full(M), at=full(M), blocking=full(M), user=full(M), need_of=full(Cn, M), first=full(Cn, M),
                          decel=torch.full((M,), float(SENTINEL), dtype=torch.float64, device=dev))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    pad = lambda vals, n, fill: (list(vals) + [fill] * n)[:n]
    ptrs = dict(d_key=pad([p(t) for t in dk], 3, None), d_qmin=pad([p(t) for t in dq], 3, None))
    for name, k in drop_map:
        ptrs[name][k] = None
    win = sc.win
    kw = dict(M=over.pop("count", M), T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=HL, hw=HW, wb=WB, win_ix0=win[0], win_iy0=win[1],
              win_nx=win[2], win_ny=win[3], K=Kn, C=Cn, d_key=(C.c_void_p * 3)(*ptrs["d_key"]), d_qmin=(C.c_void_p * 3)(*ptrs["d_qmin"]),
              r2_cap=(C.c_int32 * 3)(*pad([int(r) for r in r2_caps], 3, -5)), map_of=(C.c_int32 * 8)(*pad([int(k) for k in map_of], 8, 99)),
              d_v=p(tv), d_arc=p(ta), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), L=Ln, B=int(B), dt=float(sc.dt),
              h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), a_limit=float(a_limit), d_finite_or_null=p(tf), d_cost_or_null=p(tc),
              d_safe_or_null=p(ts), d_need=p(out.need), d_at=p(out.at), d_blocking=p(out.blocking), d_user=p(out.user), d_decel=p(out.decel),
              d_need_of=p(out.need_of), d_first=p(out.first))
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeLadderVerdict(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_ladder_verdict(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    res = SimpleNamespace(**{k: _np(getattr(out, k)) for k in LV.OUTPUTS})
    res.cost, res.safe = (None if tc is None else _np(tc)), (None if ts is None else _np(ts))
    return rc, msg, res


def _untouched(out):
    return all((getattr(out, k) == SENTINEL).all() for k in LV.OUTPUTS)


def _same(out, want, what):
    """every output is the checker's fold of the ladder-users entry's, element by element -- and so every byte was written"""
    for name in LV.OUTPUTS:
        got, w = getattr(out, name), want[name]
        assert got.dtype == w.dtype and got.shape == w.shape, (what, name, got.shape, w.shape)
        assert not (w == SENTINEL).any()
        assert got.tobytes() == w.tobytes(), (what, name, np.argwhere(got != w)[:4].tolist())


def _users_side(torch, sm, sc, levels, B, **edited):
    """fo_scene_hidden_brake_ladder_users on the whole scene at this ladder and these starts: what the verdict is defined on"""
    rc, msg, lu = LUG._raw(torch, sm, sc, detail=False, levels=np.asarray(levels, dtype=np.float64), B=B, **edited)
    assert rc == 0, msg
    return lu


def _tie(torch, sm, sc, lu, levels, B, M, what, **edited):
    """the verdict on the first M trajectories against the checker's fold of ``lu`` cut to them"""
    rc, msg, out = _raw(torch, sm, sc, levels, B, M=M, **edited)
    assert rc == 0, (what, msg)
    lens = None if sc.lens is None else sc.lens[:M]
    want = LV.verdict(lu.required_all[:M], lu.blocking[:M], lu.required[:, :M], lu.first[:, :M], list(levels), B, sc.T, lens)
    _same(out, want, what)
    assert np.array_equal(out.decel, np.where(out.need < 0, 0.0, np.append(levels, np.inf)[np.clip(out.need, 0, len(levels))])), what
    return out


_scenes = {}


def _scene(spec):
    if spec not in _scenes:
        _scenes[spec] = S.scene(*spec)
    return _scenes[spec]


# ------------------------------------------------------------------------------------------------ 1. the tie
# (seed, M, T, ragged, C, layout, L, B) of tests/hidden_brake_ladder_users_scenes.scene: M is at least the largest per_block + 1 of the
# plan at that T (256 at T = 1, 2; 78 at T = 7; 17 at T = 31) and at least 65; the lengths begin with 0, 1, 2
TIE_SCENES = {1: (201, 260, 1, True, 5, "3", 1, 1), 2: (202, 260, 2, True, 5, "3", 1, 1), 7: (207, 80, 7, True, 5, "3", 1, 1),
              31: (231, 70, 31, True, 5, "3", 1, 1)}
LADDERS = (1, 2, 3, 5, 23, 33, 64)


@pytest.mark.parametrize("T_", sorted(TIE_SCENES))
def test_tie_to_the_ladder_users_entry_at_every_form_of_the_plan(torch_cuda, T_):
    """T in {1, 2, 7, 31} x L in {1, 2, 3, 5, 23, 33, 64} x B in {1, 2, 3, 5, T} x M in {1, per_block, per_block + 1, 65}: need, at, blocking,
    user, decel, need_of and first are the checker's fold of what fo_scene_hidden_brake_ladder_users writes on the same device inputs,
    bit for bit -- G from 1 to 256, one round and several, workgroups capped by the lanes and by the rows, the last one part full; five
    users on three maps; ragged lengths that begin with 0, 1, 2 and hold negative ones, ones beyond T and ones below B"""
    torch = torch_cuda
    sm, road = UG._parked()
    sc = _scene(TIE_SCENES[T_])
    assert np.array_equal(road, sc.road) and len(sc.keys) == 3 and sc.lens[:3].tolist() == [0, 1, 2]
    groups, rounds, needs, capped = set(), set(), set(), set()
    for L in LADDERS:
        levels = LS.levels_of(L)
        for B in sorted({b for b in (1, 2, 3, 5, T_) if b <= T_}):
            Lp, G, per, _, _ = expected_plan(T_, 3, 5, L, B, sc.M)
            lu = _users_side(torch, sm, sc, levels, B)
            for M in sorted({1, per, per + 1, 65}):
                assert M <= sc.M
                out = _tie(torch, sm, sc, lu, levels, B, M, (T_, L, B, M))
                needs |= {("L" if n == L else n if n <= 0 else "mid") for n in out.need.tolist()}
                assert ((out.at == -1) == (out.need == -1)).all() and (out.at < B).all() and (out.need_of <= out.need[None]).all()
            assert out.need[0] == -1 and out.decel[0] == 0.0 and (out.need_of[:, 0] == -1).all() and (out.first[:, 0] == -1).all()   # length 0
            groups.add(G)
            rounds.add(-(-(B * Lp) // G))
            capped.add(per < 256 // G)
    assert groups == {1: {1, 2, 4, 8, 32, 64}, 2: {1, 2, 4, 8, 16, 32, 64, 128}}.get(T_, {1, 2, 4, 8, 16, 32, 64, 128, 256})
    assert rounds >= ({1} if T_ <= 2 else {1, 2}) and (T_ < 31 or {1, 2, 4, 8} <= rounds) and (T_ < 7 or capped == {False, True})
    assert -1 in needs and (T_ == 1 or {0, "L"} & needs)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C_", [1, 3, 4, 5, 8])
def test_tie_over_class_and_map_counts(torch_cuda, C_, K):
    """C in {1, 3, 4, 5, 8} x K in {1, 2, 3}: all six instantiations, widths with classes that are not there, class c on map (c + 1) % K so
    that classes share a map -- and, with K >= 2, two maps that are the very same BUFFER"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc = _scene((232, 20, 31, True, 8, "3", 1, 1))
    edited = dict(keys=sc.keys[:K], qmins=sc.qmins[:K], map_of=[(c + 1) % K for c in range(C_)], r2_caps=sc.r2_caps[:K])
    seen = set()
    for L, B in ((23, 5), (2, 31), (1, 1), (5, 3)):
        levels = LS.levels_of(L)
        lu = _users_side(torch, sm, sc, levels, B, table=sc.thr[:C_], **edited)
        out = _tie(torch, sm, sc, lu, levels, B, sc.M, (C_, K, L, B), thr=sc.thr[:C_], **edited)
        seen |= set(out.user.tolist())
        assert (out.blocking < (1 << C_)).all()
    assert -1 in seen and (C_ == 1 or len(seen) >= 2)
    if K >= 2:
        same = dict(edited, keys=[sc.keys[0]] * K, qmins=[sc.qmins[0]] * K)
        lu = _users_side(torch, sm, sc, LS.levels_of(5), 5, table=sc.thr[:C_], **same)
        _tie(torch, sm, sc, lu, LS.levels_of(5), 5, sc.M, (C_, K, "one buffer"), thr=sc.thr[:C_], **same)


def test_the_level_clear_of_every_user_lies_above_every_users_own(torch_cuda):
    """tests/hidden_brake_ladder_users_scenes.hand_scene: candidate 0 from brake start 0 needs level 2 of 0 / 3 / 8 m/s^2 though user 0
    alone needs 0 and user 1 alone 1, blocked below by user 0: need is no maximum over need_of"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc = S.hand_scene()
    for B in (1, 5, sc.T):
        lu = _users_side(torch, sm, sc, sc.levels, B)
        out = _tie(torch, sm, sc, lu, sc.levels, B, sc.M, ("hand", B))
        if B == 1:
            assert (out.need[0], out.at[0], out.blocking[0], out.user[0], out.decel[0]) == (2, 0, 0b01, 0, 8.0)
            assert out.need_of[:, 0].tolist() == [0, 1]
        assert out.need[0] >= 2 > out.need_of[:, 0].max() or B > 1


# ------------------------------------------------------------------------------------------------ 2. one level: the fail-safe verdict
def test_one_level_is_the_fail_safe_verdict(torch_cuda):
    """L = 1: need <= 0 iff fo_scene_hidden_brake_verdict at a_brake = levels[0] finds every one of the B starts fail-safe, on the same
    inputs; and need_of[c] <= 0 iff that entry's commit[c] is -1"""
    torch = torch_cuda
    sm, _ = UG._parked()
    both = set()
    for T_ in (7, 31):
        sc = _scene(TIE_SCENES[T_])
        for a_brake, B in ((8.0, 1), (8.0, 5), (2.0, T_), (0.0, 3)):
            rc, msg, fs = VG._raw_verdict(torch, sm, sc.win, sc.r2_caps, sc.keys, sc.qmins, sc.x, sc.y, sc.head, sc.v, sc.arc, a_brake, sc.dt, sc.thr,
                                          sc.map_of, B, lens=sc.lens)
            assert rc == 0, msg
            rc, msg, out = _raw(torch, sm, sc, [a_brake], B)
            assert rc == 0, msg
            assert np.array_equal(out.need <= 0, fs.fail_safe == B), (T_, a_brake, B)
            assert np.array_equal(out.need_of <= 0, fs.commit == -1) and np.array_equal(out.first, fs.first), (T_, a_brake, B)
            assert np.array_equal(out.at[out.need == 1], fs.fail_safe[out.need == 1]), (T_, a_brake, B)      # the first start that is not
            both |= set((out.need <= 0).tolist())
    assert both == {False, True}


# ------------------------------------------------------------------------------------------------ 3. the fold on the device
def _lv(**over):
    kw = dict(vehicle=VEH3, users=USERS, dt=0.1, levels=LEVELS5, starts=5, a_limit=4.0)
    kw.update(over)
    return kw


def _step_then_stage(torch, k, tr=None, **over):
    """a plain PlanningStep.run, its cost / safe copied, then the stage by its own call (on ``tr`` where given: the step itself always
    sees the stack's own candidates): (before, after, verdict)"""
    from frenetix_occlusion.step import PlanningStep
    tr = k.tr if tr is None else tr
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced")
    out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    before = (out.cost.clone(), out.safe.clone())
    lv = k.sm.hidden_brake_ladder_verdict(*tr[:4], cost=out.cost, safe=out.safe, **_lv(**over))
    torch.cuda.synchronize()
    return (_np(before[0]), _np(before[1])), (_np(out.cost), _np(out.safe)), lv


def _assert_fold(before, after, lv, a_limit):
    cost0, safe0 = before
    cost1, safe1 = after
    need, user, decel = _np(lv.need), _np(lv.user), _np(lv.decel)
    want_cost, want_safe = LV.fold(cost0, safe0, need, user, decel, len(lv.levels), a_limit)
    assert cost1.tobytes() == want_cost.tobytes() and np.array_equal(safe1, want_safe)
    others = [c for c in range(16) if c not in (LV.C_SAFE, LV.C_RES0, LV.C_RES1)]
    assert cost1[:, others].tobytes() == cost0[:, others].tobytes()             # bit-identical, NaNs included
    assert (safe1 <= safe0).all()                                               # only ever 1 -> 0
    assert cost1[:, LV.C_RES0].tobytes() == decel.tobytes() and np.array_equal(cost1[:, LV.C_RES1], user.astype(np.float64))
    assert np.array_equal(decel, np.where(need < 0, 0.0, np.append(lv.levels, np.inf)[np.clip(need, 0, len(lv.levels))]))


def _device_tie(torch, k, lv, lengths=None):
    """the ladder-users entry on the very device data the stage walked on, folded by the checker"""
    w = k.sm.window
    x, y, v = (_np(t) for t in (k.tr[0], k.tr[1], k.tr[3]))
    sc = SimpleNamespace(x=x, y=y, head=_np(lv.poses.heading), v=v, arc=_np(lv.poses.arc), lens=lengths, win=(w.ix0, w.iy0, w.nx, w.ny), dt=0.1,
                         keys=[_np(c.key) for c in lv.clearances], qmins=[_np(c.qmin) for c in lv.clearances], thr=lv.thr, map_of=lv.map_of,
                         r2_caps=[c.r2_cap for c in lv.clearances], levels=lv.levels, starts=lv.starts, T=RC.T)
    rc, msg, lu = LUG._raw(torch, k.sm, sc, detail=False)
    assert rc == 0, msg
    want = LV.verdict(lu.required_all, lu.blocking, lu.required, lu.first, list(lv.levels), lv.starts, RC.T, lengths, _np(lv.poses.finite))
    _same(SimpleNamespace(**{n: _np(getattr(lv, n)) for n in LV.OUTPUTS}), want, "the Python layer")


def test_fold_on_the_rows_of_a_real_step(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    before, after, lv = _step_then_stage(torch, k)
    assert before[1].any() and not before[1].all() and not np.isnan(before[0][:, :12]).all()          # clean rows and already unsafe ones
    _assert_fold(before, after, lv, 4.0)
    _device_tie(torch, k, lv)
    assert lv.starts == 5 and lv.a_limit == 4.0 and lv.map_of == (0, 1, 0) and lv.levels.tolist() == LEVELS5
    assert torch.equal(lv.critical_user(), lv.user.to(torch.int64)) and lv.required_deceleration() is lv.decel
    assert torch.equal(lv.brake_threat_number(8.0), lv.decel / 8.0)
    decel = _np(lv.decel)
    assert (after[1] < before[1]).any() and ((decel > 0) & (decel <= 4.0)).any()         # a flag was lowered; a graded answer was kept
    # a_limit = +inf takes safety only where no level suffices
    before, after, lv2 = _step_then_stage(torch, k, a_limit=float("inf"))
    _assert_fold(before, after, lv2, np.inf)
    assert np.array_equal(after[1], np.where(_np(lv2.need) == 5, 0, before[1]))
    for name in LV.OUTPUTS:
        assert torch.equal(getattr(lv2, name), getattr(lv, name)), name


def test_a_refused_step_stays_unsafe_and_gets_the_two_columns(torch_cuda):
    torch = torch_cuda
    import test_rule_refusal_gpu as RG
    k = VG._stack(torch, RG.REFUSING_CELL)
    before, after, lv = _step_then_stage(torch, k)
    RG.assert_refused(SimpleNamespace(cost=torch.as_tensor(before[0]), safe=torch.as_tensor(before[1])))
    _assert_fold(before, after, lv, 4.0)
    assert not after[1].any() and (after[0][:, LV.C_SAFE] == 0.0).all()
    others = [c for c in range(14) if c != LV.C_SAFE]
    assert np.isnan(after[0][:, others]).all() and after[0][:, LV.C_RES0].tobytes() == _np(lv.decel).tobytes()
    assert (after[0][:, LV.C_RES0] > 0).any()


def test_every_byte_is_written_and_a_non_finite_candidate_fails_closed(torch_cuda):
    """a NaN, an inf and a -inf in x, theta and v of candidates as the stage sees them, below their length: need = L, at = 0, blocking = 0,
    user = -2, decel = inf and the flag is lost; the same at or beyond the length does not count (the sweep's rows are those of the
    clean candidates: what a sweep makes of such a pose is not this stage's claim).  The raw entry fills buffers that held a sentinel"""
    torch = torch_cuda
    k = VG._stack(torch)
    lengths = np.full(RC.M, RC.T, dtype=np.int32)
    lengths[[3, 11, 40, 50, 51, 52]] = [9, 1, 16, 7, 0, 15]
    tr = [t.clone() for t in k.tr]
    tr[0][3, 7], tr[2][11, 0], tr[3][40, 15] = float("nan"), float("inf"), float("-inf")            # below the length
    tr[0][50, 7], tr[2][51, 0], tr[3][52, 15] = float("nan"), float("inf"), float("-inf")           # at the length
    before, after, lv = _step_then_stage(torch, k, tr=tr, lengths=lengths)
    need, at, blocking, user, decel = (_np(getattr(lv, n)) for n in ("need", "at", "blocking", "user", "decel"))
    for m in (3, 11, 40):
        assert (need[m], at[m], blocking[m], user[m], decel[m], after[1][m], after[0][m, LV.C_SAFE], after[0][m, LV.C_RES1]) == (5, 0, 0, -2, np.inf, 0, 0.0, -2.0), m
        assert after[0][m, LV.C_RES0] == np.inf
    fin = _np(lv.poses.finite)
    assert fin.sum() == RC.M - 3 and fin[[50, 51, 52]].all() and (user[[m for m in range(RC.M) if m not in (3, 11, 40)]] >= -1).all()
    assert need[51] == -1 and decel[51] == 0.0 and after[1][51] == before[1][51]                    # length 0: nothing asked, nothing taken
    _assert_fold(before, after, lv, 4.0)
    # the raw entry on a scene: every output byte replaced the sentinel, whatever M leaves of the last workgroup
    sm, _ = UG._parked()
    sc = _scene(TIE_SCENES[31])
    for M in (1, 18, 70):
        rc, msg, out = _raw(torch, sm, sc, LEVELS5, 5, M=M, finite=np.arange(M) % 3 != 1)
        assert rc == 0, msg
        assert all(not (getattr(out, n) == SENTINEL).any() for n in LV.OUTPUTS), M
        closed = np.arange(M) % 3 == 1
        assert (out.need[closed] == 5).all() and (out.user[closed] == -2).all() and np.isinf(out.decel[closed]).all() and (out.user[~closed] >= -1).all()


# ------------------------------------------------------------------------------------------------ 4. the planning step
def test_step_with_the_stage_is_the_stage_by_stage_calls(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion.step import PlanningStep
    k = VG._stack(torch)
    _, staged, lv = _step_then_stage(torch, k)
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_ladder_verdict=_lv())
    for _ in range(2):                                              # (a second run folds into fresh rows, not into folded ones)
        out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
        torch.cuda.synchronize()
        assert _np(out.cost).tobytes() == staged[0].tobytes() and np.array_equal(_np(out.safe), staged[1])
        assert out.hidden_verdict is None
        for name in LV.OUTPUTS:
            assert torch.equal(getattr(out.hidden_ladder_verdict, name), getattr(lv, name)), name
    assert (staged[1] == 0).any() and (_np(lv.need) > 0).any()
    with pytest.raises(ValueError, match="hidden_ladder_verdict"):
        PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_ladder_verdict=dict(users=USERS))
    with pytest.raises(ValueError, match="same two reserved cost columns"):
        PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_ladder_verdict=_lv(), hidden_verdict=VG._hv())
    plain = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced").run(k.sc.ego, k.sc.yaw, k.sc.v)
    assert plain.hidden_ladder_verdict is None and plain.hidden_verdict is None


def _run_ranks(tmp_path, world, backend):
    """tests/hidden_ladder_verdict_dist_worker.py as ``world`` processes, started as tests/test_distributed_gpu._run_ranks starts its worker"""
    import test_distributed_gpu as DG
    port = DG._free_port()
    out = str(tmp_path / f"ladder_verdict_{backend}_{world}.npz")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(T.ROOT, "tests", "hidden_ladder_verdict_dist_worker.py"), "--backend", backend,
                                       "--out", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=RANKS_LIMIT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    return np.load(out)


test_two_ranks_shard_the_step_with_the_stage_limit = RANKS_LIMIT + 60


def test_two_ranks_shard_the_step_with_the_stage(torch_cuda, tmp_path):
    """two ranks on one GPU, the collective over gloo: rank 1 holds rows 65 .. 129, its stage runs on those rows and on its cut of the
    ragged lengths and is queued BEFORE the all-gather -- rows [lo, hi) of every rank in cost_all are the unsharded step + stage, bit
    for bit"""
    z = _run_ranks(tmp_path, 2, "gloo")
    M = RC.M
    assert int(z["world"]) == 2 and [tuple(r) for r in z["rows"]] == [(0, 65), (65, 130)]
    assert z["cost_all"].shape == (M, 16) and z["cost_all"].tobytes() == z["ref_cost"].tobytes()
    assert z["local_cost"].tobytes() == z["ref_cost"].tobytes() and np.array_equal(z["local_safe"], z["ref_safe"])
    for name in LV.OUTPUTS:
        assert z["local_" + name].tobytes() == z["ref_" + name].tobytes(), name
    want_cost, want_safe = LV.fold(z["plain_cost"], (z["plain_cost"][:, LV.C_SAFE] > 0.5).astype(np.uint8), z["ref_need"], z["ref_user"],
                                   z["ref_decel"], len(LEVELS5), 4.0)
    assert want_cost.tobytes() == z["ref_cost"].tobytes() and np.array_equal(want_safe, z["ref_safe"])
    assert (z["plain_cost"][:, 14:16] == 0.0).all()
    for lo, hi in z["rows"]:                                        # the stage did something on either side of the boundary
        assert (z["ref_need"][lo:hi] > 0).any() and (z["ref_need"][lo:hi] <= 0).any()
        assert (z["plain_cost"][lo:hi, LV.C_SAFE] > z["ref_cost"][lo:hi, LV.C_SAFE]).any()
        assert z["cost_all"][lo:hi, LV.C_RES0].tobytes() == z["ref_decel"][lo:hi].tobytes()
    ends = np.clip(z["lengths"], 0, RC.T)
    assert (ends == 0).any() and (z["ref_need"][ends == 0] == -1).all() and ((ends > 0) & (ends < 5)).any()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_in_their_order_leave_everything_alone(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, _ = UG._parked()
    sc = _scene((233, 2, 31, False, 2, "2", 1, 1))
    cap = sc.r2_caps[0]
    cost0, safe0 = np.full((2, 16), 0.5), np.ones(2, dtype=np.uint8)
    levels = [1.0, 4.0, 8.0]

    def call(levels=levels, B=5, cost=cost0, safe=safe0, **kw):
        kw.setdefault("finite", np.ones(2, dtype=np.uint8))
        kw.setdefault("a_limit", 4.0)
        return _raw(torch, sm, sc, levels, B, cost=cost, safe=safe, **kw)

    def refused(what, **kw):
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_ladder_verdict:") and what in msg, (what, rc, msg)
        assert _untouched(out), what                                                    # nothing was launched: every canary stands
        assert (out.cost is None or (out.cost == 0.5).all()) and (out.safe is None or (out.safe == 1).all()), what

    rc, msg, out = call()
    assert rc == N.FO_OK and not (out.need == SENTINEL).any() and (out.cost[:, 14:] != 0.5).all(), msg
    # each refusal, in the header's order
    order = [("K = 0", dict(K=0)), ("C = 9", dict(C=9)), ("h_thr", dict(h_thr=None)), ("window", dict(win_nx=0)), ("r2_cap[0]", dict(r2_caps=[-1, cap])),
             ("map_of[1] = 2", dict(map_of=(0, 2))), ("M = -1", dict(count=-1)), ("L = 0", dict(L=0)), ("h_levels [L]", dict(h_levels=None)),
             ("h_levels[1]", dict(levels=[1.0, float("nan"), 8.0])), ("strictly ascending", dict(levels=[1.0, 1.0, 8.0])), ("dt", dict(dt=0.0)),
             ("a_limit", dict(a_limit=float("nan"))), ("T = 255", dict(T=255)), ("B = 0", dict(B=0)),
             ("decreases", dict(thr=np.array([[5, 4] + [9] * 29, [9] * 31]))), ("d_x", dict(drop=("d_y",))),
             ("d_key[1]", dict(drop_map=(("d_qmin", 1),))), ("d_v", dict(drop=("d_arc",))), ("d_need", dict(drop=("d_decel",))),
             ("go together", dict(cost=None)), ("half extents", dict(hl=-0.1))]
    for what, kw in order:
        refused(what, **kw)
    for (what, kw), (_, later) in zip(order, order[1:]):            # of two faults the one earlier in the order is named
        if set(kw) & set(later) or {"levels", "L", "h_levels"} >= set(kw) | set(later):
            continue
        refused(what, **dict(kw, **later))
    # the rest of the list
    refused("K = 4", K=4)
    refused("C = 0", C=0)
    refused("L = 65", L=65)
    refused("h_levels[0]", levels=[-1.0, 4.0, 8.0])
    refused("h_levels[2]", levels=[1.0, 4.0, float("inf")])
    refused("strictly ascending", levels=[1.0, 8.0, 4.0])
    refused("a_limit", a_limit=-0.5)
    refused("B = 32", B=32)
    refused("negative", thr=np.array([[-1] * 31, [9] * 31]))
    refused("lies beyond", thr=sc.thr + 169 * (cap + 1))
    refused("FO_HIDDEN_BRAKE_MAX_TABLE", C=8, T=113, map_of=(0,) * 8)
    refused("FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES", C=8, T=100, L=49, map_of=(0,) * 8, levels=np.linspace(0.5, 11.5, 49))
    for name in ("d_x", "d_y", "d_heading"):
        refused("d_x", drop=(name,))
    refused("d_key[0]", drop_map=(("d_key", 0),))
    for name in ("d_need", "d_at", "d_blocking", "d_user", "d_decel", "d_need_of", "d_first"):
        refused("d_need", drop=(name,))
    refused("go together", safe=None)
    rc, msg, out = call(cost=None, safe=None, finite=None, a_limit=float("inf"))        # neither, no finite flags, no limit: served
    assert rc == N.FO_OK and not (out.need == SENTINEL).any(), msg
    rc, msg, out = call(a_limit=0.0)                                                    # 0 is a limit
    assert rc == N.FO_OK and np.array_equal(out.safe, (out.decel <= 0.0).astype(np.uint8)), msg
    rc, msg, out = call(count=0)                                                            # M = 0: FO_OK, nothing launched
    assert rc == N.FO_OK and _untouched(out)
    ctx = N.Context(0)                                                                  # a context without a map
    assert ctx._lib.fo_scene_hidden_brake_ladder_verdict(ctx._h, C.byref(N.HiddenBrakeLadderVerdict()), None) == N.FO_E_STATE


def test_refusals_of_the_python_layer(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    k.sm.launch(k.sc.ego, k.sc.yaw)
    call = lambda **over: k.sm.hidden_brake_ladder_verdict(*k.tr[:4], **_lv(**over))
    cost = torch.zeros((RC.M, 16), dtype=torch.float64, device=k.sm.device)
    safe = torch.ones((RC.M,), dtype=torch.uint8, device=k.sm.device)
    for bad in (dict(starts=0), dict(starts=17), dict(starts=2.0), dict(a_limit=-1.0), dict(a_limit=float("nan")), dict(a_limit="much"),
                dict(levels=[]), dict(levels=[2.0, 1.0]), dict(levels=[1.0, 1.0]), dict(levels=[float("inf")]), dict(levels=None, a_limit=float("inf")),
                dict(cost=cost), dict(safe=safe), dict(cost=cost[:5], safe=safe), dict(cost=cost.float(), safe=safe),
                dict(cost=cost, safe=safe.int()), dict(cost=cost.cpu(), safe=safe.cpu()), dict(users=())):
        with pytest.raises(ValueError, match="hidden_brake_ladder_verdict"):
            call(**bad)
    assert (cost == 0).all() and (safe == 1).all()
    lv = call(cost=cost, safe=safe, starts=None, levels=None, a_limit=3.0)
    torch.cuda.synchronize()
    assert lv.starts == RC.T and lv.levels.tolist() == [0.5, 1.0, 1.5, 2.0, 2.5, 3.0] and torch.equal(cost[:, LV.C_RES0], lv.decel)
