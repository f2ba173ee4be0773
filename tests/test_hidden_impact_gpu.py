"""Hidden-traffic impact verdict on the device (fo_scene_hidden_brake_impact, SensorModel.hidden_brake_impact,
PlanningStep(hidden_impact_verdict=); DESIGN.md §5.10 "Impact verdict"): the tie to fo_scene_hidden_brake_verdict and
fo_scene_hidden_brake_users of the same library on the same device inputs and to the plain statement tests/ref_hidden_impact.py, a
hand case with numbers written out, the fold on cost rows a real planning step left, the step with and without the stage, the
pre-filled outputs, the refusals.  Integers and speeds are compared with ``==`` (a speed is one subtraction, two multiplications and
an fmax without contraction, which float64 on the host reproduces bit for bit), harms to 1e-9, the chosen user exactly -- the scenes
hold no open choice (tests/test_hidden_impact_cpu.py).  Every test runs under a time limit of its own that ends the process (a hung
kernel cannot be waited out from Python); no test provokes a fault."""
import faulthandler
import math
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_scenes as SC
import hidden_brake_users_scenes as US
import hidden_impact_cases as IC
import ref_hidden_impact as RI
import rule_refusal_cases as RC
import test_hidden_brake_users_gpu as UG
import test_hidden_brake_verdict_gpu as VG
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
INT_OUTPUTS, F64_OUTPUTS = ("user", "at", "commit", "first"), ("harm", "speed")
OUTPUTS = F64_OUTPUTS + INT_OUTPUTS
STEP_LIMIT = 240          # seconds a test may take before the process is ended with every thread's traceback
TOL = 1e-9                # the project's stated float tolerance (README, "GPU vs oracle")
PATTERN = 0xA5            # the byte every output buffer is filled with before a call
PAT_I32 = int(np.frombuffer(bytes([PATTERN] * 4), dtype=np.int32)[0])
PAT_F64 = float(np.frombuffer(bytes([PATTERN] * 8), dtype=np.float64)[0])
STEP_KINDS = (("Pedestrian", 0.36, 0.65), ("Bicycle", 2.8, 2.25), ("Car", 5.76, 2.6))     # of VG.USERS: 1.5, 4.0 and 6.0 m/s


@pytest.fixture(autouse=True)
def _time_limit(request):
    faulthandler.dump_traceback_later(getattr(request.module, request.function.__name__ + "_limit", STEP_LIMIT), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw_impact(torch, sm, win, r2_caps, keys, qmins, x, y, head, v, arc, a_brake, dt, thr, map_of, B, rows, speed_of, harm_limit=math.inf,
                lens=None, finite=None, cost=None, safe=None, alias=(), hl=HL, hw=HW, wb=WB, drop=(), drop_map=(), **over):
    """fo_scene_hidden_brake_impact on maps and trajectories of the test's own; every byte of the output buffers is pre-filled with
    PATTERN.  The arguments as tests/test_hidden_brake_verdict_gpu._raw_verdict's.  Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    M, Tn = x.shape
    thr = np.ascontiguousarray(thr, dtype=np.int32)
    Cn, Kn = thr.shape[0], len(keys)
    tx, ty, th, tv, ta = (up(a, np.float64) for a in (x, y, head, v, arc))
    dk, dq, tl, tf = [up(k, np.int32) for k in keys], [up(q, np.int32) for q in qmins], up(lens, np.int32), up(finite, np.uint8)
    if alias:
        dk[alias[0]] = dk[alias[1]]
    tc, ts = up(cost, np.float64), up(safe, np.uint8)
    trow, tsp = up(np.asarray(rows, dtype=np.float64).reshape(Cn, 4), np.float64), up(np.asarray(speed_of, dtype=np.float64), np.float64)

    def filled(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(PATTERN)
        return t
    out = SimpleNamespace(harm=filled((M, 2), torch.float64), user=filled((M,), torch.int32), speed=filled((Cn, M), torch.float64),
                          at=filled((Cn, M), torch.int32), commit=filled((Cn, M), torch.int32), first=filled((Cn, M), torch.int32))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    pad = lambda vals, n, fill: (list(vals) + [fill] * n)[:n]
    ptrs = dict(d_key=pad([p(t) for t in dk], 3, None), d_qmin=pad([p(t) for t in dq], 3, None))
    for name, k in drop_map:
        ptrs[name][k] = None
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=hl, hw=hw, wb=wb, win_ix0=win[0], win_iy0=win[1],
              win_nx=win[2], win_ny=win[3], K=Kn, C=Cn, d_key=(C.c_void_p * 3)(*ptrs["d_key"]), d_qmin=(C.c_void_p * 3)(*ptrs["d_qmin"]),
              r2_cap=(C.c_int32 * 3)(*pad([int(r) for r in r2_caps], 3, -5)), map_of=(C.c_int32 * 8)(*pad([int(k) for k in map_of], 8, 99)),
              d_v=p(tv), d_arc=p(ta), a_brake=float(a_brake), dt=float(dt), h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), B=int(B),
              d_speed_of=p(tsp), d_harm_rows=p(trow), harm_limit=float(harm_limit), d_finite_or_null=p(tf), d_cost_or_null=p(tc),
              d_safe_or_null=p(ts), d_harm=p(out.harm), d_user=p(out.user), d_speed=p(out.speed), d_at=p(out.at), d_commit=p(out.commit),
              d_first=p(out.first))
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeImpact(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_impact(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    res = SimpleNamespace(**{k: _np(getattr(out, k)) for k in OUTPUTS})
    res.cost, res.safe = (None if tc is None else _np(tc)), (None if ts is None else _np(ts))
    return rc, msg, res


def _untouched(out):
    """every output still holds the pattern in every byte"""
    return all((getattr(out, k).view(np.uint8) == PATTERN).all() for k in OUTPUTS)


def _assert_written(out, what):
    """no element of any output still holds the pattern (no result is the pattern's number: an int32 below -10^9, a float64 of
    magnitude 10^-127)"""
    for k in INT_OUTPUTS:
        assert (getattr(out, k) != PAT_I32).all(), (what, k)
    for k in F64_OUTPUTS:
        assert (getattr(out, k) != PAT_F64).all(), (what, k)


def _assert_impact(out, users, v, a_brake, dt, B, rows, speed_of, lens, what, finite=None):
    """the outputs against the checker run on the users entry's brake_first / stop / first"""
    harm, user, speed, at, n_open = RI.impact(users.brake_first, users.stop, users.first, v, a_brake, dt, B, rows, speed_of, lens, finite)
    assert n_open == 0, what
    assert out.speed.dtype == np.float64 and out.harm.dtype == np.float64 and out.at.dtype == np.int32 and out.user.dtype == np.int32
    assert np.array_equal(out.at, at), (what, "at", np.argwhere(out.at != at)[:4].tolist())
    assert out.speed.tobytes() == speed.tobytes(), (what, "speed", np.argwhere(out.speed != speed)[:4].tolist())
    worst = float(np.abs(out.harm - harm).max()) if harm.size else 0.0
    assert out.harm.shape == harm.shape and worst <= TOL, (what, "harm", worst)
    assert np.array_equal(out.user, user), (what, "user", np.argwhere(out.user != user)[:4].tolist())
    return worst


def _tie(torch, sm, sc, M, B, keys, qmins, thr, map_of, r2_caps, rows, speed_of, what, alias=(), last=False):
    """the impact entry on the first M trajectories of the scene (``last``: its last M) against the verdict entry and the users entry
    on the same device inputs and the checker's steps 1 - 6"""
    cut = lambda a: None if a is None else (a[len(a) - M:] if last else a[:M])
    x, y, head, v, arc, lens = (cut(a) for a in (sc.x, sc.y, sc.head, sc.v, sc.arc, sc.lens))
    qm = [cut(q) for q in qmins]
    rc, msg, users = UG._raw_users(torch, sm, sc.win, r2_caps, keys, qm, x, y, head, v, arc, sc.a_brake, sc.dt, thr, map_of, lens)
    assert rc == 0, msg
    rc, msg, verdict = VG._raw_verdict(torch, sm, sc.win, r2_caps, keys, qm, x, y, head, v, arc, sc.a_brake, sc.dt, thr, map_of, B, lens=lens,
                                       alias=alias)
    assert rc == 0, (what, msg)
    rc, msg, out = _raw_impact(torch, sm, sc.win, r2_caps, keys, qm, x, y, head, v, arc, sc.a_brake, sc.dt, thr, map_of, B, rows, speed_of,
                               lens=lens, alias=alias)
    assert rc == 0, (what, msg)
    _assert_written(out, what)
    for name in ("commit", "first"):
        got, want = getattr(out, name), getattr(verdict, name)
        assert got.dtype == np.int32 and np.array_equal(got, want), (what, name, np.argwhere(got != want)[:4].tolist())
    out.worst = _assert_impact(out, users, v, sc.a_brake, sc.dt, B, rows, speed_of, lens, what)
    assert ((out.at >= 0) == (out.commit >= 0)).all(), what            # a class has a hit start iff it has a commit
    assert ((out.user == -1) == (out.at < 0).all(axis=0)).all() and (out.at < B).all(), what
    return out


# ------------------------------------------------------------------------------------------------ 1. the tie
@pytest.mark.parametrize("T_", sorted(VG.TIE_SCENES))
def test_tie_to_the_verdict_and_users_entries_at_every_group_size(torch_cuda, T_):
    """T in {1, 2, 31, 64, 65, 254} x B in {1, 2, 5, T} (and 3, 12 at T = 31): commit and first are fo_scene_hidden_brake_verdict's, speed
    and at the checker's on fo_scene_hidden_brake_users' brake_first / stop / first, bit for bit; harm to 1e-9, user exactly; with M at
    per_block - 1, per_block, per_block + 1 of every (T, B), on three maps (five users; three at T = 254), on the scene's FIRST M
    trajectories (lengths 0, 1, 2 lead them) and on its LAST M (the seed's ragged lengths)"""
    torch = torch_cuda
    sm, _ = UG._parked()
    users = UG.THREE if T_ == 254 else US.USERS
    sc = VG._scene(VG.TIE_SCENES[T_], users)
    rows, speed_of = IC.rows_of(IC.kinds_of(users, IC.KINDS5, US.USERS)), [u[0] for u in users]
    assert len(sc.keys) == 3 and sc.lens[:3].tolist() == [0, 1, 2]
    seen, worst, hits = set(), 0.0, 0
    for B in VG._starts(T_):
        per = VG._per_block(T_, 3, B)
        for M in sorted({m for m in (per - 1, per, per + 1) if m >= 1}):
            assert M + 3 <= sc.M
            for last in (False, True):
                out = _tie(torch, sm, sc, M, B, sc.keys, sc.qmins, sc.thr, sc.map_of, sc.r2_caps, rows, speed_of, (T_, B, M, last), last=last)
                seen |= set(out.user.tolist())
                worst, hits = max(worst, out.worst), hits + int((out.at >= 0).sum())
                if not last:
                    assert out.harm[0].tolist() == [0.0, 0.0] and out.user[0] == -1 and (out.at[:, 0] == -1).all() and (out.speed[:, 0] == 0.0).all()
    print(f"T = {T_}: worst |harm - checker| = {worst:.3e}, {hits} (class, trajectory) pairs with a hit, users chosen {sorted(seen)}")
    assert -1 in seen and (sc.M < 10 or len(seen) >= 2)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C_", [1, 4, 5, 8])
def test_tie_over_class_and_map_counts(torch_cuda, C_, K):
    """C in {1, 4, 5, 8} x K in {1, 2, 3}: all six instantiations, widths with classes that are not there, class c on map (c + 1) % K --
    and, with K >= 2, map 1 handed over as the very BUFFER of map 0"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc, keys, qmins, cap = UG._three_maps()
    map_of = [(c + 1) % K for c in range(C_)]
    rows, speed_of = IC.rows_of(IC.KINDS8[:C_]), UG.SPEEDS8[:C_]
    seen = set()
    for B in (1, 5, 31):
        out = _tie(torch, sm, sc, sc.M, B, keys[:K], qmins[:K], sc.thr[:C_], map_of, [cap] * K, rows, speed_of, (C_, K, B))
        seen |= set(out.user.tolist())
    assert len(seen) >= 2
    if K >= 2:
        same = [keys[0]] + keys[:K - 1]
        same_q = [qmins[0]] + qmins[:K - 1]
        _tie(torch, sm, sc, sc.M, 5, same, same_q, sc.thr[:C_], map_of, [cap] * K, rows, speed_of, (C_, K, "alias"), alias=(1, 0))


# ------------------------------------------------------------------------------------------------ 2. a hand case with known numbers
# the pedestrian of IC.KINDS5 against an ego of IC.EGO_MASS, walking at 2 m/s: split_obst = 1093.3 / (1093.3 + 75), p0 = 3.164,
# p1 = -0.288 * split_obst, p2 = 4.591, p3 = -0.185 * 75 / (1093.3 + 75)
PED_ROW = (3.164, -0.26951159804844643, 4.591, -0.011876230420268767)
HAND = [
    # v0, a_brake, wall_x, B -> first, speed, at, (obstacle harm, ego harm), user
    # 8 m/s, 4 m/s^2, dt 0.5: from b = 0 the speeds are 8 6 4 2 0 and the poses 0 4 7 9 10 m; the front reaches the wall at 10 m at
    # sample 2, where the ego has 8 - 4 * (2 * 0.5) = 4 m/s left: w = 6, 1 / (1 + exp(3.164 - 0.2695... * 6))
    ((8.0, 4.0, 10.0, 1), 2, 4.0, 0, (0.17553005433799326, 0.01077447298141762), 0),
    # the wall at 14 m: braking from b = 0 the ego comes to rest short of it; the candidate itself reaches it at sample 3 (x = 12 m), so
    # every start b >= 3 meets it at v[3] = 8 m/s, and the starts 1, 2 at less: w = 10
    ((8.0, 4.0, 14.0, 6), 3, 8.0, 3, (0.3848804152117187, 0.011292746193229827), 0),
    # 2 m/s: the ego stands after one step of 1 m, far short of the wall: no hit start, no harm
    ((2.0, 4.0, 14.0, 1), 11, 0.0, -1, (0.0, 0.0), -1),
    # a_brake = 0: the manoeuvre is the candidate, met at sample 3 at the full 8 m/s from b = 0 on
    ((8.0, 0.0, 14.0, 1), 3, 8.0, 0, (0.3848804152117187, 0.011292746193229827), 0),
]


def test_hand_case_with_known_numbers(torch_cuda):
    torch = torch_cuda
    sm, road = UG._parked()
    assert np.abs(IC.rows_of((IC.KINDS5[0],))[0] - np.array(PED_ROW)).max() <= 1e-15
    for (v0, a_brake, wall_x, B), first, speed, at, harm, user in HAND:
        h = IC.wall_case(v0, a_brake, wall_x)
        assert np.array_equal(road, h.road)
        rc, msg, out = _raw_impact(torch, sm, h.win, [h.r2_cap], [h.key], [h.qmin], h.x, h.y, h.head, h.v, h.arc, h.a_brake, h.dt, h.thr, [0], B,
                                   [PED_ROW], [2.0])
        assert rc == 0, msg
        what = (v0, a_brake, wall_x, B)
        assert out.first.tolist() == [[first]] and out.speed.tolist() == [[speed]] and out.at.tolist() == [[at]] and out.user.tolist() == [user], what
        assert abs(out.harm[0, 0] - harm[0]) <= TOL and abs(out.harm[0, 1] - harm[1]) <= TOL, (what, out.harm.tolist())
        if at < 0:
            assert out.harm.tolist() == [[0.0, 0.0]] and out.commit.tolist() == [[-1]]
        # the same numbers from the formula, not from the recorded digits
        if at >= 0:
            assert abs(harm[0] - 1.0 / (1.0 + math.exp(PED_ROW[0] + PED_ROW[1] * (speed + 2.0)))) <= 1e-15


# ------------------------------------------------------------------------------------------------ 3. the fold on the device
def _iv(**over):
    kw = dict(vehicle=VG.VEH3, ego_mass=RC.VEH[3], users=VG.USERS, kinds=STEP_KINDS, dt=0.1, a_brake=8.0, starts=5, harm_limit=0.1)
    kw.update(over)
    return kw


def _step_then_stage(torch, k, tr=None, **over):
    """a plain PlanningStep.run, its cost / safe copied, then the stage by its own call (on ``tr`` where given): (before, after, result)"""
    from frenetix_occlusion.step import PlanningStep
    tr = k.tr if tr is None else tr
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced")
    out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    assert not hasattr(out, "hidden_impact_verdict")
    before = (out.cost.clone(), out.safe.clone())
    iv = k.sm.hidden_brake_impact(*tr[:4], cost=out.cost, safe=out.safe, **_iv(**over))
    torch.cuda.synchronize()
    return (_np(before[0]), _np(before[1])), (_np(out.cost), _np(out.safe)), iv


def _assert_fold(before, after, iv, harm_limit):
    cost0, safe0 = before
    cost1, safe1 = after
    harm, user = _np(iv.harm), _np(iv.user)
    want_cost, want_safe = RI.fold(cost0, safe0, harm, user, harm_limit)
    assert cost1.tobytes() == want_cost.tobytes() and np.array_equal(safe1, want_safe)
    others = [c for c in range(16) if c not in (RI.C_SAFE, RI.C_RES0, RI.C_RES1)]
    assert cost1[:, others].tobytes() == cost0[:, others].tobytes()             # bit-identical, NaNs included
    assert (safe1 <= safe0).all()                                               # only ever 1 -> 0
    assert cost1[:, RI.C_RES0].tobytes() == harm[:, 0].tobytes() and np.array_equal(cost1[:, RI.C_RES1], user.astype(np.float64))


def _assert_stage_is_the_checker(torch, k, iv, B, x, y, v):
    """the tie through the Python layer: the users entry on the very device data the stage walked on, then the checker"""
    w = k.sm.window
    rc, msg, users = UG._raw_users(torch, k.sm, (w.ix0, w.iy0, w.nx, w.ny), [c.r2_cap for c in iv.clearances], [_np(c.key) for c in iv.clearances],
                                   [_np(c.qmin) for c in iv.clearances], x, y, _np(iv.poses.heading), v, _np(iv.poses.arc), 8.0, 0.1, iv.thr,
                                   iv.map_of)
    assert rc == 0, msg
    out = SimpleNamespace(**{n: _np(getattr(iv, n)) for n in OUTPUTS})
    rows = IC.rows_of(STEP_KINDS, RC.VEH[3])
    assert np.abs(iv.rows - rows).max() <= 1e-15 and iv.speed_of.tolist() == [u[0] for u in VG.USERS]
    return _assert_impact(out, users, v, 8.0, 0.1, B, iv.rows, iv.speed_of, None, "stage", finite=_np(iv.poses.finite))


def test_fold_on_the_rows_of_a_real_step(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    before, after, iv = _step_then_stage(torch, k)
    assert before[1].any() and not np.isnan(before[0][:, :12]).all()
    _assert_fold(before, after, iv, 0.1)
    x, y, v = (_np(t) for t in (k.tr[0], k.tr[1], k.tr[3]))
    _assert_stage_is_the_checker(torch, k, iv, 5, x, y, v)
    harm = _np(iv.harm)
    print(f"step rows: obstacle harm min {harm[:, 0].min():.4f} max {harm[:, 0].max():.4f}, {len(set(harm[:, 0].tolist()))} distinct values over "
          f"{len(harm)} candidates; users {sorted(set(_np(iv.user).tolist()))}")
    assert (harm[:, 0] > 0.0).any() and (harm[:, 0] < 1.0).all() and len(set(harm[:, 0].tolist())) > 2     # graded, not one value
    assert iv.starts == 5 and iv.harm_limit == 0.1 and iv.map_of == (0, 1, 0)
    assert torch.equal(iv.critical_user(), iv.user.to(torch.int64)) and torch.equal(iv.obstacle_harm(), iv.harm[:, 0]) and torch.equal(iv.ego_harm(), iv.harm[:, 1])
    # the chosen user's speed and harm by the accessors
    user = _np(iv.user)
    picked = _np(iv.impact_speed())
    want = np.where(user >= 0, _np(iv.speed)[np.clip(user, 0, None), np.arange(len(user))], 0.0)
    assert np.array_equal(picked, want) and torch.equal(iv.impact_speed(1), iv.speed[1])
    per = np.stack([_np(iv.harm_of(c)) for c in range(3)])                        # [C, M, 2]
    best = np.where(user >= 0, per[np.clip(user, 0, None), np.arange(len(user)), 0], 0.0)
    assert np.abs(best - harm[:, 0]).max() <= TOL and np.abs(per[:, :, 0].max(axis=0) - harm[:, 0]).max() <= TOL
    # harm_limit = inf takes nothing away from finite candidates; 0 takes every candidate with a hit
    before, after, iv_inf = _step_then_stage(torch, k, harm_limit=math.inf)
    _assert_fold(before, after, iv_inf, math.inf)
    assert np.array_equal(after[1], before[1])
    before, after, iv0 = _step_then_stage(torch, k, harm_limit=0.0)
    _assert_fold(before, after, iv0, 0.0)
    assert np.array_equal(after[1], before[1] * (_np(iv0.user) == -1))


def test_a_refused_step_stays_unsafe_and_gets_the_two_columns(torch_cuda):
    torch = torch_cuda
    import test_rule_refusal_gpu as RG
    k = VG._stack(torch, RG.REFUSING_CELL)
    before, after, iv = _step_then_stage(torch, k)
    RG.assert_refused(SimpleNamespace(cost=torch.as_tensor(before[0]), safe=torch.as_tensor(before[1])))
    _assert_fold(before, after, iv, 0.1)
    assert not after[1].any() and (after[0][:, RI.C_SAFE] == 0.0).all()
    others = [c for c in range(14) if c != RI.C_SAFE]
    assert np.isnan(after[0][:, others]).all() and after[0][:, RI.C_RES0].tobytes() == _np(iv.harm)[:, 0].tobytes()
    assert (after[0][:, RI.C_RES0] > 0).any()


def test_a_non_finite_candidate_fails_closed(torch_cuda):
    """a NaN, an inf and a -inf in x, theta and v of three candidates as the stage sees them: harm (1, 1), user -2 and safe = 0 even at
    harm_limit = inf, which takes nothing else away"""
    torch = torch_cuda
    k = VG._stack(torch)
    tr = [t.clone() for t in k.tr]
    tr[0][3, 7], tr[2][11, 0], tr[3][40, 15] = float("nan"), float("inf"), float("-inf")
    before, after, iv = _step_then_stage(torch, k, tr=tr, harm_limit=math.inf)
    _assert_fold(before, after, iv, math.inf)
    harm, user = _np(iv.harm), _np(iv.user)
    for m in (3, 11, 40):
        assert (harm[m].tolist(), user[m], after[1][m], after[0][m, RI.C_SAFE], after[0][m, RI.C_RES0], after[0][m, RI.C_RES1]) == ([1.0, 1.0], -2, 0, 0.0, 1.0, -2.0), m
    rest = [m for m in range(RC.M) if m not in (3, 11, 40)]
    assert _np(iv.poses.finite).sum() == RC.M - 3 and (user[rest] >= -1).all() and np.array_equal(after[1][rest], before[1][rest])


# ------------------------------------------------------------------------------------------------ 4. the planning step
def test_step_with_the_stage_is_the_stage_by_stage_calls(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion.step import PlanningStep
    k = VG._stack(torch)
    plain, staged, iv = _step_then_stage(torch, k)
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_impact_verdict=_iv())
    for _ in range(2):                                              # (a second run folds into fresh rows, not into folded ones)
        out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
        torch.cuda.synchronize()
        assert _np(out.cost).tobytes() == staged[0].tobytes() and np.array_equal(_np(out.safe), staged[1])
        for name in OUTPUTS:
            assert torch.equal(getattr(out.hidden_impact_verdict, name), getattr(iv, name)), name
    assert (staged[1] < plain[1]).any() and (_np(iv.user) >= 0).any()
    # None: no such attribute, and cost / safe are the step's
    out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_impact_verdict=None).run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert not hasattr(out, "hidden_impact_verdict") and _np(out.cost).tobytes() == plain[0].tobytes() and np.array_equal(_np(out.safe), plain[1])
    for two in (dict(hidden_verdict=VG._hv(), hidden_impact_verdict=_iv()),
                dict(hidden_ladder_verdict=dict(vehicle=VG.VEH3, users=VG.USERS, dt=0.1, levels=[2.0, 8.0], starts=5, a_limit=8.0),
                     hidden_impact_verdict=_iv())):
        with pytest.raises(ValueError, match="same two reserved cost columns"):
            PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", **two)
    with pytest.raises(ValueError, match="hidden_impact_verdict"):
        PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_impact_verdict=dict(users=VG.USERS))


def test_rows_are_uploaded_once_per_set_of_users(torch_cuda):
    """the second call with the same users, kinds, mass and coefficients reuses the device buffer of the first"""
    torch = torch_cuda
    k = VG._stack(torch)
    k.sm.launch(k.sc.ego, k.sc.yaw)
    k.sm.hidden_brake_impact(*k.tr[:4], **_iv())
    first = dict(k.sm._hbi_rows)
    k.sm.hidden_brake_impact(*k.tr[:4], **_iv(harm_limit=0.5, starts=3))
    assert len(first) >= 1 and all(k.sm._hbi_rows[key][2] is val[2] for key, val in first.items()) and len(k.sm._hbi_rows) == len(first)
    k.sm.hidden_brake_impact(*k.tr[:4], **_iv(ego_mass=2000.0))
    torch.cuda.synchronize()
    assert len(k.sm._hbi_rows) == len(first) + 1


def test_through_the_interface(torch_cuda, tmp_path):
    """FOInterface.hidden_brake_impact on scenario 1: harm_limit from the configuration's metric_thresholds.harm, a_brake from a_max,
    the default kinds by ascending speed with the dimensions of the agent manager's phantoms -- the sensor model's call with all of
    that spelled out, bit for bit"""
    torch = torch_cuda
    import test_hidden_witness_gpu as WG
    from frenetix_occlusion import synthetic as SY
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    ego, yaw = WG._drive(fo, sc, 3)
    traj = SY.make_trajectories(64, 31, WG.DT, seed=WG.SEED, ego_pos=ego, ego_yaw=yaw)
    users = ((13.9, "road", "lanes"), (2.0, "road", "any"), (7.0, "road", "lanes"))       # not in order of speed on purpose
    iv = fo.hidden_brake_impact(traj, users, starts=5)
    pr, am = fo.config["agent_manager"]["prediction"], fo.config["agent_manager"]
    kind = lambda name, fl, fw: (name, am[name.lower()]["length"] * pr[fl], am[name.lower()]["width"] * pr[fw])
    want_kinds = (kind("Car", "size_factor_length_s", "size_factor_width_s"), kind("Pedestrian", "size_factor_length_s", "size_factor_width_s"),
                  kind("Bicycle", "size_factor_length_l", "size_factor_width_l"))
    assert iv.kinds == want_kinds and fo.phantom_kind("Car") == want_kinds[0]
    limit = fo.config["metrics"]["metric_thresholds"]["harm"]
    assert iv.harm_limit == (math.inf if limit is None else float(limit)) and iv.starts == 5
    veh = SY.VEHICLE_BMW320I
    ref = fo.sensor_model.hidden_brake_impact(traj["x"], traj["y"], traj["theta"], traj["v"], vehicle=veh[:3], ego_mass=veh[3], users=users,
                                              kinds=want_kinds, dt=WG.DT, a_brake=veh[4], starts=5, harm_limit=iv.harm_limit,
                                              margin=fo.occlusion_memory["margin"])
    torch.cuda.synchronize()
    for name in OUTPUTS:
        assert torch.equal(getattr(iv, name), getattr(ref, name)), name
    assert np.abs(iv.rows - IC.rows_of(want_kinds, veh[3])).max() <= 1e-15
    named = fo.hidden_brake_impact(traj, users, kinds=("Car", "Pedestrian", ("Bicycle",) + want_kinds[2][1:]), harm_limit=0.5, starts=5)
    assert named.kinds == want_kinds and named.harm_limit == 0.5 and torch.equal(named.harm, iv.harm)
    with pytest.raises(ValueError, match="kinds is required"):
        fo.hidden_brake_impact(traj, users[:2])
    with pytest.raises(ValueError, match="no dimensions"):
        fo.hidden_brake_impact(traj, users, kinds=("Car", "Tram", "Bicycle"))


# ------------------------------------------------------------------------------------------------ 5. every byte is written
def test_every_byte_of_every_output_is_written(torch_cuda):
    """the outputs are pre-filled with a byte pattern: after a call no element holds it, at M below, at and above a multiple of the
    trajectories per workgroup, with and without lengths and finite flags"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc = VG._scene(VG.TIE_SCENES[31], US.USERS)
    rows, speed_of = IC.rows_of(IC.KINDS5), [u[0] for u in US.USERS]
    per = VG._per_block(31, 3, 5)
    for M in (1, per - 1, per, per + 1, sc.M):
        for lens, finite in ((None, None), (sc.lens[:M], np.arange(M, dtype=np.uint8) % 2)):
            rc, msg, out = _raw_impact(torch, sm, sc.win, sc.r2_caps, sc.keys, [q[:M] for q in sc.qmins], sc.x[:M], sc.y[:M], sc.head[:M], sc.v[:M],
                                       sc.arc[:M], sc.a_brake, sc.dt, sc.thr, sc.map_of, 5, rows, speed_of, lens=lens, finite=finite)
            assert rc == 0, msg
            _assert_written(out, (M, lens is None))
            assert not _untouched(out)
            if finite is not None:
                assert (out.user[finite == 0] == -2).all() and (out.harm[finite == 0] == 1.0).all() and (out.user[finite == 1] >= -1).all()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_of_the_c_entry(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, _ = UG._parked()
    h = IC.wall_case(8.0, 4.0, 10.0)
    cost0, safe0 = np.full((1, 16), 0.5), np.ones(1, dtype=np.uint8)
    base = dict(lens=None, finite=np.ones(1, dtype=np.uint8), cost=cost0, safe=safe0, harm_limit=0.1)

    def call(B=1, thr=h.thr, keys=None, r2=None, map_of=(0,), **kw):
        args = dict(base)
        args.update(kw)
        a_brake, dt = args.pop("a_brake", h.a_brake), args.pop("dt", h.dt)
        return _raw_impact(torch, sm, h.win, [h.r2_cap] if r2 is None else r2, [h.key] if keys is None else keys,
                           [h.qmin] * (1 if keys is None else len(keys)), h.x, h.y, h.head, h.v, h.arc, a_brake, dt, thr, map_of, B, [PED_ROW], [2.0],
                           **args)

    def refused(what, **kw):
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_impact:") and what in msg, (what, rc, msg)
        assert _untouched(out), what                                                    # nothing was launched: every byte of the pattern stands
        assert (out.cost is None or (out.cost == 0.5).all()) and (out.safe is None or (out.safe == 1).all()), what

    rc, msg, out = call()
    assert rc == N.FO_OK and out.speed.tolist() == [[4.0]] and out.safe.tolist() == [0] and out.cost[0, RI.C_RES0] == out.harm[0, 0] > 0.1, msg
    rc, msg, out = call(harm_limit=math.inf)
    assert rc == N.FO_OK and out.safe.tolist() == [1] and out.cost[0, RI.C_SAFE] == 0.5, msg
    refused("harm_limit", harm_limit=-0.5)
    refused("harm_limit", harm_limit=float("nan"))
    refused("d_speed_of", drop=("d_speed_of",))
    refused("d_speed_of", drop=("d_harm_rows",))
    refused("B = 0", B=0)
    refused("B = 17", B=h.T + 1)
    refused("go together", cost=None)
    refused("go together", safe=None)
    rc, msg, out = call(cost=None, safe=None, finite=None)                              # neither, and no finite flags: served
    assert rc == N.FO_OK and out.speed.tolist() == [[4.0]], msg
    refused("K = 0", K=0)
    refused("K = 4", K=4)
    refused("C = 0", C=0)
    refused("C = 9", C=9)
    refused("h_thr", h_thr=None)
    refused("window", win_nx=0)
    refused("r2_cap[0]", r2=[-1])
    refused("map_of[0] = 1", map_of=(1,))
    refused("M = -1", M=-1)
    refused("a_brake", a_brake=float("nan"))
    refused("a_brake", a_brake=-1.0)
    refused("dt", dt=0.0)
    refused("T = 255", T=255)
    refused("decreases", thr=np.array([[5, 4] + [9] * (h.T - 2)]))
    refused("negative", thr=np.array([[-1] * h.T]))
    refused("lies beyond", thr=h.thr + 169 * (h.r2_cap + 1))
    refused("FO_HIDDEN_BRAKE_MAX_TABLE", C=8, T=113, map_of=(0,) * 8)
    for name in ("d_x", "d_y", "d_heading"):
        refused("d_x", drop=(name,))
    refused("d_key[0]", drop_map=(("d_key", 0),))
    refused("d_key[0]", drop_map=(("d_qmin", 0),))
    refused("d_v", drop=("d_v",))
    refused("d_v", drop=("d_arc",))
    for name in ("d_harm", "d_user", "d_speed", "d_at", "d_commit", "d_first"):
        refused("d_harm", drop=(name,))
    refused("half extents", hl=-0.1)
    rc, msg, out = call(M=0)                                                            # M = 0: FO_OK, nothing launched
    assert rc == N.FO_OK and _untouched(out)
    ctx = N.Context(0)                                                                  # a context without a map
    assert ctx._lib.fo_scene_hidden_brake_impact(ctx._h, C.byref(N.HiddenBrakeImpact()), None) == N.FO_E_STATE


def test_refusals_of_the_python_layer(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    k.sm.launch(k.sc.ego, k.sc.yaw)
    call = lambda **over: k.sm.hidden_brake_impact(*k.tr[:4], **_iv(**over))
    cost = torch.zeros((RC.M, 16), dtype=torch.float64, device=k.sm.device)
    safe = torch.ones((RC.M,), dtype=torch.uint8, device=k.sm.device)
    for bad in (dict(starts=0), dict(starts=17), dict(harm_limit=-1.0), dict(harm_limit=float("nan")), dict(harm_limit=None),
                dict(kinds=STEP_KINDS[:2]), dict(kinds=(("Building", 1.0, 1.0),) * 3), dict(kinds=("Car",) * 3), dict(ego_mass=0.0),
                dict(ego_mass="heavy"), dict(coeff=dict(lr4s_const=1.0)), dict(cost=cost), dict(safe=safe), dict(cost=cost[:5], safe=safe),
                dict(a_brake=-1.0), dict(users=())):
        with pytest.raises(ValueError, match="hidden_brake_impact"):
            call(**bad)
    assert (cost == 0).all() and (safe == 1).all()
    iv = call(cost=cost, safe=safe, starts=None)
    torch.cuda.synchronize()
    assert iv.starts == RC.T and torch.equal(cost[:, RI.C_RES0], iv.harm[:, 0])
