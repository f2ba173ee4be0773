"""Hidden-traffic fail-safe verdict on the device (fo_scene_hidden_poses, fo_scene_hidden_brake_verdict, PlanningStep(hidden_verdict=);
DESIGN.md §5.10 "Fail-safe verdict"): the tie to fo_scene_hidden_brake_users of the same library on the same device inputs and to the
fold of tests/ref_hidden_brake_verdict.py, the pose preparation against numpy, the fold on cost rows a real planning step left, the
step with and without the stage, the refusals.  Every verdict output is an exact integer: all comparisons are ``==``.  Every test runs
under a time limit of its own that ends the process (a hung kernel cannot be waited out from Python); no test provokes a fault."""
import faulthandler
import glob
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_scenes as SC
import hidden_brake_users_scenes as US
import ref_hidden_brake_verdict as BV
import rule_refusal_cases as RC
import test_hidden_brake_users_gpu as UG
import test_hidden_brake_verdict_cpu as VC
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
OUTPUTS = ("fail_safe", "user", "commit", "first")
STEP_LIMIT = 240          # seconds a test may take before the process is ended with every thread's traceback
TRACE_LIMIT = 200         # ... and a traced child process of the trace test; that test starts two of them
USERS = ((1.5, "road", "any"), (4.0, "euclid", "any"), (6.0, "road", "any"))      # of the step tests: two maps, three classes
VEH3 = RC.VEH[:3]


@pytest.fixture(autouse=True)
def _time_limit(request):
    faulthandler.dump_traceback_later(getattr(request.module, request.function.__name__ + "_limit", STEP_LIMIT), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw_verdict(torch, sm, win, r2_caps, keys, qmins, x, y, head, v, arc, a_brake, dt, thr, map_of, B, commit_min=0, lens=None,
                 finite=None, cost=None, safe=None, alias=(), hl=HL, hw=HW, wb=WB, drop=(), drop_map=(), **over):
    """fo_scene_hidden_brake_verdict on maps and trajectories of the test's own; the output buffers are pre-filled with a pattern.
    ``cost`` / ``safe``: host arrays, uploaded and returned as the call left them; ``alias``: (k, j) -- map k is the BUFFER of map j;
    ``drop`` / ``drop_map`` / ``over`` as in tests/test_hidden_brake_users_gpu._raw_users.  Returns (rc, message, outputs)"""
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
    out = SimpleNamespace(fail_safe=torch.full((M,), -7, dtype=torch.int32, device=dev), user=torch.full((M,), -7, dtype=torch.int32, device=dev),
                          commit=torch.full((Cn, M), -7, dtype=torch.int32, device=dev),
                          first=torch.full((Cn, M), -7, dtype=torch.int32, device=dev))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    pad = lambda vals, n, fill: (list(vals) + [fill] * n)[:n]
    ptrs = dict(d_key=pad([p(t) for t in dk], 3, None), d_qmin=pad([p(t) for t in dq], 3, None))
    for name, k in drop_map:
        ptrs[name][k] = None
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=hl, hw=hw, wb=wb, win_ix0=win[0], win_iy0=win[1],
              win_nx=win[2], win_ny=win[3], K=Kn, C=Cn, d_key=(C.c_void_p * 3)(*ptrs["d_key"]), d_qmin=(C.c_void_p * 3)(*ptrs["d_qmin"]),
              r2_cap=(C.c_int32 * 3)(*pad([int(r) for r in r2_caps], 3, -5)), map_of=(C.c_int32 * 8)(*pad([int(k) for k in map_of], 8, 99)),
              d_v=p(tv), d_arc=p(ta), a_brake=float(a_brake), dt=float(dt), h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), B=int(B),
              commit_min=int(commit_min), d_finite_or_null=p(tf), d_cost_or_null=p(tc), d_safe_or_null=p(ts),
              d_fail_safe=p(out.fail_safe), d_user=p(out.user), d_commit=p(out.commit), d_first=p(out.first))
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeVerdict(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_verdict(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    res = SimpleNamespace(**{k: _np(getattr(out, k)) for k in OUTPUTS})
    res.cost, res.safe = (None if tc is None else _np(tc)), (None if ts is None else _np(ts))
    return rc, msg, res


def _tie(torch, sm, sc, M, B, keys, qmins, thr, map_of, r2_caps, what, alias=(), last=False):
    """the verdict on the first M trajectories of the scene (``last``: its last M) against the users entry on the same device inputs
    and the checker's fold"""
    cut = lambda a: None if a is None else (a[len(a) - M:] if last else a[:M])
    x, y, head, v, arc, lens = (cut(a) for a in (sc.x, sc.y, sc.head, sc.v, sc.arc, sc.lens))
    qm = [cut(q) for q in qmins]
    rc, msg, users = UG._raw_users(torch, sm, sc.win, r2_caps, keys, qm, x, y, head, v, arc, sc.a_brake, sc.dt, thr, map_of, lens)
    assert rc == 0, msg
    rc, msg, out = _raw_verdict(torch, sm, sc.win, r2_caps, keys, qm, x, y, head, v, arc, sc.a_brake, sc.dt, thr, map_of, B, lens=lens,
                                alias=alias)
    assert rc == 0, (what, msg)
    commit, fail_safe, user = BV.verdict(users.commit, B)
    for name, want in (("commit", commit), ("first", users.first), ("fail_safe", fail_safe), ("user", user)):
        got = getattr(out, name)
        assert got.dtype == np.int32 and got.shape == want.shape, (what, name)
        assert np.array_equal(got, want), (what, name, np.argwhere(got != want)[:4].tolist())
    return out


def _per_block(T_, K, B):
    G = min(64, 1 << (B - 1).bit_length())
    return max(1, min(256 // G, 32768 // (T_ * (48 + 4 * K))))


_scenes = {}


def _scene(spec, users):
    if (spec, users) not in _scenes:
        _scenes[spec, users] = US.user_scene(spec, users)
    return _scenes[spec, users]


# ------------------------------------------------------------------------------------------------ 1. the tie
# (seed, M, T, entry, ragged): M is at least the largest per_block + 1 of the brake starts asked at that T, and leaves rows behind the
# scene's first three (the lengths 0, 1, 2) for the cut from the end
TIE_SCENES = {1: (111, 260, 1, 0, True), 2: (112, 260, 2, 1, True), 31: (113, 21, 31, 2, True), 64: (114, 12, 64, 0, True),
              65: (115, 12, 65, 1, True), 254: (116, 6, 254, 2, True)}


def _starts(T_):
    """B in {1, 2, 5, T}; at T = 31 also 3 and 12, so that every group size below 64 is run (64 is B = T at T >= 64)"""
    return sorted({b for b in (1, 2, 5, T_) + ((3, 12) if T_ == 31 else ()) if b <= T_})


@pytest.mark.parametrize("T_", sorted(TIE_SCENES))
def test_tie_to_the_users_entry_at_every_group_size(torch_cuda, T_):
    """T in {1, 2, 31, 64, 65, 254} x B in {1, 2, 5, T} (and 3, 12 at T = 31: G = 4 and 16): commit, first, fail_safe and user are
    fo_scene_hidden_brake_users' and the checker's fold, bit for bit, with M at per_block - 1, per_block, per_block + 1 of every
    (T, B), on three maps (five users; three at T = 254, where the table holds no more).  Every (T, B, M) is run twice: on the scene's
    FIRST M trajectories, which begin with the lengths 0, 1, 2 (so every one of them has those, and lengths below B), and on its LAST
    M, whose ragged lengths are the seed's (negative ones, ones beyond T, ones below B, whole ones)"""
    torch = torch_cuda
    sm, _ = UG._parked()
    users = UG.THREE if T_ == 254 else US.USERS
    sc = _scene(TIE_SCENES[T_], users)
    assert len(sc.keys) == 3 and sc.lens[:3].tolist() == [0, 1, 2]
    groups, verdicts = set(), set()
    for B in _starts(T_):
        per = _per_block(T_, 3, B)
        groups.add(min(64, 1 << (B - 1).bit_length()))
        for M in sorted({m for m in (per - 1, per, per + 1) if m >= 1}):
            assert M + 3 <= sc.M
            for last in (False, True):
                out = _tie(torch, sm, sc, M, B, sc.keys, sc.qmins, sc.thr, sc.map_of, sc.r2_caps, (T_, B, M, last), last=last)
                verdicts |= {("B" if f == B else f if f == 0 else "mid") for f in out.fail_safe.tolist()}
                assert ((out.user == -1) == (out.fail_safe == B)).all() and (out.commit < B).all()
                if not last:
                    assert out.fail_safe[0] == B and (out.commit[:, 0] == -1).all() and (out.first[:, 0] == -1).all()   # length 0
    assert groups == {1: {1}, 2: {1, 2}, 31: {1, 2, 4, 8, 16, 32}}.get(T_, {1, 2, 8, 64})
    assert "B" in verdicts and (sc.M < 10 or 0 in verdicts or "mid" in verdicts)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C_", [1, 4, 5, 8])
def test_tie_over_class_and_map_counts(torch_cuda, C_, K):
    """C in {1, 4, 5, 8} x K in {1, 2, 3}: all six instantiations, widths with classes that are not there, class c on map (c + 1) % K so
    that classes share a map -- and, with K >= 2, map 1 handed over as the very BUFFER of map 0"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc, keys, qmins, cap = UG._three_maps()
    map_of = [(c + 1) % K for c in range(C_)]
    seen = set()
    for B in (1, 5, 31):
        out = _tie(torch, sm, sc, sc.M, B, keys[:K], qmins[:K], sc.thr[:C_], map_of, [cap] * K, (C_, K, B))
        seen |= set(out.user.tolist())
    assert -1 in seen and (C_ == 1 or len(seen) >= 2)
    if K >= 2:
        same = [keys[0]] + keys[:K - 1]
        same_q = [qmins[0]] + qmins[:K - 1]
        _tie(torch, sm, sc, sc.M, 5, same, same_q, sc.thr[:C_], map_of, [cap] * K, (C_, K, "alias"), alias=(1, 0))


def test_against_the_checkers_own_walk(torch_cuda):
    """the ties above hold the verdict against the users ENTRY, whose kernel walks a manoeuvre with the very code this kernel walks
    with (hbu_walk): a fault in it moves both alike.  Here the checker's walk (tests/ref_hidden_brake_users.py) and fold stand in the
    entry's place: T = 31, five users on three maps, ragged lengths, B in {1, 5, T}"""
    torch = torch_cuda
    sm, road = UG._parked()
    sc = _scene(TIE_SCENES[31], US.USERS)
    assert len(sc.keys) == 3
    _, _, ref_commit, ref_first = UG.BU.brake_users(sc.keys, sc.win, road, sc.qmins, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, UG.HL,
                                                   UG.HW, UG.WB, sc.a_brake, sc.dt, sc.thr, sc.map_of, sc.lens)
    assert (ref_commit >= 0).any() and (ref_commit < 0).any()
    for B in (1, 5, 31):
        rc, msg, out = _raw_verdict(torch, sm, sc.win, sc.r2_caps, sc.keys, sc.qmins, sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt,
                                    sc.thr, sc.map_of, B, lens=sc.lens)
        assert rc == 0, (B, msg)
        commit, fail_safe, user = BV.verdict(ref_commit, B)
        for name, want in (("commit", commit), ("first", ref_first), ("fail_safe", fail_safe), ("user", user)):
            got = getattr(out, name)
            assert np.array_equal(got, want), (B, name, np.argwhere(got != want)[:4].tolist())


# ------------------------------------------------------------------------------------------------ 2. the pose preparation
def _poses(torch, sm, x, y, theta, v, lens=None):
    out = sm.hidden_poses(*(torch.as_tensor(a).to(sm.device) for a in (x, y, theta, v)), lengths=lens)
    torch.cuda.synchronize()
    return _np(out.heading), _np(out.arc), _np(out.finite)


def test_arc_is_numpys_sequential_sum(torch_cuda):
    """dyadic inputs -- every segment a 3-4-5 triangle in eighths, so that every operation is exact -- and random ones: bit-equal to
    numpy's travelled_arc (a sequential cumsum, uncontracted products); T = 1, 2, 31 and 254, M on both sides of the workgroup's 64"""
    torch = torch_cuda
    from frenetix_occlusion.hidden_traffic import travelled_arc
    sm, _ = UG._parked()
    rng = np.random.default_rng(5)
    for M, Tn in ((1, 1), (63, 2), (64, 31), (65, 31), (130, 254)):
        k = rng.integers(-40, 41, (M, Tn)).astype(np.float64)
        flip = rng.integers(0, 2, (M, Tn)) * 2.0 - 1.0
        x, y = np.cumsum(3.0 * k / 8.0, axis=1), np.cumsum(4.0 * k * flip / 8.0, axis=1)
        z = np.zeros((M, Tn))
        _, arc, fin = _poses(torch, sm, x, y, z, z)
        want = travelled_arc(x, y)
        assert np.array_equal(want[:, 1:], np.cumsum(5.0 * np.abs(k[:, 1:]) / 8.0, axis=1)) and arc.tobytes() == want.tobytes(), (M, Tn)
        assert fin.tolist() == [1] * M
        x, y = rng.normal(0.0, 30.0, (M, Tn)), rng.normal(0.0, 30.0, (M, Tn))
        _, arc, _ = _poses(torch, sm, x, y, z, z)
        want = travelled_arc(x, y)
        print(f"arc, random inputs, M = {M}, T = {Tn}: {int((arc != want).sum())} of {arc.size} values differ from numpy")
        assert arc.tobytes() == want.tobytes(), (M, Tn)


HEADING_MEASURED = 2.0 ** -53      # the worst |device - numpy| over THETAS on an MI355X (DESIGN.md §5.10 "Fail-safe verdict", Measured)
HEADING_BOUND = 2.0 * HEADING_MEASURED


def _thetas():
    pi = np.pi
    base = [0.0, -0.0, pi / 2, -pi / 2, pi, -pi, 1e-300, -1e-300, 1e6, -1e6]
    near = [n * pi / 2 + s * 1e-8 for n in range(-8, 9) for s in (-1.0, 1.0)]
    spread = np.linspace(-7.0, 7.0, 203).tolist()
    return np.array(base + near + spread, dtype=np.float64)


def test_heading_is_one_sincos_per_sample(torch_cuda):
    """(cos, sin) against numpy's over 0, +-pi/2, +-pi, +-1e-300, +-1e6 and values 1e-8 off multiples of pi/2: within twice the
    difference measured on an MI355X (another libm under numpy may itself move by an ulp), which is never above 2^-50"""
    torch = torch_cuda
    sm, _ = UG._parked()
    assert HEADING_BOUND <= 2.0 ** -50
    th = _thetas()
    Tn = 31
    M = -(-len(th) // Tn)
    theta = np.resize(th, (M, Tn))
    z = np.zeros((M, Tn))
    head, _, fin = _poses(torch, sm, z, z, theta, z)
    want = np.stack((np.cos(theta), np.sin(theta)), -1)
    worst = float(np.abs(head - want).max())
    print(f"heading: worst |device - numpy| = {worst!r} = {worst / 2.0 ** -53:.3f} * 2^-53 over {len(th)} headings")
    assert worst <= HEADING_BOUND and fin.all()
    assert head[0, 0].tolist() == [1.0, 0.0] and np.abs((head ** 2).sum(-1) - 1.0).max() < 4e-16


def test_finite_flag(torch_cuda):
    """a NaN or an inf in each of the four inputs, before len, at len and beyond it: only a sample before len counts"""
    torch = torch_cuda
    sm, _ = UG._parked()
    Tn, bads = 8, (np.nan, np.inf, -np.inf)
    rows, lens, want = [], [], []
    for which in range(4):
        for bad in bads:
            for at, ln, ok in ((2, 8, 0), (2, 3, 0), (2, 2, 1), (5, 3, 1), (0, 1, 0), (0, 0, 1), (7, 8, 0), (7, 100, 0), (3, -4, 1)):
                rows.append((which, bad, at))
                lens.append(ln)
                want.append(ok)
    M = len(rows)
    arrs = [np.tile(np.linspace(0.0, 1.0, Tn), (M, 1)) for _ in range(4)]
    for m, (which, bad, at) in enumerate(rows):
        arrs[which][m, at] = bad
    lens = np.array(lens, dtype=np.int32)
    _, _, fin = _poses(torch, sm, *arrs, lens=lens)
    assert fin.dtype == np.uint8 and fin.tolist() == want == BV.finite_flags(*arrs, lens).tolist()
    _, _, fin = _poses(torch, sm, *arrs)                           # without lengths every sample counts
    assert fin.tolist() == [0] * M


# ------------------------------------------------------------------------------------------------ 3. the fold on the device
_stacks = {}


def _stack(torch, cell=0.5):
    """sensor model + spawn locator + sweep of tests/rule_refusal_cases.py on the right-turn scene (built once per cell size): 130
    candidates of 16 samples; at 0.25 m cells the rule list is refused"""
    if cell not in _stacks:
        _stacks[cell] = RC.stack(torch, RC.turn_scene(cell))
    return _stacks[cell]


def _hv(**over):
    kw = dict(vehicle=VEH3, users=USERS, dt=0.1, a_brake=8.0, starts=5, commit_min=5)
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
    hv = k.sm.hidden_brake_verdict(*tr[:4], cost=out.cost, safe=out.safe, **_hv(**over))
    torch.cuda.synchronize()
    return (_np(before[0]), _np(before[1])), (_np(out.cost), _np(out.safe)), hv


def _assert_fold(before, after, hv, commit_min):
    cost0, safe0 = before
    cost1, safe1 = after
    fs, user = _np(hv.fail_safe), _np(hv.user)
    want_cost, want_safe = BV.fold(cost0, safe0, fs, user, commit_min)
    assert cost1.tobytes() == want_cost.tobytes() and np.array_equal(safe1, want_safe)
    others = [c for c in range(16) if c not in (BV.C_SAFE, BV.C_RES0, BV.C_RES1)]
    assert cost1[:, others].tobytes() == cost0[:, others].tobytes()             # bit-identical, NaNs included
    assert (safe1 <= safe0).all()                                               # only ever 1 -> 0
    assert np.array_equal(cost1[:, BV.C_RES0], fs.astype(np.float64)) and np.array_equal(cost1[:, BV.C_RES1], user.astype(np.float64))


def test_fold_on_the_rows_of_a_real_step(torch_cuda):
    torch = torch_cuda
    k = _stack(torch)
    before, after, hv = _step_then_stage(torch, k)
    assert before[1].any() and not np.isnan(before[0][:, :12]).all()
    _assert_fold(before, after, hv, 5)
    # the tie through the Python layer: the users entry on the very device data the verdict walked on
    w = k.sm.window
    x, y, v = (_np(t) for t in (k.tr[0], k.tr[1], k.tr[3]))
    rc, msg, users = UG._raw_users(torch, k.sm, (w.ix0, w.iy0, w.nx, w.ny), [c.r2_cap for c in hv.clearances], [_np(c.key) for c in hv.clearances],
                                   [_np(c.qmin) for c in hv.clearances], x, y, _np(hv.poses.heading), v, _np(hv.poses.arc), 8.0, 0.1, hv.thr,
                                   hv.map_of)
    assert rc == 0, msg
    commit, fail_safe, user = BV.verdict(users.commit, 5, _np(hv.poses.finite))
    assert np.array_equal(_np(hv.first), users.first) and np.array_equal(_np(hv.commit), commit) and np.array_equal(_np(hv.fail_safe), fail_safe) and np.array_equal(_np(hv.user), user)
    assert hv.starts == 5 and hv.commit_min == 5 and hv.map_of == (0, 1, 0) and torch.equal(hv.critical_user(), hv.user.to(torch.int64))
    # commit_min = 0 takes nothing away
    before, after, hv0 = _step_then_stage(torch, k, commit_min=0)
    _assert_fold(before, after, hv0, 0)
    assert np.array_equal(after[1], before[1])


def test_hand_case_flips_exactly_the_fast_candidate(torch_cuda):
    """tests/test_hidden_brake_verdict_cpu.hand_case on the device.  The pair it folds into is NOT a step over these two candidates
    with no phantoms, as the issue words it: it is two rows that a real step over the right-turn scene's own candidates found safe --
    rows with a real step's bits in every column, and safe = 1 as an empty agent set would leave it.  What is shown is the fold:
    exactly the fast candidate's flag goes 1 -> 0, the creeping one's row keeps every bit but the two columns"""
    torch = torch_cuda
    k = _stack(torch)
    before, _, _ = _step_then_stage(torch, k, commit_min=0)
    safe_rows = np.flatnonzero(before[1])[:2]
    assert len(safe_rows) == 2
    cost, safe = before[0][safe_rows].copy(), before[1][safe_rows].copy()
    sm, road = UG._parked()
    h = VC.hand_case()
    assert np.array_equal(road, h.road)
    rc, msg, out = _raw_verdict(torch, sm, h.win, [h.r2_cap], [h.key], [h.qmin], h.x, h.y, h.head, h.v, h.arc, h.a_brake, h.dt, h.thr, [0],
                                h.B, commit_min=h.B, finite=np.ones(2, dtype=np.uint8), cost=cost, safe=safe)
    assert rc == 0, msg
    assert out.fail_safe.tolist() == [h.B, 0] and out.user.tolist() == [-1, 0] and out.commit.tolist() == [[-1, 0]]
    assert out.safe.tolist() == [1, 0] and out.cost[:, BV.C_SAFE].tolist() == [cost[0, BV.C_SAFE], 0.0]
    _assert_fold((cost, safe), (out.cost, out.safe), SimpleNamespace(fail_safe=torch.as_tensor(out.fail_safe), user=torch.as_tensor(out.user)), h.B)


def test_a_refused_step_stays_unsafe_and_gets_the_two_columns(torch_cuda):
    torch = torch_cuda
    import test_rule_refusal_gpu as RG
    k = _stack(torch, RG.REFUSING_CELL)
    before, after, hv = _step_then_stage(torch, k)
    RG.assert_refused(SimpleNamespace(cost=torch.as_tensor(before[0]), safe=torch.as_tensor(before[1])))
    _assert_fold(before, after, hv, 5)
    assert not after[1].any() and (after[0][:, BV.C_SAFE] == 0.0).all()
    others = [c for c in range(14) if c != BV.C_SAFE]
    assert np.isnan(after[0][:, others]).all() and np.array_equal(after[0][:, BV.C_RES0], _np(hv.fail_safe).astype(np.float64))
    assert (after[0][:, BV.C_RES0] > 0).any()


def test_a_non_finite_candidate_fails_closed(torch_cuda):
    """a NaN, an inf and a -inf in x, theta and v of three candidates as the stage sees them (the sweep's rows are those of the clean
    candidates: what a sweep makes of such a pose is not this stage's claim)"""
    torch = torch_cuda
    k = _stack(torch)
    tr = [t.clone() for t in k.tr]
    tr[0][3, 7], tr[2][11, 0], tr[3][40, 15] = float("nan"), float("inf"), float("-inf")
    _, after, hv = _step_then_stage(torch, k, tr=tr)
    fs, user = _np(hv.fail_safe), _np(hv.user)
    for m in (3, 11, 40):
        assert (fs[m], user[m], after[1][m], after[0][m, BV.C_SAFE], after[0][m, BV.C_RES1]) == (0, -2, 0, 0.0, -2.0), m
    assert _np(hv.poses.finite).sum() == RC.M - 3 and (user[[m for m in range(RC.M) if m not in (3, 11, 40)]] >= -1).all()


# ------------------------------------------------------------------------------------------------ 4. the planning step
def test_step_with_the_stage_is_the_stage_by_stage_calls(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion.step import PlanningStep
    k = _stack(torch)
    _, staged, hv = _step_then_stage(torch, k)
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_verdict=_hv())
    for _ in range(2):                                              # (a second run folds into fresh rows, not into folded ones)
        out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
        torch.cuda.synchronize()
        assert _np(out.cost).tobytes() == staged[0].tobytes() and np.array_equal(_np(out.safe), staged[1])
        for name in OUTPUTS:
            assert torch.equal(getattr(out.hidden_verdict, name), getattr(hv, name)), name
    assert (staged[1] == 0).any() and (_np(hv.fail_safe) < 5).any()
    with pytest.raises(ValueError, match="hidden_verdict"):
        PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_verdict=dict(users=USERS))


def _run_ranks(tmp_path, world, backend):
    """tests/hidden_verdict_dist_worker.py as ``world`` processes, started as tests/test_distributed_gpu._run_ranks starts its worker"""
    import test_distributed_gpu as DG
    port = DG._free_port()
    out = str(tmp_path / f"verdict_{backend}_{world}.npz")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(T.ROOT, "tests", "hidden_verdict_dist_worker.py"), "--backend", backend,
                                       "--out", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=TRACE_LIMIT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    return np.load(out)


def _check_gathered(z, world):
    """rows [lo, hi) of every rank in cost_all are the unsharded step + stage, bit for bit: the two columns, the lowered flag, and
    every column the stage does not own"""
    M = RC.M
    per = -(-M // world)
    assert int(z["world"]) == world and [tuple(r) for r in z["rows"]] == [(min(r * per, M), min(r * per + per, M)) for r in range(world)]
    assert z["cost_all"].shape == (M, 16) and z["cost_all"].tobytes() == z["ref_cost"].tobytes()
    for lo, hi in z["rows"]:
        assert hi > lo
        assert np.array_equal(z["cost_all"][lo:hi, BV.C_RES0], z["ref_fail_safe"][lo:hi].astype(np.float64))
        assert np.array_equal(z["cost_all"][lo:hi, BV.C_RES1], z["ref_user"][lo:hi].astype(np.float64))
        assert np.array_equal(z["cost_all"][lo:hi, BV.C_SAFE], z["ref_safe"][lo:hi].astype(np.float64))
    # what each rank holds of its own rows, put end to end, is the unsharded answer too (the lengths were cut at the rank's rows)
    assert z["local_cost"].tobytes() == z["ref_cost"].tobytes() and np.array_equal(z["local_safe"], z["ref_safe"])
    assert np.array_equal(z["local_fail_safe"], z["ref_fail_safe"]) and np.array_equal(z["local_user"], z["ref_user"])
    # the stage did something on either side of every boundary, and the case is not degenerate
    want_cost, want_safe = BV.fold(z["plain_cost"], (z["plain_cost"][:, BV.C_SAFE] > 0.5).astype(np.uint8), z["ref_fail_safe"], z["ref_user"], 5)
    assert want_cost.tobytes() == z["ref_cost"].tobytes() and np.array_equal(want_safe, z["ref_safe"])
    assert (z["plain_cost"][:, 14:16] == 0.0).all()
    for lo, hi in z["rows"]:
        assert (z["ref_fail_safe"][lo:hi] < 5).any() and (z["ref_fail_safe"][lo:hi] == 5).any()
        assert (z["plain_cost"][lo:hi, BV.C_SAFE] > z["ref_cost"][lo:hi, BV.C_SAFE]).any()          # a flag was lowered in these rows
    short = np.clip(z["lengths"], 0, RC.T) <= 1                     # no manoeuvre and no sample to meet anything beyond the first
    assert short.any() and (z["ref_fail_safe"][np.clip(z["lengths"], 0, RC.T) == 0] == 5).all()


test_two_ranks_shard_the_step_with_the_stage_limit = TRACE_LIMIT + 60
test_forced_collective_on_the_gpu_carries_the_columns_limit = TRACE_LIMIT + 60


def test_two_ranks_shard_the_step_with_the_stage(torch_cuda, tmp_path):
    """two ranks on one GPU, the collective over gloo (the harness of tests/test_distributed_gpu.py): rank 1 holds rows 65 .. 129, its
    stage runs on those rows and on its cut of the ragged lengths and is queued BEFORE the all-gather -- a stage queued behind it, or
    on the wrong rows, would leave cost_all without rank 1's columns"""
    _check_gathered(_run_ranks(tmp_path, 2, "gloo"), 2)


def test_forced_collective_on_the_gpu_carries_the_columns(torch_cuda, tmp_path):
    """over RCCL: two ranks on two GPUs, or -- RCCL refuses two ranks on one device -- ONE rank with the collective forced: the
    gathered matrix is then a buffer of its own, filled by all_gather_into_tensor on the GPU from the block the stage folded into, so
    a stage queued behind the collective would not show in cost_all"""
    world = min(2, torch_cuda.cuda.device_count())
    _check_gathered(_run_ranks(tmp_path, world, "nccl"), world)


_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import hashlib
import numpy as np, torch
import rule_refusal_cases as RC
import test_hidden_brake_verdict_gpu as VG
from frenetix_occlusion.step import PlanningStep
k = RC.stack(torch, RC.turn_scene(0.5))
ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_verdict=VG._hv() if sys.argv[1] == "with" else None)
h = hashlib.sha256()
for step in range(3):
    out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    cost = out.cost.cpu().numpy().copy()
    cost[:, [12, 14, 15]] = 0.0
    h.update(cost.tobytes())
print("child ok", h.hexdigest())
'''


def _trace(tmp_path, what):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_brake_verdict.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"), tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + what)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), what],
                       capture_output=True, text=True, timeout=TRACE_LIMIT)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    return "\n".join(open(f).read() for f in files).splitlines(), r.stdout.split("child ok")[1].split()[0]


test_kernel_trace_of_the_step_without_the_stage_is_todays_limit = 2 * TRACE_LIMIT + 60


def test_kernel_trace_of_the_step_without_the_stage_is_todays(torch_cuda, tmp_path):
    """three runs of a step: with hidden_verdict=None none of the stage's kernels is launched (no pose preparation, no clearance, no
    brake kernel); with it one pose preparation and one verdict launch per run and the clearances' launches, while the step's own
    kernels are launched as often as before and every column the stage does not own holds the same bits"""
    import collections
    import re
    is_stage = lambda name: name.startswith(("fo_hidden_poses", "fo_hr_", "fo_hc_"))

    def kernels(lines):
        found = [re.search(r"fo_\w+", line) for line in lines]
        return collections.Counter(m.group(0) for m in found if m)

    lines, digest_without = _trace(tmp_path, "without")
    without = kernels(lines)
    assert not any(is_stage(k) for k in without), without
    assert sum(n for k, n in without.items() if k.startswith("fo_reduce_kernel")) == 3 and sum(without.values()) >= 3 * 5, without
    lines, digest_with = _trace(tmp_path, "with")
    with_ = kernels(lines)
    count = lambda k: sum(n for name, n in with_.items() if name.startswith(k))
    assert count("fo_hidden_poses_kernel") == 3 and count("fo_hr_brake_verdict_kernel") == 3 and count("fo_hr_brake") == 3
    assert count("fo_hc_traj_kernel") == 6                          # two maps per run
    assert {k: n for k, n in with_.items() if not is_stage(k)} == dict(without)
    assert digest_with == digest_without


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_of_the_c_entries(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, _ = UG._parked()
    h = VC.hand_case()
    cost0, safe0 = np.full((2, 16), 0.5), np.ones(2, dtype=np.uint8)
    base = dict(lens=None, finite=np.ones(2, dtype=np.uint8), cost=cost0, safe=safe0, commit_min=2)

    def call(B=h.B, thr=h.thr, keys=None, r2=None, map_of=(0,), **kw):
        args = dict(base)
        args.update(kw)
        a_brake, dt = args.pop("a_brake", h.a_brake), args.pop("dt", h.dt)
        return _raw_verdict(torch, sm, h.win, [h.r2_cap] if r2 is None else r2, [h.key] if keys is None else keys,
                            [h.qmin] * (1 if keys is None else len(keys)), h.x, h.y, h.head, h.v, h.arc, a_brake, dt, thr, map_of, B, **args)

    def refused(what, **kw):
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_verdict:") and what in msg, (what, rc, msg)
        assert all((getattr(out, k) == -7).all() for k in OUTPUTS), what               # nothing was launched: every canary stands
        assert (out.cost is None or (out.cost == 0.5).all()) and (out.safe is None or (out.safe == 1).all()), what

    rc, msg, out = call()
    assert rc == N.FO_OK and out.fail_safe.tolist() == [h.B, 0] and out.safe.tolist() == [1, 0], msg
    refused("B = 0", B=0)
    refused("B = 32", B=h.T + 1)
    refused("commit_min = -1", commit_min=-1)
    refused("commit_min = 6", commit_min=h.B + 1)
    refused("go together", cost=None)
    refused("go together", safe=None)
    rc, msg, out = call(cost=None, safe=None, finite=None)                              # neither, and no finite flags: served
    assert rc == N.FO_OK and out.fail_safe.tolist() == [h.B, 0], msg
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
    for name in ("d_fail_safe", "d_user", "d_commit", "d_first"):
        refused("d_fail_safe", drop=(name,))
    refused("half extents", hl=-0.1)
    rc, msg, out = call(M=0)                                                            # M = 0: FO_OK, nothing launched
    assert rc == N.FO_OK and all((getattr(out, k) == -7).all() for k in OUTPUTS)
    ctx = N.Context(0)                                                                  # a context without a map
    args = N.HiddenBrakeVerdict()
    assert ctx._lib.fo_scene_hidden_brake_verdict(ctx._h, C.byref(args), None) == N.FO_E_STATE

    # the pose preparation
    dev = sm.device
    z = torch.zeros((2, 4), dtype=torch.float64, device=dev)
    outs = dict(d_heading=torch.full((2, 4, 2), -7.0, dtype=torch.float64, device=dev), d_arc=torch.full((2, 4), -7.0, dtype=torch.float64, device=dev),
                d_finite=torch.full((2,), 77, dtype=torch.uint8, device=dev))

    def poses(what, **over):
        kw = dict(M=2, T=4, d_x=z.data_ptr(), d_y=z.data_ptr(), d_theta=z.data_ptr(), d_v=z.data_ptr(), d_len_or_null=None,
                  **{n: t.data_ptr() for n, t in outs.items()})
        kw.update(over)
        rc = sm.ctx._lib.fo_scene_hidden_poses(sm.ctx._h, C.byref(N.HiddenPoses(**kw)), N.current_stream(0))
        torch.cuda.synchronize()
        msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_poses:") and what in msg, (what, rc, msg)
        assert (outs["d_heading"] == -7.0).all() and (outs["d_arc"] == -7.0).all() and (outs["d_finite"] == 77).all(), what

    poses("M = -1", M=-1)
    poses("T = 0", T=0)
    poses("T = 255", T=255)
    for name in ("d_x", "d_y", "d_theta", "d_v"):
        poses("d_x", **{name: None})
    for name in outs:
        poses("d_heading", **{name: None})
    assert sm.ctx._lib.fo_scene_hidden_poses(sm.ctx._h, C.byref(N.HiddenPoses(M=0)), N.current_stream(0)) == N.FO_OK
    assert ctx._lib.fo_scene_hidden_poses(ctx._h, C.byref(N.HiddenPoses(M=0)), None) == N.FO_OK      # needs no map


def test_refusals_of_the_python_layer(torch_cuda):
    torch = torch_cuda
    k = _stack(torch)
    k.sm.launch(k.sc.ego, k.sc.yaw)
    call = lambda **over: k.sm.hidden_brake_verdict(*k.tr[:4], **_hv(**over))
    cost = torch.zeros((RC.M, 16), dtype=torch.float64, device=k.sm.device)
    safe = torch.ones((RC.M,), dtype=torch.uint8, device=k.sm.device)
    for bad in (dict(starts=0), dict(starts=17), dict(starts=2.0), dict(commit_min=-1), dict(commit_min=6), dict(commit_min=True),
                dict(cost=cost), dict(safe=safe), dict(cost=cost[:5], safe=safe), dict(cost=cost.float(), safe=safe),
                dict(cost=cost, safe=safe.int()), dict(cost=cost.cpu(), safe=safe.cpu()), dict(a_brake=-1.0), dict(users=())):
        with pytest.raises(ValueError, match="hidden_brake_verdict"):
            call(**bad)
    assert (cost == 0).all() and (safe == 1).all()
    hv = call(cost=cost, safe=safe, starts=None)
    torch.cuda.synchronize()
    assert hv.starts == RC.T and torch.equal(cost[:, BV.C_RES0], hv.fail_safe.to(torch.float64))
