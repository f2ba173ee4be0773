"""Hidden-traffic brake ladder by road users on the device (fo_scene_hidden_brake_ladder_users, DESIGN.md §5.10 "Brake ladder by road
users") against the plain statement of the definition (tests/ref_hidden_brake_ladder_users.py) and against its two parents run on the
same device state: fo_scene_hidden_brake_users level by level and fo_scene_hidden_brake_ladder class by class.  On the seeded scenes
the key maps and qmin arrays are the clearance checkers' and are handed straight to the entry; the checker is handed what the device
was handed.  Every output is an exact integer: all comparisons are ``==``.  Every test runs under a time limit of its own that ends the
process (a hung kernel cannot be waited out from Python); no test provokes a fault."""
import copy
import faulthandler
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_ladder_users_scenes as S
import hidden_brake_scenes as SC
import ref_hidden_brake_ladder_users as LU
import ref_hidden_clearance as HC
import test_hidden_brake_gpu as BG
import test_hidden_brake_ladder_gpu as LG
import test_hidden_brake_users_gpu as UG
import test_hidden_reach_gpu as T
import test_hidden_witness_gpu as WG
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
SUMMARY, DETAIL = LU.SUMMARY, ("brake_first", "stop")
SENTINEL = -7          # no output ever holds it: an element that still does was not written
_parked = BG._parked
STEP_LIMIT = 240       # seconds a test may take before the process is ended with every thread's traceback


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw(torch, sm, sc, detail=True, keys=None, qmins=None, v=None, arc=None, drop=(), drop_map=(), **over):
    """fo_scene_hidden_brake_ladder_users on the maps and trajectories of scene ``sc`` (or on edited data of it); the output buffers are
    pre-filled with SENTINEL.  Arrays that are the same object go up once: two such maps are the same buffer.  ``drop``: names of
    pointers to hand over as NULL; ``drop_map``: (name, k) entries of d_key / d_qmin to hand over as NULL; ``over``: fields of the
    structure to replace, ``levels`` and ``table`` the host arrays.  Returns (rc, message, outputs)"""
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
    keys, qmins, v, arc = pick(keys, "keys"), pick(qmins, "qmins"), pick(v, "v"), pick(arc, "arc")
    M, Tn = sc.x.shape
    thr = np.ascontiguousarray(over.pop("table", sc.thr), dtype=np.int32)
    levels = np.ascontiguousarray(over.pop("levels", sc.levels), dtype=np.float64)
    map_of = over.pop("map_of", sc.map_of)
    r2_caps = over.pop("r2_caps", sc.r2_caps)
    Cn, Kn, Ln, Bn = thr.shape[0], len(keys), len(levels), int(over.get("B", sc.starts))
    Bbuf = min(max(Bn, 1), Tn)                          # (a refused B still gets buffers, which must stay as they are)
    tx, ty, th, tv, ta = (up(a, np.float64) for a in (sc.x, sc.y, sc.head, v, arc))
    dk, dq, tl = [up(k, np.int32) for k in keys], [up(q, np.int32) for q in qmins], up(sc.lens, np.int32)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=dev)
    out = SimpleNamespace(required=full(Cn, M, Bbuf), last_unclear=full(Cn, M, Bbuf), commit=full(Cn, M, Ln), first=full(Cn, M),
                          required_all=full(M, Bbuf), last_unclear_all=full(M, Bbuf), blocking=full(M, Bbuf), brake_first=full(Cn, M, Bbuf, Ln),
                          stop=full(M, Bbuf, Ln))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    pad = lambda vals, n, fill: (list(vals) + [fill] * n)[:n]
    ptrs = dict(d_key=pad([p(t) for t in dk], 3, None), d_qmin=pad([p(t) for t in dq], 3, None))
    for name, k in drop_map:
        ptrs[name][k] = None
    win = sc.win
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=HL, hw=HW, wb=WB, win_ix0=win[0], win_iy0=win[1],
              win_nx=win[2], win_ny=win[3], K=Kn, C=Cn, d_key=(C.c_void_p * 3)(*ptrs["d_key"]), d_qmin=(C.c_void_p * 3)(*ptrs["d_qmin"]),
              r2_cap=(C.c_int32 * 3)(*pad([int(r) for r in r2_caps], 3, -5)), map_of=(C.c_int32 * 8)(*pad([int(k) for k in map_of], 8, 99)),
              d_v=p(tv), d_arc=p(ta), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), L=Ln, B=Bn, dt=float(sc.dt),
              h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), d_required=p(out.required), d_last_unclear=p(out.last_unclear),
              d_commit=p(out.commit), d_first=p(out.first), d_required_all=p(out.required_all), d_last_unclear_all=p(out.last_unclear_all),
              d_blocking=p(out.blocking), d_brake_first_or_null=p(out.brake_first) if detail else None,
              d_stop_or_null=p(out.stop) if detail else None)
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeLadderUsers(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_ladder_users(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(**{k: _np(getattr(out, k)) for k in SUMMARY + DETAIL})


def _untouched(out, names=SUMMARY + DETAIL):
    return all((getattr(out, k) == SENTINEL).all() for k in names)


def _same(out, ref, what, names=SUMMARY + DETAIL):
    """every output is the checker's, element by element -- and so every byte was written: the buffers held SENTINEL"""
    for k in names:
        got, r = getattr(out, k), getattr(ref, k)
        assert got.dtype == r.dtype and got.shape == r.shape, (what, k, got.shape, r.shape)
        assert not (r == SENTINEL).any()
        assert np.array_equal(got, r), (what, k, np.argwhere(got != r)[:4].tolist())


def _both(torch, sm, sc, ref, what, **edited):
    """the device's outputs with the detail and without it against the checker's ``ref``; returns the detailed run's"""
    rc, msg, out = _raw(torch, sm, sc, **edited)
    assert rc == 0, msg
    _same(out, ref, what)
    rc, msg, lean = _raw(torch, sm, sc, detail=False, **edited)
    assert rc == 0, msg
    _same(lean, ref, (what, "no detail"), SUMMARY)
    assert _untouched(lean, DETAIL)
    return out


def _device_ties(torch, sm, sc, out, what):
    """both parents on the device.  Level by level: slice l of brake_first and stop, and first, are what fo_scene_hidden_brake_users gives
    at a_brake = levels[l] for b < B, commit[..., l] is its commit where that is < B, else -1.  Class by class: row c of required,
    last_unclear, commit and brake_first, and stop, are what fo_scene_hidden_brake_ladder gives on the arrival map behind the key map of
    class c (the first sample whose threshold the key lies within) with first[c]"""
    nb = sc.starts
    for n, a_brake in enumerate(sc.levels):
        rc, msg, one = UG._raw_users(torch, sm, sc.win, sc.r2_caps, sc.keys, sc.qmins, sc.x, sc.y, sc.head, sc.v, sc.arc, float(a_brake), sc.dt,
                                     sc.thr, sc.map_of, sc.lens)
        assert rc == 0, msg
        assert np.array_equal(out.brake_first[..., n], one.brake_first[:, :, :nb]), (what, n, "brake_first")
        assert np.array_equal(out.stop[..., n], one.stop[:, :nb]) and np.array_equal(out.first, one.first), (what, n, "stop, first")
        assert np.array_equal(out.commit[..., n], np.where(one.commit < nb, one.commit, -1)), (what, n, "commit")
    for c, k in enumerate(sc.map_of):
        A = S.arrival_of(sc.keys[k], sc.thr[c])
        r2 = np.arange(sc.T, dtype=np.int32)            # (any admissible table: the ladder's kernel reads the map, not the table)
        rc, msg, one = LG._raw_ladder(torch, sm, sc.win, r2, A, out.first[c], sc.x, sc.y, sc.head, sc.v, sc.arc, sc.levels, nb, sc.dt, sc.lens)
        assert rc == 0, msg
        for name in ("required", "last_unclear", "commit", "brake_first"):
            assert np.array_equal(getattr(out, name)[c], getattr(one, name)), (what, c, name)
        assert np.array_equal(out.stop, one.stop), (what, c, "stop")


# ------------------------------------------------------------------------------------------------ 1. the scenes
@pytest.mark.parametrize("spec", S.SCENES, ids=lambda s: "-".join(str(v) for v in s))
def test_scenes_at_the_plans_switch_points(torch_cuda, spec):
    """tests/hidden_brake_ladder_users_scenes.SCENES -- L in {1, 2, 5, 23, 33, 48, 64}, B in {1, T}, C in {1, 3, 4, 5, 8}, one to three maps,
    two maps in one buffer and a map nobody names, T in {2, 31, 33, 100, 254}, M in {1, 2, 3, 70}, ragged and full lengths, lanes on a part of
    a wave, on one, two and four waves -- with the detail and without it against the checker, and against both parents on the device"""
    torch = torch_cuda
    sm, road = _parked()
    sc, ref = S.checked(spec)
    assert np.array_equal(road, sc.road)
    out = _both(torch, sm, sc, ref, spec)
    _device_ties(torch, sm, sc, out, spec)


def test_the_level_clear_of_every_user_lies_above_every_users_own(torch_cuda):
    """tests/hidden_brake_ladder_users_scenes.hand_scene, whose rows tests/test_hidden_brake_ladder_users_cpu.py derives by hand: the
    device finds required_all = 2 above the users' own 0 and 1, blocked below by user 0 alone -- a maximum over per-user ladders would
    have said 1"""
    torch = torch_cuda
    sm, road = _parked()
    sc, ref = S.checked("hand")
    out = _both(torch, sm, sc, ref, "hand")
    assert out.required[:, 0, 0].tolist() == [0, 1] and out.required_all[0, 0] == 2 and out.blocking[0, 0] == 0b01
    assert len(LU.above_every_user(out, None, sc.T)) == 33
    _device_ties(torch, sm, sc, out, "hand")


def test_every_kind_of_answer_on_the_device(torch_cuda):
    """the kinds tests/test_hidden_brake_ladder_users_cpu.py asks of the scenes, counted on the DEVICE's outputs: an interior
    required_all, one of -1 with a manoeuvre, one of 0, a non-monotone pair, a pair above every user's own, pairs without a manoeuvre"""
    torch = torch_cuda
    sm, road = _parked()
    tot = {}
    for spec in S.SCENES[:2] + ["hand"]:
        sc, ref = S.checked(spec)
        rc, msg, out = _raw(torch, sm, sc)
        assert rc == 0, msg
        for k, n in LU.kinds(out, sc.lens, sc.T).items():
            tot[k] = tot.get(k, 0) + int(n)
    print(tot)
    assert tot["interior"] >= 20 and tot["none"] >= 20 and tot["zero"] >= 20 and tot["non_monotone"] >= 1 and tot["above"] >= 1 and tot["no_manoeuvre"] >= 1


# ------------------------------------------------------------------------------------------------ 2. edited inputs
def test_edited_inputs(torch_cuda):
    """what the kernel is handed as data may hold anything: (a) key maps and qmin arrays that are no clearance's -- random, negative,
    NONE everywhere, different on every map --, (b) NaN and infinities in v and arc, (c) an arc that is not monotone.  No index depends
    on any of it beyond the clamped segment index; every row is the checker's"""
    torch = torch_cuda
    sm, road = _parked()
    sc = copy.copy(S.scene(35, 12, 31, False, 5, "3", 5, 31))
    plain = _both(torch, sm, sc, S.check(sc), "plain")
    rng = np.random.default_rng(78)
    top = int(sc.thr.max())
    keys2, qmins2 = [], []
    for key, qmin in zip(sc.keys, sc.qmins):
        k2 = rng.integers(-5, 2 * top, key.shape).astype(np.int64)
        k2[rng.random(key.shape) < 0.3] = HC.NONE
        k2[rng.random(key.shape) < 0.02] = -2 ** 31
        q2 = rng.integers(-5, 2 * top, qmin.shape).astype(np.int64)
        q2[rng.random(qmin.shape) < 0.5] = HC.NONE
        keys2.append(k2)
        qmins2.append(q2)
    out = _both(torch, sm, sc, S.check(sc, keys=keys2, qmins=qmins2), "edited maps", keys=keys2, qmins=qmins2)
    assert (out.first != plain.first).any() and np.array_equal(out.stop, plain.stop)
    none = [np.full(k.shape, HC.NONE, dtype=np.int64) for k in sc.keys]
    qnone = [np.full(q.shape, HC.NONE, dtype=np.int64) for q in sc.qmins]
    out = _both(torch, sm, sc, S.check(sc, keys=none, qmins=qnone), "keys at NONE", keys=none, qmins=qnone)
    assert (out.first == -1).all() and (out.commit == -1).all() and (out.blocking == 0).all() and (out.last_unclear_all == -1).all()
    v, arc = sc.v.copy(), sc.arc.copy()
    v[4, :] = np.nan
    v[5, 3] = np.nan
    arc[7, 12] = np.nan
    arc[8, 0] = np.nan
    arc[9, 30] = np.nan
    v[10, 2], v[11, 2] = np.inf, -np.inf
    out = _both(torch, sm, sc, S.check(sc, v=v, arc=arc), "NaN", v=v, arc=arc)
    others = [m for m in range(sc.M) if m not in (4, 5, 7, 8, 9, 10, 11)]
    assert np.array_equal(out.required_all[others], plain.required_all[others]) and np.array_equal(out.first, plain.first)
    arc = sc.arc.copy()
    for m in range(0, sc.M, 3):
        arc[m] = rng.permutation(arc[m])
    arc[2, :] = arc[2, 7]
    _both(torch, sm, sc, S.check(sc, arc=arc), "non-monotone arc", arc=arc)
    _both(torch, sm, sc, S.check(sc, keys=keys2, qmins=qmins2, v=v, arc=arc), "everything edited", keys=keys2, qmins=qmins2, v=v, arc=arc)


# ------------------------------------------------------------------------------------------------ 3. through SensorModel
def test_every_level_and_every_user_through_the_sensor_model(torch_cuda):
    """scenario 1 after five steps with the occlusion memory on, through ``SensorModel``, mixed users on all three forecasts: ONE
    ``hidden_brake_ladder_users`` call against ``hidden_brake_users(a_brake=level)`` for every level, against
    ``hidden_brake_ladder(v_max=s_c, metric_c, flow_c)`` -- its own forecast, its arrival map from ``hidden_reach`` -- for every user,
    and against the checker on the clearances' own maps; a ``hidden_brake_users`` call before and after gives the same bits"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrakeLadderUsers
    sc = T._scenario("scenario1")
    sm, obs = T._sensor(sc, memory={})
    ego, yaw = T._drive(torch, sm, obs, sc, 5)
    # (the fan, the lengths and the users of tests/test_hidden_brake_users_gpu.py's drive, whose 6 m/s^2 is level 1 here: that test finds
    # candidates that are not fail-safe there, so some level is unclear here)
    traj = SY.make_trajectories(48, 31, T.DT, seed=20250701, ego_pos=ego, ego_yaw=yaw)
    lens = np.random.default_rng(5).integers(0, 33, 48).astype(np.int32)
    users = ((7.0, "road", "lanes"), (2.0, "road", "any"), (13.9, "road", "lanes"), (2.0, "euclid", "any"), (7.0, "road", "any"))
    levels = np.array([2.0, 6.0, 11.5])
    starts = 20
    kw = dict(vehicle=T.VEH, dt=T.DT, lengths=lens)
    args = (traj["x"], traj["y"], traj["theta"], traj["v"])
    snap = lambda r: [_np(getattr(r, k)).copy() for k in UG.OUTPUTS]
    before = snap(sm.hidden_brake_users(*args, users=users, a_brake=6.0, **kw))
    hblu = sm.hidden_brake_ladder_users(*args, users=users, decelerations=levels, starts=starts, detail=True, **kw)
    lean = sm.hidden_brake_ladder_users(*args, users=users, decelerations=levels, starts=starts, **kw)
    after = snap(sm.hidden_brake_users(*args, users=users, a_brake=6.0, **kw))
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert isinstance(hblu, HiddenBrakeLadderUsers) and hblu.users == users and hblu.map_of == (0, 1, 0, 2, 1)
    assert lean.brake_first is None and lean.stop is None and all(np.array_equal(_np(getattr(lean, k)), _np(getattr(hblu, k))) for k in SUMMARY)
    got = SimpleNamespace(**{k: _np(getattr(hblu, k)) for k in SUMMARY + DETAIL})
    # ... and those bits are the new result's slice of level 1
    assert np.array_equal(got.brake_first[..., 1], before[0][:, :, :starts]) and np.array_equal(got.stop[..., 1], before[1][:, :starts])
    assert np.array_equal(got.commit[..., 1], np.where(before[2] < starts, before[2], -1)) and np.array_equal(got.first, before[3])
    for n, a_brake in enumerate(levels):
        hbu = sm.hidden_brake_users(*args, users=users, a_brake=float(a_brake), **kw)
        bf, st, cm = hblu.level(n)
        assert np.array_equal(_np(bf), _np(hbu.brake_first)[:, :, :starts]) and np.array_equal(_np(st), _np(hbu.stop)[:, :starts]), n
        commit = _np(hbu.commit)
        assert np.array_equal(_np(cm), np.where(commit < starts, commit, -1)) and np.array_equal(got.first, _np(hbu.first)), n
    for c, (s_c, metric, flow) in enumerate(users):
        hbl = sm.hidden_brake_ladder(*args, v_max=s_c, decelerations=levels, starts=starts, metric=metric, flow=flow, **kw)
        for name in ("required", "last_unclear", "commit", "brake_first"):
            assert np.array_equal(getattr(got, name)[c], _np(getattr(hbl, name))), (c, name)
        assert np.array_equal(got.stop, _np(hbl.stop)) and np.array_equal(got.first[c], _np(hbl.reach.first)), c
        assert np.array_equal(_np(hblu.required_deceleration(c)), _np(hbl.required_deceleration()), equal_nan=True)
        assert np.array_equal(_np(hblu.monotone(c)), _np(hbl.monotone()))
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    ref = LU.ladder_users([_np(c.key) for c in hblu.clearances], win, road, [_np(c.qmin) for c in hblu.clearances], sm.raster_origin, sm.cell_size,
                          x, y, _np(hblu.clearances[0].heading), _np(hblu.arc), v, T.HL, T.HW, T.WB, levels, starts, T.DT, hblu.thr, hblu.map_of, lens)
    _same(got, ref, "scenario 1")
    print(LU.kinds(ref, lens, 31))
    assert hblu.required_deceleration().device.type == "cuda" and (got.last_unclear_all >= 0).any() and (got.required_all >= 0).any()
    mask = _np(hblu.blocking_users())
    assert np.array_equal(mask, (got.blocking[None] >> np.arange(5)[:, None, None] & 1) != 0)
    req = np.where(got.required_all >= 0, np.append(levels, np.inf)[got.required_all], np.inf)
    req = np.where((got.required_all < 0) & (got.last_unclear_all < 0), np.nan, req)
    assert np.array_equal(_np(hblu.required_deceleration()), req, equal_nan=True)
    assert np.array_equal(_np(hblu.brake_threat_number(11.5)), req / 11.5, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, road = _parked()
    lib = sm.ctx._lib
    key = np.zeros((9, 12), dtype=np.int32)
    x = np.zeros((2, 4))
    head = np.zeros((2, 4, 2))
    head[..., 0] = 1.0
    qmin = np.zeros((2, 4), dtype=np.int32)
    thr = [[0, 169, 169, 169 * 30], [5, 5, 5, 5]]
    base = SimpleNamespace(win=(3, 1, 12, 9), x=x, y=x, head=head, v=x, arc=x, lens=None, dt=0.1, keys=[key, key.copy()], qmins=[qmin, qmin.copy()],
                           thr=np.array(thr), map_of=(0, 1), r2_caps=(30, 40), levels=np.array([2.0, 4.0]), starts=3, T=4, M=2)

    def call(**kw):
        return _raw(torch, sm, base, **kw)

    rc, msg, out = call()
    assert rc == N.FO_OK and (out.commit == 0).all() and (out.first == 0).all() and (out.required_all == -1).all() and (out.blocking == 3).all(), msg
    assert (out.stop >= 0).all() and not (out.brake_first == SENTINEL).any()
    nan, inf = float("nan"), float("inf")
    ext = N.HIDDEN_REACH_MAX_HALF_EXTENT * sm.cell_size
    nine = [[1, 1, 1, 1]] * 9
    refused = [
        (dict(K=0), "K = 0 outside [1, FO_HIDDEN_BRAKE_MAX_MAPS = 3]"), (dict(K=4), "K = 4 outside"), (dict(K=-1), "K = -1 outside"),
        (dict(C=0), "C = 0 outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = 8]"), (dict(C=9), "C = 9"), (dict(table=nine, map_of=(0,) * 9), "C = 9"),
        (dict(drop=("h_thr",)), "h_thr"),
        (dict(map_of=(0, 2)), "map_of[1] = 2 outside [0, K = 2)"), (dict(map_of=(-1, 0)), "map_of[0] = -1 outside [0, K = 2)"),
        (dict(map_of=(0, 1), K=1), "map_of[1] = 1 outside [0, K = 1)"),
        (dict(table=[[0, 9, 8, 30], [5, 5, 5, 5]]), "h_thr[0] decreases at entry 2"), (dict(table=[thr[0], [-1, 5, 5, 5]]), "h_thr[1][0] = -1 is negative"),
        (dict(table=[[0, 1, 2, 169 * 30 + 1], thr[1]]), "h_thr[0][T-1] = 5071 lies beyond 169 r2_cap[0] = 5070"),
        (dict(r2_caps=(30, -1)), "r2_cap[1] = -1 is negative"),
        (dict(r2_caps=(30, (N.HIDDEN_REACH_MAX_HALO + 1) ** 2)), "r2_cap[1] = 65025 is a reach of more than FO_HIDDEN_REACH_MAX_HALO"),
        (dict(M=-1), "M = -1"), (dict(T=0), "T = 0"), (dict(T=255), "T = 255"),
        (dict(L=0), "L = 0 outside [1, FO_HIDDEN_BRAKE_MAX_LEVELS = 64]"), (dict(L=65), "L = 65 outside"), (dict(L=-1), "L = -1 outside"),
        (dict(drop=("h_levels",)), "no decelerations h_levels"),
        (dict(levels=[2.0, -0.5]), "h_levels[1] = -0.5"), (dict(levels=[nan, 1.0]), "h_levels[0] = nan"), (dict(levels=[1.0, inf]), "h_levels[1] = inf"),
        (dict(B=0), "B = 0 outside [1, T = 4]"), (dict(B=5), "B = 5 outside [1, T = 4]"), (dict(B=-3), "B = -3 outside"),
        (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"), (dict(dt=nan), "dt"), (dict(dt=inf), "dt"),
        (dict(drop_map=(("d_key", 0),)), "d_key[0]"), (dict(drop_map=(("d_key", 1),)), "d_key[1]"), (dict(drop_map=(("d_qmin", 1),)), "d_qmin[1]"),
        (dict(drop=("d_x",)), "d_x"), (dict(drop=("d_y",)), "d_x"), (dict(drop=("d_heading",)), "d_heading"),
        (dict(drop=("d_v",)), "d_v"), (dict(drop=("d_arc",)), "d_arc"),
        (dict(drop=("d_required",)), "d_required"), (dict(drop=("d_last_unclear",)), "d_last_unclear"), (dict(drop=("d_commit",)), "d_commit"),
        (dict(drop=("d_first",)), "d_first"), (dict(drop=("d_required_all",)), "d_required_all"), (dict(drop=("d_last_unclear_all",)), "d_last_unclear_all"),
        (dict(drop=("d_blocking",)), "d_blocking"),
        (dict(drop=("d_stop_or_null",)), "given whole or not at all (d_stop_or_null is missing)"),
        (dict(drop=("d_brake_first_or_null",)), "given whole or not at all (d_brake_first_or_null is missing)"),
        (dict(win_nx=0), "window"), (dict(win_ny=40000), "window"),
        (dict(hl=-0.1), "half extents"), (dict(hw=nan), "half extents"), (dict(wb=ext * 1.01), "half extents"),
    ]
    for kw, text in refused:
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_ladder_users:") and text in msg, (kw, rc, msg)
        assert _untouched(out), kw
    # the order: the table's size before the budget, the budget before the rows (tables of the size the call states, rows that decrease)
    big = np.ones((8, 254), dtype=np.int32)
    big[:, 0] = 9
    full_ladder = np.linspace(0.0, 6.3, 64)
    rc, msg, out = call(levels=full_ladder, T=254, table=big[:4], map_of=(0, 1, 0, 1))
    assert rc == N.FO_E_ARG and "C * T = 4 * 254 = 1016 entries" in msg and _untouched(out)
    rc, msg, out = call(levels=full_ladder, T=110, table=np.ascontiguousarray(big[:, :110]), map_of=(0,) * 8)
    assert rc == N.FO_E_ARG and _untouched(out)
    assert "880 thresholds (C * T = 8 * 110) and 64 levels take 4 * 880 + 8 * 64 = 4032 bytes" in msg and "FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES = 3584" in msg
    rc, msg, out = call(levels=full_ladder, T=254, table=big[:3], map_of=(0, 1, 0))         # 3 048 + 512 bytes fit: the rows are looked at
    assert rc == N.FO_E_ARG and "h_thr[0] decreases at entry 1 (1 after 9)" in msg and _untouched(out)
    # what lies beyond K, C and L is not looked at
    rc, msg, out = call()
    assert rc == N.FO_OK and not _untouched(out), msg
    # M = 0: fine, and nothing is written
    empty = copy.copy(base)
    empty.x = empty.y = empty.v = empty.arc = np.zeros((0, 4))
    empty.head, empty.qmins = np.zeros((0, 4, 2)), [qmin[:0], qmin[:0].copy()]
    rc, msg, out = _raw(torch, sm, empty)
    assert rc == N.FO_OK, msg
    # no parameters, and a context without a map
    assert lib.fo_scene_hidden_brake_ladder_users(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert lib.fo_scene_hidden_brake_ladder_users(ctx._h, C.byref(N.HiddenBrakeLadderUsers()), None) == N.FO_E_STATE
    assert N.load().fo_abi_version() == 12
    # the host layer refuses before any device work
    with pytest.raises(ValueError, match="at most 3584 are possible"):
        sm.hidden_brake_ladder_users(np.zeros((2, 110)), np.zeros((2, 110)), np.zeros((2, 110)), np.zeros((2, 110)), vehicle=SC.VEH,
                                     users=((1.0, "road", "any"),) * 8, dt=SC.DT, decelerations=np.linspace(0.0, 6.3, 64))


# ------------------------------------------------------------------------------------------------ 5. through the interface
def test_interface_defaults_and_independence(torch_cuda, tmp_path):
    """``FOInterface.hidden_brake_ladder_users`` with its defaults against the checker; ``hidden_brake_users`` and the other
    hidden-traffic entries give the same bits before the call and after it, and the level of ``a_max`` is ``hidden_brake_users``'
    default call"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrakeLadderUsers
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    traj = SY.make_trajectories(8, 31, T.DT, seed=3, ego_pos=np.asarray(sc.ego_initial)[:2], ego_yaw=float(sc.ego_initial[2]))
    users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
    with pytest.raises(RuntimeError, match="hidden_brake_ladder_users needs a previous evaluate_scenario"):
        fo.hidden_brake_ladder_users(traj, users)
    ego, yaw = WG._drive(fo, sc, 2)
    traj = SY.make_trajectories(8, 31, T.DT, seed=3, ego_pos=ego, ego_yaw=yaw)

    def others():
        u = fo.hidden_brake_users(traj, users)
        r = fo.hidden_reach(traj, v_max=7.0, metric="road", flow="lanes")
        b = fo.hidden_brake_ladder(traj, v_max=7.0, metric="road", flow="lanes", starts=5)
        parts = [u.brake_first, u.stop, u.commit, u.first, r.arrival, r.first, b.required, b.last_unclear, b.commit]
        return [_np(p).copy() for p in parts]

    before = others()
    hblu = fo.hidden_brake_ladder_users(traj, users, detail=True)
    after = others()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
    assert isinstance(hblu, HiddenBrakeLadderUsers) and hblu.dt == T.DT and hblu.map_of == (0, 1, 1)
    assert hblu.decelerations.tolist() == [0.5 * k for k in range(1, 24)] and SY.VEHICLE_BMW320I[4] == 11.5
    bf, st, cm = hblu.level(22)                                   # a_max: hidden_brake_users' default deceleration
    assert np.array_equal(_np(bf), before[0]) and np.array_equal(_np(st), before[1]) and np.array_equal(_np(cm), before[2])
    assert np.array_equal(_np(hblu.first), before[3])
    sm = fo.sensor_model
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    ref = LU.ladder_users([_np(c.key) for c in hblu.clearances], win, road, [_np(c.qmin) for c in hblu.clearances], sm.raster_origin, sm.cell_size,
                          x, y, _np(hblu.clearances[0].heading), _np(hblu.arc), v, T.HL, T.HW, T.WB, hblu.decelerations, 31, T.DT, hblu.thr, hblu.map_of)
    _same(SimpleNamespace(**{k: _np(getattr(hblu, k)) for k in SUMMARY + DETAIL}), ref, "interface")
    lean = fo.hidden_brake_ladder_users(traj, users, starts=5)
    assert lean.brake_first is None and np.array_equal(_np(lean.required_all), _np(hblu.required_all)[:, :5])
