"""Hidden-traffic brake clearance by road users on the device (fo_scene_hidden_brake_users, DESIGN.md §5.10 "Brake clearance by road
users") against the plain statement of the definition (tests/ref_hidden_brake_users.py) and, user by user, against
fo_scene_hidden_brake_classes and fo_scene_hidden_brake of the same library on the same device state.  On the seeded scenes the key
maps and qmin arrays are the clearance checkers' and are handed straight to the entry; the checker is handed what the device was
handed.  Every output is an exact integer: all comparisons are ``==``.  Every test runs under a time limit of its own that ends the
process (a hung kernel cannot be waited out from Python); no test provokes a fault."""
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
import ref_hidden_brake_users as BU
import ref_hidden_clearance as HC
import test_hidden_brake_gpu as BG
import test_hidden_reach_flow_gpu as FG
import test_hidden_reach_gpu as T
import test_hidden_witness_gpu as WG
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
OUTPUTS = ("brake_first", "stop", "commit", "first")
_parked = BG._parked
STEP_LIMIT = 240          # seconds a test may take before the process is ended with every thread's traceback
TRACE_LIMIT = 200         # ... and a traced child process of the last test; that test starts two of them


@pytest.fixture(autouse=True)
def _time_limit(request):
    """the one timer of this file: STEP_LIMIT, or the module attribute ``<test name>_limit`` where a test has one"""
    faulthandler.dump_traceback_later(getattr(request.module, request.function.__name__ + "_limit", STEP_LIMIT), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw_users(torch, sm, win, r2_caps, keys, qmins, x, y, head, v, arc, a_brake, dt, thr, map_of, lens=None, hl=HL, hw=HW, wb=WB, drop=(),
               drop_map=(), **over):
    """fo_scene_hidden_brake_users on maps and trajectories of the test's own; the output buffers are pre-filled with a pattern.
    ``drop``: names of pointers to hand over as NULL; ``drop_map``: (name, k) entries of d_key / d_qmin to hand over as NULL; ``over``:
    fields of the structure to replace.  Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    M, Tn = x.shape
    thr = np.ascontiguousarray(thr, dtype=np.int32)
    Cn, Kn = thr.shape[0], len(keys)
    tx, ty, th, tv, ta = (up(a, np.float64) for a in (x, y, head, v, arc))
    dk, dq, tl = [up(k, np.int32) for k in keys], [up(q, np.int32) for q in qmins], up(lens, np.int32)
    out = SimpleNamespace(brake_first=torch.full((Cn, M, Tn), -7, dtype=torch.int32, device=dev),
                          stop=torch.full((M, Tn), -7, dtype=torch.int32, device=dev),
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
              d_v=p(tv), d_arc=p(ta), a_brake=float(a_brake), dt=float(dt), h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)),
              d_brake_first=p(out.brake_first), d_stop=p(out.stop), d_commit=p(out.commit), d_first=p(out.first))
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeUsers(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_users(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(**{k: _np(getattr(out, k)) for k in OUTPUTS})


def _untouched(out):
    return all((getattr(out, k) == -7).all() for k in OUTPUTS)


def _same(out, ref, what):
    for k, r in zip(OUTPUTS, ref):
        got = getattr(out, k)
        assert got.dtype == r.dtype and got.shape == r.shape, (what, k, got.shape, r.shape)
        assert np.array_equal(got, r), (what, k, np.argwhere(got != r)[:4].tolist())


def _both(torch, sm, road, sc, what, keys=None, qmins=None, thr=None, map_of=None, r2_caps=None, a_brake=None, v=None, arc=None):
    """the device's outputs and the checker's on the same data; asserts that they are equal and returns the device's"""
    pick = lambda given, own: getattr(sc, own) if given is None else given
    keys, qmins, thr, map_of = pick(keys, "keys"), pick(qmins, "qmins"), pick(thr, "thr"), pick(map_of, "map_of")
    r2_caps, a_brake, v, arc = pick(r2_caps, "r2_caps"), pick(a_brake, "a_brake"), pick(v, "v"), pick(arc, "arc")
    rc, msg, out = _raw_users(torch, sm, sc.win, r2_caps, keys, qmins, sc.x, sc.y, sc.head, v, arc, a_brake, sc.dt, thr, map_of, sc.lens)
    assert rc == 0, msg
    ref = BU.brake_users(keys, sc.win, road, qmins, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, arc, v, HL, HW, WB, a_brake, sc.dt, thr, map_of, sc.lens)
    _same(out, ref, what)
    return out


_scenes = {}


def _scene(spec, users=US.USERS):
    """the scene with its maps by the checkers, computed once per (spec, users) and never changed"""
    if (spec, users) not in _scenes:
        _scenes[spec, users] = US.user_scene(spec, users)
    return _scenes[spec, users]


# ------------------------------------------------------------------------------------------------ 1. the random scenes
# T = 3 is not among tests/hidden_brake_scenes.RANDOM_SCENES (G = 4, 64 trajectories per workgroup), nor are the edges of the workgroup
# at T = 254 (4 per workgroup) -- the largest LDS a call can ask for: three maps and as many classes as 896 entries leave, 64 008 bytes
EXTRA = [(91, 63, 3, 0, True), (92, 64, 3, 1, False), (93, 65, 3, 2, True), (82, 3, 254, 0, True), (83, 4, 254, 2, False), (84, 5, 254, 1, False)]
THREE = (US.USERS[0], US.USERS[3], US.USERS[4])      # one user per map: T = 254 leaves room for three


@pytest.mark.parametrize("T_", [1, 2, 3, 31, 32, 33, 64, 65, 254])
def test_random_scenes_three_maps(torch_cuda, T_):
    """tests/hidden_brake_scenes.RANDOM_SCENES and the six scenes above, five users on three maps (three at T = 254): T in {1, 2, 3, 31,
    32, 33, 64, 65, 254}, M on both sides of every trajectories-per-workgroup edge, ragged lengths with 0, 1, 2, negative ones and ones
    beyond T, windows over the whole road, a part of it and the raster's corner"""
    torch = torch_cuda
    sm, road = _parked()
    specs = [s for s in SC.RANDOM_SCENES + EXTRA if s[2] == T_]
    per = 256 // min(64, 1 << max(T_ - 1, 0).bit_length())
    assert {s[1] for s in specs} >= {per - 1, per, per + 1} and any(s[4] for s in specs)
    hits = 0
    for spec in specs:
        sc = _scene(spec, THREE if T_ == 254 else US.USERS)
        assert len(sc.keys) == 3
        out = _both(torch, sm, road, sc, spec)
        hits += int((out.brake_first >= 0).sum()) + int((out.first >= 0).sum())
    assert hits > 0


def test_the_forecasts_are_told_apart(torch_cuda):
    """the scenes in which, by the checker (tests/test_hidden_brake_users_cpu.py), the same 4 m/s has different rows along the lanes,
    along the road and as the crow flies: the device has them too, and every kind of commit"""
    torch = torch_cuda
    sm, road = _parked()
    out = _both(torch, sm, road, _scene((31, 7, 31, 2, False)), "scene 31")
    assert (out.commit[1] != out.commit[2]).any() and (out.brake_first[1] != out.brake_first[2]).any()
    assert (out.commit[2] != out.commit[3]).any() and (out.brake_first[2] != out.brake_first[3]).any()
    out = _both(torch, sm, road, _scene((35, 70, 31, 1, True)), "scene 35")
    assert (out.commit[1] != out.commit[2]).sum() >= 10
    assert (out.commit == -1).any() and (out.commit == 0).any() and (out.commit > 0).any()


def test_ragged_lengths(torch_cuda):
    """lengths of 0, 1, 2, T - 1, T, beyond T and negative, written down: the maps and the clearances are the checkers' for these very
    lengths; rows beyond a trajectory's length are -1 in brake_first and stop"""
    import copy
    torch = torch_cuda
    sm, road = _parked()
    sc = copy.copy(_scene((33, 9, 31, 1, False)))
    sc.lens = np.array([0, 1, 2, 30, 31, 32, 1000, -1, -2 ** 31], dtype=np.int32)
    sc.qmins = [US.forecast_maps(sc, f, cap)[1] for f, cap in zip(sc.maps, sc.r2_caps)]
    out = _both(torch, sm, road, sc, "ragged")
    for m, n in enumerate([0, 1, 2, 30, 31, 31, 31, 0, 0]):
        assert (out.brake_first[:, m, max(n - 1, 0):] == -1).all() and (out.stop[m, n:] == -1).all() and (out.stop[m, :n] >= 0).all(), m
    assert (out.commit[:, [0, 7, 8]] == -1).all() and (out.first[:, [0, 7, 8]] == -1).all() and (out.brake_first >= 0).any()


# ------------------------------------------------------------------------------------------------ 2. class counts, map counts, map_of
SPEEDS8 = (8.0, 1.5, 0.0, 4.0, 4.0, 6.5, 0.25, 2.0)
_maps8 = {}


def _three_maps(spec=(35, 24, 31, 1, True)):
    """(scene, keys [3], qmins [3]) -- the three forecasts of one scene at the cap of the fastest of SPEEDS8, so that every class may be
    put on every map"""
    if spec not in _maps8:
        sc = US.user_scene(spec, tuple((s, "road", "any") for s in SPEEDS8), maps=False)
        cap = sc.r2_caps[0]
        made = [US.forecast_maps(sc, f, cap) for f in (("road", "lanes"), ("euclid", "any"), ("road", "any"))]
        _maps8[spec] = (sc, [m[0] for m in made], [m[1] for m in made], cap)
    return _maps8[spec]


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C_", [1, 2, 3, 4, 5, 6, 7, 8])
def test_class_and_map_counts(torch_cuda, C_, K):
    """C = 1 .. 8 against K = 1 .. 3: all six instantiations (4 or 8 classes wide, one to three maps), widths with classes that are not
    there, unsorted and repeated speeds, a motionless class; class c on map (c + 1) % K, so that with C < K a map goes unnamed.  With
    K = 1 the whole result is fo_scene_hidden_brake_classes' on the same inputs; the row of a class is the same whatever else is asked"""
    torch = torch_cuda
    sm, road = _parked()
    sc, keys, qmins, cap = _three_maps()
    map_of = [(c + 1) % K for c in range(C_)]
    out = _both(torch, sm, road, sc, (C_, K), keys=keys[:K], qmins=qmins[:K], thr=sc.thr[:C_], map_of=map_of, r2_caps=[cap] * K)
    assert out.brake_first.shape == (C_, 24, 31) and (out.brake_first >= 0).any() and (out.commit < 0).any()
    import test_hidden_brake_classes_gpu as CG
    for c in (0, C_ - 1):
        k = map_of[c]
        rc, msg, alone = CG._raw_classes(torch, sm, sc.win, cap, keys[k], qmins[k], sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt,
                                         sc.thr[c:c + 1], sc.lens)
        assert rc == 0, msg
        assert np.array_equal(alone.brake_first[0], out.brake_first[c]) and np.array_equal(alone.commit[0], out.commit[c])
        assert np.array_equal(alone.first[0], out.first[c]) and np.array_equal(alone.stop, out.stop)
    if K == 1:
        rc, msg, whole = CG._raw_classes(torch, sm, sc.win, cap, keys[0], qmins[0], sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt,
                                         sc.thr[:C_], sc.lens)
        assert rc == 0, msg
        assert all(np.array_equal(getattr(whole, k), getattr(out, k)) for k in OUTPUTS)


def test_map_of_permutations_and_an_unused_map(torch_cuda):
    """the same three users with the maps handed over in every order and map_of turned with them: the same rows; (1, 0, 1) and a map in
    the middle that no class names (its pointers are valid: "not read" is not tested by a fault)"""
    import itertools
    torch = torch_cuda
    sm, road = _parked()
    sc, keys, qmins, cap = _three_maps()
    thr = sc.thr[[0, 3, 5]]
    base = _both(torch, sm, road, sc, "identity", keys=keys, qmins=qmins, thr=thr, map_of=[0, 1, 2], r2_caps=[cap] * 3)
    assert (base.brake_first[0] != base.brake_first[1]).any() or (base.commit[0] != base.commit[1]).any()
    for order in itertools.permutations(range(3)):
        out = _both(torch, sm, road, sc, order, keys=[keys[k] for k in order], qmins=[qmins[k] for k in order], thr=thr,
                    map_of=[order.index(c) for c in range(3)], r2_caps=[cap] * 3)
        assert all(np.array_equal(getattr(out, k), getattr(base, k)) for k in OUTPUTS), order
    one = _both(torch, sm, road, sc, "(1, 0, 1)", keys=keys[:2], qmins=qmins[:2], thr=thr, map_of=[1, 0, 1], r2_caps=[cap] * 2)
    gap = _both(torch, sm, road, sc, "(2, 0, 2)", keys=[keys[0], keys[2], keys[1]], qmins=[qmins[0], qmins[2], qmins[1]], thr=thr, map_of=[2, 0, 2],
                r2_caps=[cap] * 3)
    assert all(np.array_equal(getattr(one, k), getattr(gap, k)) for k in OUTPUTS)


def test_table_of_exactly_896_entries(torch_cuda):
    """C = 8, T = 112, three maps: the table fills the kernel argument to its last entry; 8 x 113 is refused"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    sc, keys, qmins, cap = _three_maps((118, 5, 112, 2, True))
    assert sc.thr.size == 896
    map_of = [2, 0, 1, 1, 0, 2, 2, 0]
    out = _both(torch, sm, road, sc, "896", keys=keys, qmins=qmins, thr=sc.thr, map_of=map_of, r2_caps=[cap] * 3)
    assert (out.brake_first >= 0).any() and (out.stop >= 0).any()
    sc, keys, qmins, cap = _three_maps((98, 3, 113, 0, False))
    rc, msg, out = _raw_users(torch, sm, sc.win, [cap] * 3, keys, qmins, sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt, sc.thr, map_of, sc.lens)
    assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_users: C * T = 8 * 113 = 904") and "FO_HIDDEN_BRAKE_MAX_TABLE = 896" in msg
    assert _untouched(out)


# ------------------------------------------------------------------------------------------------ 3. edited inputs
def test_edited_inputs(torch_cuda):
    """what the kernel is handed as data may hold anything: (a) key maps and qmin arrays that are no clearance's -- random, negative,
    NONE, values above every threshold, different on every map --, (b) NaN and infinities in v and arc, (c) an arc that is not monotone.
    No index depends on any of it beyond the clamped segment index; every row is the checker's"""
    torch = torch_cuda
    sm, road = _parked()
    sc = _scene((35, 70, 31, 1, True))
    M = sc.M
    plain = _both(torch, sm, road, sc, "plain")
    rng = np.random.default_rng(78)
    top = int(sc.thr.max())
    keys2, qmins2 = [], []
    for key, qmin in zip(sc.keys, sc.qmins):
        k2 = rng.integers(-5, 2 * top, key.shape).astype(np.int32)
        k2[rng.random(key.shape) < 0.3] = HC.NONE
        k2[rng.random(key.shape) < 0.02] = -2 ** 31
        q2 = rng.integers(-5, 2 * top, qmin.shape).astype(np.int32)
        q2[rng.random(qmin.shape) < 0.5] = HC.NONE
        keys2.append(k2)
        qmins2.append(q2)
    out = _both(torch, sm, road, sc, "edited maps", keys=keys2, qmins=qmins2)
    assert (out.first != plain.first).any() and np.array_equal(out.stop, plain.stop)
    assert (out.brake_first[1] != out.brake_first[2]).any()          # (the same speed on two random maps)
    v, arc = sc.v.copy(), sc.arc.copy()
    v[4, :] = np.nan
    v[5, 3] = np.nan
    arc[7, 12] = np.nan
    arc[8, 0] = np.nan
    arc[9, 30] = np.nan
    v[10, 2], v[11, 2] = np.inf, -np.inf
    out = _both(torch, sm, road, sc, "NaN", v=v, arc=arc)
    others = [m for m in range(M) if m not in (4, 5, 7, 8, 9, 10, 11)]
    for k in ("brake_first", "commit", "first"):
        assert np.array_equal(getattr(out, k)[:, others], getattr(plain, k)[:, others]), k
    assert np.array_equal(out.stop[others], plain.stop[others]) and np.array_equal(out.first, plain.first)
    arc = sc.arc.copy()
    for m in range(0, M, 3):
        arc[m] = rng.permutation(arc[m])
    arc[2, :] = arc[2, 7]
    _both(torch, sm, road, sc, "non-monotone arc", arc=arc)
    _both(torch, sm, road, sc, "everything edited", keys=keys2, qmins=qmins2, v=v, arc=arc, a_brake=0.5)


# ------------------------------------------------------------------------------------------------ 4. through SensorModel
def test_every_user_equals_its_own_forecast(torch_cuda):
    """scenario 1 after five steps with the occlusion memory on, the bench's fan, through ``SensorModel``, mixed users on all three
    forecasts: row c of every output of ONE ``hidden_brake_users`` call equals, bit for bit, ``hidden_brake_classes(speeds=(s_c,),
    metric_c, flow_c)`` and ``hidden_brake(v_max=s_c, metric_c, flow_c)`` -- their forecasts, their walks -- and the checker on the
    clearances' own maps"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrakeUsers
    sc = T._scenario("scenario1")
    sm, obs = T._sensor(sc, memory={})
    ego, yaw = T._drive(torch, sm, obs, sc, 5)
    traj = SY.make_trajectories(48, 31, T.DT, seed=20250701, ego_pos=ego, ego_yaw=yaw)
    lens = np.random.default_rng(5).integers(0, 33, 48).astype(np.int32)
    users = ((7.0, "road", "lanes"), (2.0, "road", "any"), (13.9, "road", "lanes"), (2.0, "euclid", "any"), (7.0, "road", "any"))
    kw = dict(vehicle=T.VEH, dt=T.DT, a_brake=6.0, lengths=lens)
    hbu = sm.hidden_brake_users(traj["x"], traj["y"], traj["theta"], traj["v"], users=users, **kw)
    assert isinstance(hbu, HiddenBrakeUsers) and hbu.users == users and hbu.map_of == (0, 1, 0, 2, 1)
    assert [(c.metric, c.flow) for c in hbu.clearances] == [("road", "lanes"), ("road", "any"), ("euclid", "any")]
    assert all(c.from_memory and c.heading is hbu.clearances[0].heading for c in hbu.clearances)
    assert [int(hbu.thr[c].max()) for c in (2, 4, 3)] == [169 * c.r2_cap for c in hbu.clearances]
    got = SimpleNamespace(**{k: _np(getattr(hbu, k)) for k in OUTPUTS})
    for c, (s_c, metric, flow) in enumerate(users):
        hbc = sm.hidden_brake_classes(traj["x"], traj["y"], traj["theta"], traj["v"], speeds=(s_c,), metric=metric, flow=flow, **kw)
        hb = sm.hidden_brake(traj["x"], traj["y"], traj["theta"], traj["v"], v_max=s_c, metric=metric, flow=flow, **kw)
        assert np.array_equal(hbu.thr[c], hbc.thr[0]) and np.array_equal(hbu.thr[c].astype(np.int64), 169 * hb.reach.r2.astype(np.int64))
        for one, first in ((SimpleNamespace(brake_first=hbc.brake_first[0], commit=hbc.commit[0], stop=hbc.stop), hbc.first[0]), (hb, hb.reach.first)):
            assert np.array_equal(got.brake_first[c], _np(one.brake_first)), (c, "brake_first")
            assert np.array_equal(got.stop, _np(one.stop)), (c, "stop")
            assert np.array_equal(got.commit[c], _np(one.commit)), (c, "commit")
            assert np.array_equal(got.first[c], _np(first)), (c, "first")
        assert np.array_equal(_np(hbu.arc), _np(hb.arc))
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    ref = BU.brake_users([_np(c.key) for c in hbu.clearances], win, road, [_np(c.qmin) for c in hbu.clearances], sm.raster_origin, sm.cell_size,
                         x, y, _np(hbu.clearances[0].heading), _np(hbu.arc), v, T.HL, T.HW, T.WB, 6.0, T.DT, hbu.thr, hbu.map_of, lens)
    _same(got, ref, "scenario 1")
    print("commit >= 0 per user:", (got.commit >= 0).sum(axis=1).tolist())
    assert (got.brake_first >= 0).any() and (got.commit[0] != got.commit[4]).any()      # 7 m/s along the lanes and along the road
    cu = _np(hbu.critical_user())
    speeds = np.asarray([u[0] for u in users])
    rank = np.lexsort((np.arange(5), speeds))                                            # by speed, the lower index first
    want = np.array([next((int(c) for c in rank if got.commit[c, m] >= 0), -1) for m in range(48)])
    assert hbu.critical_user().device.type == "cuda" and np.array_equal(cu, want)
    assert np.array_equal(_np(hbu.critical_speed()), np.where(want >= 0, speeds[np.maximum(want, 0)], np.inf))
    assert np.array_equal(_np(hbu.decided_until()), _np(hb.decided_until()))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, road = _parked()
    lib = sm.ctx._lib
    win = (3, 1, 12, 9)
    key = np.zeros((9, 12), dtype=np.int32)
    x = np.zeros((2, 4))
    head = np.zeros((2, 4, 2))
    head[..., 0] = 1.0
    qmin = np.zeros((2, 4), dtype=np.int32)
    thr = [[0, 169, 169, 169 * 30], [5, 5, 5, 5]]

    def call(table=thr, a_brake=4.0, dt=0.1, r2_caps=(30, 40), map_of=(0, 1), n_maps=2, **kw):
        return _raw_users(torch, sm, win, r2_caps, [key] * n_maps, [qmin] * n_maps, x, x, head, x, x, a_brake, dt, np.array(table, dtype=np.int32),
                          map_of, **kw)

    rc, msg, out = call()
    assert rc == N.FO_OK and (out.commit == 0).all() and (out.first == 0).all() and (out.stop >= 0).all(), msg
    nan, inf = float("nan"), float("inf")
    ext = N.HIDDEN_REACH_MAX_HALF_EXTENT * sm.cell_size
    nine = [[1, 1, 1, 1]] * 9
    refused = [
        (dict(K=0), "K = 0 outside [1, FO_HIDDEN_BRAKE_MAX_MAPS = 3]"), (dict(K=4), "K = 4 outside"), (dict(K=-1), "K = -1 outside"),
        (dict(C=0), "C = 0 outside [1, FO_HIDDEN_BRAKE_MAX_CLASSES = 8]"), (dict(C=9), "C = 9"), (dict(table=nine, map_of=(0,) * 9), "C = 9"),
        (dict(C=-1), "C = -1"),
        (dict(drop=("h_thr",)), "h_thr"),
        (dict(map_of=(0, 2)), "map_of[1] = 2 outside [0, K = 2)"), (dict(map_of=(-1, 0)), "map_of[0] = -1 outside [0, K = 2)"),
        (dict(map_of=(0, 1), K=1), "map_of[1] = 1 outside [0, K = 1)"),
        (dict(table=[[0, 9, 8, 30], [5, 5, 5, 5]]), "h_thr[0] decreases at entry 2"), (dict(table=[thr[0], [5, 5, 5, 4]]), "h_thr[1] decreases at entry 3"),
        (dict(table=[thr[0], [-1, 5, 5, 5]]), "h_thr[1][0] = -1 is negative"),
        (dict(table=[[0, 1, 2, 169 * 30 + 1], thr[1]]), "h_thr[0][T-1] = 5071 lies beyond 169 r2_cap[0] = 5070"),
        (dict(r2_caps=(29, 40)), "beyond 169 r2_cap[0] = 4901"),
        (dict(table=[thr[1], [0, 1, 2, 169 * 40 + 1]]), "h_thr[1][T-1] = 6761 lies beyond 169 r2_cap[1] = 6760"),
        (dict(table=[thr[1], [0, 1, 2, 169 * 40]], map_of=(1, 0)), "h_thr[1][T-1] = 6760 lies beyond 169 r2_cap[0] = 5070"),
        (dict(r2_caps=(30, -1)), "r2_cap[1] = -1 is negative"), (dict(r2_caps=((N.HIDDEN_REACH_MAX_HALO + 1) ** 2, 40)), "r2_cap[0] = 65025 is a reach of more than FO_HIDDEN_REACH_MAX_HALO"),
        (dict(r2_caps=(30, (N.HIDDEN_REACH_MAX_HALO + 1) ** 2)), "r2_cap[1] = 65025 is a reach of more than FO_HIDDEN_REACH_MAX_HALO"),
        (dict(M=-1), "M = -1"), (dict(T=0), "T = 0"), (dict(T=255), "T = 255"), (dict(T=449), "T = 449"),
        (dict(a_brake=-0.5), "a_brake"), (dict(a_brake=nan), "a_brake"), (dict(a_brake=inf), "a_brake"),
        (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"), (dict(dt=nan), "dt"), (dict(dt=inf), "dt"),
        (dict(drop_map=(("d_key", 0),)), "d_key[0]"), (dict(drop_map=(("d_key", 1),)), "d_key[1]"), (dict(drop_map=(("d_qmin", 1),)), "d_qmin[1]"),
        (dict(drop=("d_x",)), "d_x"), (dict(drop=("d_y",)), "d_x"), (dict(drop=("d_heading",)), "d_heading"),
        (dict(drop=("d_v",)), "d_v"), (dict(drop=("d_arc",)), "d_arc"),
        (dict(drop=("d_brake_first",)), "d_brake_first"), (dict(drop=("d_stop",)), "d_stop"), (dict(drop=("d_commit",)), "d_commit"),
        (dict(drop=("d_first",)), "d_first"),
        (dict(win_nx=0), "window"), (dict(win_ny=40000), "window"),
        (dict(hl=-0.1), "half extents"), (dict(hw=nan), "half extents"), (dict(wb=ext * 1.01), "half extents"),
    ]
    for kw, text in refused:
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_users:") and text in msg, (kw, rc, msg)
        assert _untouched(out), kw
    # what lies beyond K and beyond C is not looked at: the third map's pointers are NULL, its cap and map_of[2 ..] are nonsense
    rc, msg, out = call()
    assert rc == N.FO_OK and not _untouched(out), msg
    # M = 0: fine, and nothing is written; the lengths are optional
    e = np.zeros((0, 4))
    rc, msg, out = _raw_users(torch, sm, win, (30, 40), [key] * 2, [qmin[:0]] * 2, e, e, np.zeros((0, 4, 2)), e, e, 4.0, 0.1, np.array(thr, dtype=np.int32), (0, 1))
    assert rc == N.FO_OK, msg
    # no parameters, and a context without a map
    assert lib.fo_scene_hidden_brake_users(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert lib.fo_scene_hidden_brake_users(ctx._h, C.byref(N.HiddenBrakeUsers()), None) == N.FO_E_STATE
    assert N.load().fo_abi_version() == 12
    # the host layer refuses before any device work
    with pytest.raises(ValueError, match="at most 896 are possible"):
        sm.hidden_brake_users(np.zeros((2, 113)), np.zeros((2, 113)), np.zeros((2, 113)), np.zeros((2, 113)), vehicle=SC.VEH,
                              users=((1.0, "road", "any"),) * 8, dt=SC.DT, a_brake=4.0)


# ------------------------------------------------------------------------------------------------ 6. through the interface
def test_interface_defaults_and_independence(torch_cuda, tmp_path):
    """``FOInterface.hidden_brake_users`` with its defaults against the checker; the other hidden-traffic entries give the same bits
    before the call and after it"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrakeUsers
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    traj = SY.make_trajectories(16, 31, T.DT, seed=3, ego_pos=np.asarray(sc.ego_initial)[:2], ego_yaw=float(sc.ego_initial[2]))
    users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
    with pytest.raises(RuntimeError, match="hidden_brake_users needs a previous evaluate_scenario"):
        fo.hidden_brake_users(traj, users)
    ego, yaw = WG._drive(fo, sc, 2)
    traj = SY.make_trajectories(16, 31, T.DT, seed=3, ego_pos=ego, ego_yaw=yaw)

    def others():
        r = fo.hidden_reach(traj, v_max=7.0, metric="road", flow="lanes")
        c = fo.hidden_clearance(traj, metric="road")
        b = fo.hidden_brake(traj, v_max=7.0)
        k = fo.hidden_brake_classes(traj, (2.0, 7.0), metric="road")
        parts = [r.arrival, r.cells, r.first, r.slack, r.road_dist, c.key, c.qmin, c.dist, b.brake_first, b.stop, b.commit, b.reach.arrival,
                 k.brake_first, k.stop, k.commit, k.first]
        return [_np(p).copy() for p in parts]

    before = others()
    hbu = fo.hidden_brake_users(traj, users)
    after = others()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
    assert isinstance(hbu, HiddenBrakeUsers) and hbu.a_brake == SY.VEHICLE_BMW320I[4] and hbu.dt == T.DT and hbu.map_of == (0, 1, 1)
    sm = fo.sensor_model
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    ref = BU.brake_users([_np(c.key) for c in hbu.clearances], win, road, [_np(c.qmin) for c in hbu.clearances], sm.raster_origin, sm.cell_size,
                         x, y, _np(hbu.clearances[0].heading), _np(hbu.arc), v, T.HL, T.HW, T.WB, hbu.a_brake, T.DT, hbu.thr, hbu.map_of)
    _same(SimpleNamespace(**{k: _np(getattr(hbu, k)) for k in OUTPUTS}), ref, "interface")
    hb = fo.hidden_brake(traj, v_max=7.0, metric="road", flow="lanes")
    assert np.array_equal(_np(hbu.brake_first)[1], _np(hb.brake_first)) and np.array_equal(_np(hbu.commit)[1], _np(hb.commit))
    assert np.array_equal(_np(hbu.first)[1], _np(hb.reach.first)) and np.array_equal(_np(hbu.stop), _np(hb.stop))


# ------------------------------------------------------------------------------------------------ 7. the kernels of a drive
_TRACE_CHILD = '''
import hashlib, pathlib, sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import numpy as np, torch
import test_hidden_reach_gpu as T
import test_hidden_witness_gpu as WG
from frenetix_occlusion import synthetic as SY
sc = T._scenario("scenario1")
fo = WG._interface(pathlib.Path(sys.argv[2]), sc)
h = hashlib.sha256()
for step in range(3):
    ego, yaw = WG._drive(fo, sc, 1, first=step)
    traj = SY.make_trajectories(64, 31, 0.1, seed=1, ego_pos=ego, ego_yaw=yaw)
    if sys.argv[1] == "users":
        outs = fo.hidden_brake_users(traj, ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))).clearances
    else:
        first = fo.hidden_clearance(traj, v_cap=2.0, metric="road", flow="any")
        outs = (first, fo.hidden_clearance(traj, v_cap=13.9, metric="road", flow="lanes"))
    ba = fo.trajectory_safety_assessment_batch(traj)
    torch.cuda.synchronize()
    parts = [fo.sensor_model.cell_class, fo.sensor_model.occlusion_memory_hidden, fo.sensor_model.occlusion_memory_hidden_vehicles,
             ba.cost if ba is not None else np.zeros(1), np.array([sp.position for sp in fo.spawn_points], dtype=np.float64)]
    for out in outs:
        parts += [out.key, out.qmin, out.dist]
    for p in parts:
        h.update(np.ascontiguousarray(p.cpu().numpy() if torch.is_tensor(p) else p).tobytes())
print("child ok", h.hexdigest())
'''


def _trace(tmp_path, what):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_brake_users.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"), tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + what)
    cfg = tmp_path / ("cfg_" + what)
    cfg.mkdir()
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), what, str(cfg)],
                       capture_output=True, text=True, timeout=TRACE_LIMIT)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    return "\n".join(open(f).read() for f in files).splitlines(), r.stdout.split("child ok")[1].split()[0]


test_kernel_trace_one_launch_beyond_the_clearances_limit = 2 * TRACE_LIMIT + 60


def test_kernel_trace_one_launch_beyond_the_clearances(torch_cuda, tmp_path):
    """three steps of a drive with one call each: with the two ``hidden_clearance`` calls alone no brake kernel of any kind is launched,
    with ``hidden_brake_users`` exactly one fo_hr_brake_users_kernel per call -- the instantiation of 4 classes on 2 maps -- next to the
    clearances' own launches, whose counts do not change, and no other brake kernel; class bytes, H_k, V_k, spawn points, costs and
    every output of the clearances are the same bits either way"""
    lines, digest_clearances = _trace(tmp_path, "clearances")
    count = lambda k: sum(k in line for line in lines)
    assert count("fo_hr_brake") == 0 and count("fo_hc_traj_kernel") == 6
    names = ("fo_hr_rows_kernel", "fo_hr_cols_kernel", "fo_hr_road_band_kernel", "fo_hr_flow_band_kernel", "fo_hc_road_merge_kernel",
             "fo_hc_traj_kernel", "fo_hr_traj_kernel")
    base = {k: count(k) for k in names}
    lines, digest_users = _trace(tmp_path, "users")
    assert count("fo_hr_brake_users_kernel") == 3 and count("fo_hr_brake") == 3
    assert count("fo_hr_brake_users_kernelILi4ELi2E") + count("fo_hr_brake_users_kernel<4, 2>") == 3
    assert {k: count(k) for k in names} == base
    assert digest_users == digest_clearances
