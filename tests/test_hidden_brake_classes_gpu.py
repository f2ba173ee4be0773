"""Hidden-traffic brake clearance by classes on the device (fo_scene_hidden_brake_classes, DESIGN.md §5.10 "Brake clearance by
classes") against the plain statement of the definition (tests/ref_hidden_brake_classes.py) and, class by class, against
fo_scene_hidden_brake of the same library on the same device state.  The checker is handed what the device was handed -- the key map
and qmin the device's own clearance wrote, the headings, the chord lengths and the threshold table -- as data.  Every output is an
exact integer: all comparisons are ``==``."""
import glob
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_classes_scenes as CS
import hidden_brake_scenes as SC
import ref_hidden_brake_classes as BCL
import ref_hidden_clearance as HC
import test_hidden_brake_gpu as BG
import test_hidden_clearance_gpu as CG
import test_hidden_reach_flow_gpu as FG
import test_hidden_reach_gpu as T
import test_hidden_witness_gpu as WG
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
OUTPUTS = ("brake_first", "stop", "commit", "first")
_parked = BG._parked


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw_classes(torch, sm, win, r2_cap, key, qmin, x, y, head, v, arc, a_brake, dt, thr, lens=None, hl=HL, hw=HW, wb=WB, drop=(), **over):
    """fo_scene_hidden_brake_classes on maps and trajectories of the test's own; the output buffers are pre-filled with a pattern.
    ``drop``: names of pointers to hand over as NULL; ``over``: fields of the structure to replace.  Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    M, Tn = x.shape
    thr = np.ascontiguousarray(thr, dtype=np.int32)
    Cn = thr.shape[0]
    tx, ty, th, tv, ta = (up(a, np.float64) for a in (x, y, head, v, arc))
    dk, dq, tl = up(key, np.int32), up(qmin, np.int32), up(lens, np.int32)
    out = SimpleNamespace(brake_first=torch.full((Cn, M, Tn), -7, dtype=torch.int32, device=dev),
                          stop=torch.full((M, Tn), -7, dtype=torch.int32, device=dev),
                          commit=torch.full((Cn, M), -7, dtype=torch.int32, device=dev),
                          first=torch.full((Cn, M), -7, dtype=torch.int32, device=dev))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=hl, hw=hw, wb=wb, win_ix0=win[0], win_iy0=win[1],
              win_nx=win[2], win_ny=win[3], r2_cap=int(r2_cap), C=Cn, d_key=p(dk), d_qmin=p(dq), d_v=p(tv), d_arc=p(ta), a_brake=float(a_brake),
              dt=float(dt), h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), d_brake_first=p(out.brake_first), d_stop=p(out.stop),
              d_commit=p(out.commit), d_first=p(out.first))
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeClasses(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_classes(sm.ctx._h, C.byref(args), N.current_stream(0))
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


def _clearance(torch, sm, sc):
    """the scene's clearance on the device, by the metric and flow of the entry the scene names: (key, qmin) as the device wrote them"""
    from frenetix_occlusion import _native as N
    if sc.entry.endswith("_flow"):
        assert FG._set_moves(sm, sc.moves) == N.FO_OK
        rc, msg, o = FG._raw_clearance(torch, sm, sc.cls, sc.win, sc.r2_cap, sc.hidden, sc.x, sc.y, sc.head, sc.lens)
    else:
        rc, msg, o = CG._raw(torch, sm, sc.cls, sc.win, sc.r2_cap, "road" if sc.entry.endswith("_road") else "euclid", sc.hidden, sc.x, sc.y,
                             sc.head, sc.lens)
    assert rc == 0, msg
    return o.key, o.qmin


def _both(torch, sm, road, sc, key, qmin, what, thr=None, a_brake=None, v=None, arc=None, stats=None):
    """the device's outputs and the checker's on the same data; asserts that they are equal and returns the device's"""
    thr = sc.thr if thr is None else thr
    a_brake = sc.a_brake if a_brake is None else a_brake
    v = sc.v if v is None else v
    arc = sc.arc if arc is None else arc
    rc, msg, out = _raw_classes(torch, sm, sc.win, sc.r2_cap, key, qmin, sc.x, sc.y, sc.head, v, arc, a_brake, sc.dt, thr, sc.lens)
    assert rc == 0, msg
    ref = BCL.brake_classes(key, sc.win, road, qmin, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, arc, v, HL, HW, WB, a_brake, sc.dt, thr, sc.lens, stats)
    _same(out, ref, what)
    return out


# ------------------------------------------------------------------------------------------------ 1. the random scenes
def test_random_scenes_all_three_metrics(torch_cuda):
    """tests/hidden_brake_scenes.RANDOM_SCENES with three classes: T in {1, 2, 31, 32, 33, 64, 65, 254}, M = 1 and around every
    trajectories-per-workgroup edge, ragged lengths with 0, 1 and 2, windows over the whole road, a part of it and the raster's corner,
    key maps of the Euclidean, the road and the lane-flow clearance"""
    torch = torch_cuda
    sm, road = _parked()
    seen = dict(differ=0, safe_slow=0, hits=0, none=0, later=0)
    entries = set()
    for spec in SC.RANDOM_SCENES:
        sc = CS.class_scene(spec, maps=False)
        key, qmin = _clearance(torch, sm, sc)
        out = _both(torch, sm, road, sc, key, qmin, spec)
        entries.add(sc.entry)
        seen["differ"] += int((out.commit[0] != out.commit[2]).sum())
        seen["safe_slow"] += int(((out.commit[0] == -1) & (out.commit[2] >= 0)).sum())
        seen["hits"] += int((out.brake_first >= 0).sum())
        seen["none"] += int((out.commit < 0).sum())
        seen["later"] += int((out.commit > 0).sum())
    print(seen)
    assert entries == set(SC.ENTRIES) and {spec[1] for spec in SC.RANDOM_SCENES} >= {1, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257}
    assert min(seen.values()) > 20


# ------------------------------------------------------------------------------------------------ 2. class counts and the table's edge
@pytest.mark.parametrize("speeds", [(8.0,), (0.0, 8.0), (4.0, 1.5, 8.0), (8.0, 1.5, 0.0, 4.0, 4.0, 6.5, 0.25, 2.0), (1.0, 2.0, 3.0, 4.0, 5.0)],
                         ids=lambda s: "C%d" % len(s))
def test_class_counts(torch_cuda, speeds):
    """C = 1, 2, 3, 8 (and 5: a width of 8 with three classes that are not there), unsorted and repeated speeds, a motionless class:
    every row is the checker's, and the row of a speed is the same whatever the other classes are"""
    torch = torch_cuda
    sm, road = _parked()
    sc = CS.class_scene((35, 24, 31, 1, True), speeds=speeds, maps=False)
    key, qmin = _clearance(torch, sm, sc)
    out = _both(torch, sm, road, sc, key, qmin, speeds)
    assert out.brake_first.shape == (len(speeds), 24, 31) and (out.brake_first >= 0).any() and (out.commit < 0).any()
    c = speeds.index(8.0) if 8.0 in speeds else 3
    rc, msg, alone = _raw_classes(torch, sm, sc.win, sc.r2_cap, key, qmin, sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt, sc.thr[c:c + 1], sc.lens)
    assert rc == 0, msg
    assert np.array_equal(alone.brake_first[0], out.brake_first[c]) and np.array_equal(alone.commit[0], out.commit[c])
    assert np.array_equal(alone.first[0], out.first[c]) and np.array_equal(alone.stop, out.stop)
    if len(speeds) == 8:
        assert np.array_equal(out.brake_first[3], out.brake_first[4]) and np.array_equal(out.commit[3], out.commit[4])


@pytest.mark.parametrize("C, Tn", [(7, 128), (8, 112)])
def test_table_of_exactly_896_entries(torch_cuda, C, Tn):
    torch = torch_cuda
    sm, road = _parked()
    speeds = (8.0, 1.5, 0.0, 4.0, 4.0, 6.5, 0.25, 2.0)[:C]
    # (seeds whose classes differ, by the checker: the motionless class loses a candidate fewer than the others)
    sc = CS.class_scene(({7: 107, 8: 118}[C], 5, Tn, C % 3, True), speeds=speeds, maps=False)
    assert sc.thr.size == 896
    key, qmin = _clearance(torch, sm, sc)
    out = _both(torch, sm, road, sc, key, qmin, (C, Tn))
    assert (out.brake_first >= 0).any() and (out.stop >= 0).any() and (out.commit[2] != out.commit[0]).any()


def test_table_of_904_entries_is_refused(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    sc = CS.class_scene((98, 3, 113, 0, False), speeds=(8.0, 1.5, 0.0, 4.0, 4.0, 6.5, 0.25, 2.0), maps=False)
    key, qmin = _clearance(torch, sm, sc)
    rc, msg, out = _raw_classes(torch, sm, sc.win, sc.r2_cap, key, qmin, sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt, sc.thr, sc.lens)
    assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_classes: C * T = 8 * 113 = 904") and "FO_HIDDEN_BRAKE_MAX_TABLE = 896" in msg
    assert _untouched(out)
    rc, msg, out = _raw_classes(torch, sm, sc.win, sc.r2_cap, key, qmin, sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt, sc.thr[:7], sc.lens)
    assert rc == 0, msg
    with pytest.raises(ValueError, match="at most 896 are possible"):
        sm.hidden_brake_classes(sc.x, sc.y, np.zeros_like(sc.x), sc.v, vehicle=SC.VEH, speeds=(1.0,) * 8, dt=SC.DT, a_brake=4.0)


# ------------------------------------------------------------------------------------------------ 3. beyond the window
def test_footprints_across_and_beyond_the_window(torch_cuda):
    """a window over columns 30 .. 99 of the road, all of it seen and empty: the road beyond its right edge is unobserved (key 0).
    Class 0 does not move (thr = 0: only unobserved road itself), class 1 comes out of it at 8 m/s.  (a) a candidate that drives
    across that edge, (b) one outside the window on the raster all the time, (c) one beside the raster, (d) one that drives off the
    raster's end"""
    torch = torch_cuda
    sm, road = _parked()
    win = SC.WINDOWS[1]
    sc = SC.scene(1, 0, 31, entry=0, win=win, blobs=0)
    sc.cls = SC.class_bytes(np.random.default_rng(0), win, road, 0, specks=False)
    starts = [(SC.ORIGIN[0] + 60 * SC.CS, -1.75, 10.0), (SC.ORIGIN[0] + 112 * SC.CS, -1.75, 6.0), (20.0, 12.0, 10.0), (60.0, 1.75, 14.0)]
    k = np.arange(31, dtype=np.float64)
    sc.x = np.stack([x0 + k * (v * SC.DT) for x0, _, v in starts])
    sc.y = np.stack([np.full(31, y0) for _, y0, _ in starts])
    sc.head = np.zeros((4, 31, 2))
    sc.head[..., 0] = 1.0
    sc.v = np.stack([np.full(31, v) for _, _, v in starts])
    sc.arc = SC.travelled_arc(sc.x, sc.y)
    sc.lens, sc.M = None, 4
    sc.tables = CS.reach_tables((0.0, 8.0), 31, margin=0.0)
    sc.thr = CS.thresholds(sc.tables)
    sc.r2_cap = int(sc.tables[1][-1])
    assert (sc.thr[0] == 0).all()
    key, qmin = _clearance(torch, sm, sc)
    assert (key[sc.cls == 3] > 0).all() and (key[sc.cls == 3] != HC.NONE).any()
    out = _both(torch, sm, road, sc, key, qmin, "edges", a_brake=5.0)
    first = out.first
    assert first[0].tolist() == [int(first[0, 0]), 0, -1, 0] and 12 < first[0, 0] < 22
    assert 0 < out.commit[0, 0] < first[0, 0] and (out.brake_first[0, 0, :out.commit[0, 0]] == -1).all()
    assert 0 <= first[1, 0] < first[0, 0] and 0 <= out.commit[1, 0] < out.commit[0, 0]      # traffic coming out of it arrives sooner
    assert out.commit[0, 1] == 0 and out.brake_first[0, 1].tolist() == list(range(1, 31)) + [-1]
    assert (out.commit[:, 2] == -1).all() and (out.brake_first[:, 2] == -1).all()
    assert out.commit[0, 3] == 0 and out.brake_first[0, 3, -2] == -1 and out.brake_first[0, 3, 0] == 1


# ------------------------------------------------------------------------------------------------ 4. equality with hidden_brake
@pytest.mark.parametrize("metric, flow", [("euclid", "any"), ("road", "any"), ("road", "lanes")])
def test_every_class_equals_hidden_brake_at_its_speed(torch_cuda, metric, flow):
    """scenario 1 after five steps with the occlusion memory on, the bench's fan, through ``SensorModel``: row c of every output of ONE
    ``hidden_brake_classes`` call equals, bit for bit, ``hidden_brake(v_max=speeds[c])`` -- its forecast, its walk -- and the
    checker on the clearance's own maps"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrakeClasses
    sc = T._scenario("scenario1")
    sm, obs = T._sensor(sc, memory={})
    ego, yaw = T._drive(torch, sm, obs, sc, 5)
    traj = SY.make_trajectories(48, 31, T.DT, seed=20250701, ego_pos=ego, ego_yaw=yaw)
    lens = np.random.default_rng(5).integers(0, 33, 48).astype(np.int32) if metric == "euclid" else None
    speeds = (7.0, 2.0, 13.9)
    kw = dict(vehicle=T.VEH, dt=T.DT, a_brake=6.0, lengths=lens, metric=metric, flow=flow)
    hbc = sm.hidden_brake_classes(traj["x"], traj["y"], traj["theta"], traj["v"], speeds=speeds, **kw)
    assert isinstance(hbc, HiddenBrakeClasses) and hbc.speeds == speeds and hbc.clearance.metric == metric and hbc.clearance.flow == flow
    assert hbc.clearance.from_memory and int(hbc.thr.max()) == 169 * hbc.clearance.r2_cap
    got = SimpleNamespace(**{k: _np(getattr(hbc, k)) for k in OUTPUTS})
    for c, v_c in enumerate(speeds):
        hb = sm.hidden_brake(traj["x"], traj["y"], traj["theta"], traj["v"], v_max=v_c, **kw)
        assert np.array_equal(hbc.thr[c].astype(np.int64), 169 * hb.reach.r2.astype(np.int64))
        assert np.array_equal(got.brake_first[c], _np(hb.brake_first)), (c, "brake_first")
        assert np.array_equal(got.stop, _np(hb.stop)), (c, "stop")
        assert np.array_equal(got.commit[c], _np(hb.commit)), (c, "commit")
        assert np.array_equal(got.first[c], _np(hb.reach.first)), (c, "first")
        assert np.array_equal(_np(hbc.arc), _np(hb.arc))
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    stats = {}
    ref = BCL.brake_classes(_np(hbc.clearance.key), win, road, _np(hbc.clearance.qmin), sm.raster_origin, sm.cell_size, x, y,
                            _np(hbc.clearance.heading), _np(hbc.arc), v, T.HL, T.HW, T.WB, 6.0, T.DT, hbc.thr, lens, stats)
    _same(got, ref, (metric, flow))
    print(metric, flow, "commit >= 0 per class:", (got.commit >= 0).sum(axis=1).tolist(), stats)
    assert (got.brake_first >= 0).any() and (got.commit[1] != got.commit[2]).any()
    vc = _np(hbc.critical_speed())
    want = np.where(got.commit >= 0, np.asarray(speeds)[:, None], np.inf).min(axis=0)
    assert hbc.critical_speed().device.type == "cuda" and np.array_equal(vc, want)
    assert np.array_equal(_np(hbc.decided_until()), _np(hb.decided_until()))


# ------------------------------------------------------------------------------------------------ 5. edited inputs
def test_edited_inputs(torch_cuda):
    """what the kernel is handed as data may hold anything: (a) a key map and a qmin that are no clearance's -- random, negative, NONE,
    values above every threshold --, (b) NaN and infinities in v and arc, (c) an arc that is not monotone.  Nothing here can read out of
    range: no index depends on key, qmin, v or arc beyond the clamped segment index; every row is the checker's"""
    torch = torch_cuda
    sm, road = _parked()
    sc = CS.class_scene((35, 24, 31, 1, True), maps=False)
    key, qmin = _clearance(torch, sm, sc)
    plain = _both(torch, sm, road, sc, key, qmin, "plain")
    rng = np.random.default_rng(77)
    # (a)
    top = int(sc.thr.max())
    key2 = rng.integers(-5, 2 * top, key.shape).astype(np.int32)
    key2[rng.random(key.shape) < 0.3] = HC.NONE
    key2[rng.random(key.shape) < 0.02] = -2 ** 31
    qmin2 = rng.integers(-5, 2 * top, qmin.shape).astype(np.int32)
    qmin2[rng.random(qmin.shape) < 0.5] = HC.NONE
    out = _both(torch, sm, road, sc, key2, qmin2, "edited maps")
    assert (out.first != plain.first).any() and np.array_equal(out.stop, plain.stop)
    # (b)
    v, arc = sc.v.copy(), sc.arc.copy()
    v[4, :] = np.nan
    v[5, 3] = np.nan
    arc[7, 12] = np.nan
    arc[8, 0] = np.nan
    arc[9, 30] = np.nan
    v[10, 2], v[11, 2] = np.inf, -np.inf
    out = _both(torch, sm, road, sc, key, qmin, "NaN", v=v, arc=arc)
    others = [m for m in range(24) if m not in (4, 5, 7, 8, 9, 10, 11)]
    for k in ("brake_first", "commit", "first"):
        assert np.array_equal(getattr(out, k)[:, others], getattr(plain, k)[:, others]), k
    assert np.array_equal(out.stop[others], plain.stop[others]) and np.array_equal(out.first, plain.first)
    # (c)
    arc = sc.arc.copy()
    for m in range(0, 24, 3):
        arc[m] = rng.permutation(arc[m])
    arc[2, :] = arc[2, 7]
    _both(torch, sm, road, sc, key, qmin, "non-monotone arc", arc=arc)
    _both(torch, sm, road, sc, key2, qmin2, "everything edited", v=v, arc=arc, a_brake=0.5)


# ------------------------------------------------------------------------------------------------ 6. refusals
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

    def call(table=thr, a_brake=4.0, dt=0.1, r2_cap=30, **kw):
        return _raw_classes(torch, sm, win, r2_cap, key, qmin, x, x, head, x, x, a_brake, dt, np.array(table, dtype=np.int32), **kw)

    rc, msg, out = call()
    assert rc == N.FO_OK and (out.commit == 0).all() and (out.first == 0).all() and (out.stop >= 0).all(), msg
    nan, inf = float("nan"), float("inf")
    ext = N.HIDDEN_REACH_MAX_HALF_EXTENT * sm.cell_size
    nine = [[1, 1, 1, 1]] * 9
    refused = [
        (dict(C=0), "C = 0"), (dict(C=9), "C = 9"), (dict(table=nine), "C = 9"), (dict(C=-1), "C = -1"),
        (dict(drop=("h_thr",)), "h_thr"),
        (dict(table=[[0, 9, 8, 30], [5, 5, 5, 5]]), "h_thr[0] decreases at entry 2"), (dict(table=[thr[0], [5, 5, 5, 4]]), "h_thr[1] decreases at entry 3"),
        (dict(table=[thr[0], [-1, 5, 5, 5]]), "h_thr[1][0] = -1 is negative"),
        (dict(table=[thr[0], [5, 5, 5, 169 * 30 + 1]]), "beyond 169 r2_cap"), (dict(r2_cap=29), "beyond 169 r2_cap"),
        (dict(r2_cap=-1), "r2_cap = -1"), (dict(r2_cap=(N.HIDDEN_REACH_MAX_HALO + 1) ** 2), "FO_HIDDEN_REACH_MAX_HALO"),
        (dict(M=-1), "M = -1"), (dict(T=0), "T = 0"), (dict(T=255), "T = 255"), (dict(T=449), "T = 449"),
        (dict(a_brake=-0.5), "a_brake"), (dict(a_brake=nan), "a_brake"), (dict(a_brake=inf), "a_brake"),
        (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"), (dict(dt=nan), "dt"), (dict(dt=inf), "dt"),
        (dict(drop=("d_key",)), "d_key"), (dict(drop=("d_qmin",)), "d_qmin"),
        (dict(drop=("d_x",)), "d_x"), (dict(drop=("d_y",)), "d_x"), (dict(drop=("d_heading",)), "d_heading"),
        (dict(drop=("d_v",)), "d_v"), (dict(drop=("d_arc",)), "d_arc"),
        (dict(drop=("d_brake_first",)), "d_brake_first"), (dict(drop=("d_stop",)), "d_stop"), (dict(drop=("d_commit",)), "d_commit"),
        (dict(drop=("d_first",)), "d_first"),
        (dict(win_nx=0), "window"), (dict(win_ny=40000), "window"),
        (dict(hl=-0.1), "half extents"), (dict(hw=nan), "half extents"), (dict(wb=ext * 1.01), "half extents"),
    ]
    for kw, text in refused:
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake_classes:") and text in msg, (kw, rc, msg)
        assert _untouched(out), kw
    # M = 0: fine, and nothing is written; the lengths are optional; no move table is asked for
    e = np.zeros((0, 4))
    rc, msg, out = _raw_classes(torch, sm, win, 30, key, qmin[:0], e, e, np.zeros((0, 4, 2)), e, e, 4.0, 0.1, np.array(thr, dtype=np.int32))
    assert rc == N.FO_OK, msg
    assert FG._set_moves(sm, None) == N.FO_OK and call()[0] == N.FO_OK
    # no parameters, and a context without a map
    assert lib.fo_scene_hidden_brake_classes(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert lib.fo_scene_hidden_brake_classes(ctx._h, C.byref(N.HiddenBrakeClasses()), None) == N.FO_E_STATE
    assert N.load().fo_abi_version() == 12


# ------------------------------------------------------------------------------------------------ 7. through the interface
def test_interface_defaults_and_independence(torch_cuda, tmp_path):
    """``FOInterface.hidden_brake_classes`` with its defaults against the checker; the other hidden-traffic entries give the same bits
    before the call and after it"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrakeClasses
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    traj = SY.make_trajectories(16, 31, T.DT, seed=3, ego_pos=np.asarray(sc.ego_initial)[:2], ego_yaw=float(sc.ego_initial[2]))
    with pytest.raises(RuntimeError, match="hidden_brake_classes needs a previous evaluate_scenario"):
        fo.hidden_brake_classes(traj, (2.0, 7.0))
    ego, yaw = WG._drive(fo, sc, 2)
    traj = SY.make_trajectories(16, 31, T.DT, seed=3, ego_pos=ego, ego_yaw=yaw)

    def others():
        r = fo.hidden_reach(traj, v_max=7.0, metric="road", flow="lanes")
        c = fo.hidden_clearance(traj, metric="road")
        b = fo.hidden_brake(traj, v_max=7.0)
        w = fo.hidden_witness(traj, v_max=7.0)
        parts = [r.arrival, r.cells, r.first, r.slack, r.road_dist, c.key, c.qmin, c.dist, b.brake_first, b.stop, b.commit, b.reach.arrival,
                 w.cell, w.source, w.steps, w.dist, w.dirs]
        return [_np(p).copy() for p in parts]

    before = others()
    speeds = (2.0, 7.0, 13.9)
    hbc = fo.hidden_brake_classes(traj, speeds, metric="road", flow="lanes")
    after = others()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
    assert isinstance(hbc, HiddenBrakeClasses) and hbc.a_brake == SY.VEHICLE_BMW320I[4] and hbc.dt == T.DT and hbc.clearance.flow == "lanes"
    assert hbc.clearance.margin == fo.occlusion_memory["margin"] or fo.occlusion_memory["margin"] is None
    sm = fo.sensor_model
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    ref = BCL.brake_classes(_np(hbc.clearance.key), win, road, _np(hbc.clearance.qmin), sm.raster_origin, sm.cell_size, x, y,
                            _np(hbc.clearance.heading), _np(hbc.arc), v, T.HL, T.HW, T.WB, hbc.a_brake, T.DT, hbc.thr)
    _same(SimpleNamespace(**{k: _np(getattr(hbc, k)) for k in OUTPUTS}), ref, "interface")
    # the row of 7 m/s is the hidden_brake of the independence check (same metric and flow)
    hb = fo.hidden_brake(traj, v_max=7.0, metric="road", flow="lanes")
    assert np.array_equal(_np(hbc.brake_first)[1], _np(hb.brake_first)) and np.array_equal(_np(hbc.commit)[1], _np(hb.commit))
    assert np.array_equal(_np(hbc.first)[1], _np(hb.reach.first)) and np.array_equal(_np(hbc.stop), _np(hb.stop))


# ------------------------------------------------------------------------------------------------ 8. the kernels of a drive
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
    if sys.argv[1] == "classes":
        out = fo.hidden_brake_classes(traj, (2.0, 7.0, 13.9), metric="road", flow="lanes").clearance
    else:
        out = fo.hidden_clearance(traj, v_cap=13.9, metric="road", flow="lanes")
    ba = fo.trajectory_safety_assessment_batch(traj)
    torch.cuda.synchronize()
    parts = [fo.sensor_model.cell_class, fo.sensor_model.occlusion_memory_hidden, fo.sensor_model.occlusion_memory_hidden_vehicles,
             ba.cost if ba is not None else np.zeros(1), out.key, out.qmin, out.dist,
             np.array([sp.position for sp in fo.spawn_points], dtype=np.float64)]
    for p in parts:
        h.update(np.ascontiguousarray(p.cpu().numpy() if torch.is_tensor(p) else p).tobytes())
print("child ok", h.hexdigest())
'''


def _trace(tmp_path, what):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_brake_classes.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"), tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + what)
    cfg = tmp_path / ("cfg_" + what)
    cfg.mkdir()
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), what, str(cfg)],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    return "\n".join(open(f).read() for f in files).splitlines(), r.stdout.split("child ok")[1].split()[0]


def test_kernel_trace_one_launch_beyond_the_clearances(torch_cuda, tmp_path):
    """three steps of a drive with one call each: with ``hidden_clearance`` alone no brake kernel of either kind is launched, with
    ``hidden_brake_classes`` exactly one fo_hr_brake_classes_kernel per call next to the clearance's own launches, whose counts do
    not change; class bytes, H_k, V_k, spawn points, costs and every output of the clearance are the same bits either way"""
    lines, digest_clearance = _trace(tmp_path, "clearance")
    count = lambda k: sum(k in line for line in lines)
    assert count("fo_hr_brake") == 0 and count("fo_hc_traj_kernel") == 3
    names = ("fo_hr_rows_kernel", "fo_hr_cols_kernel", "fo_hr_flow_band_kernel", "fo_hc_road_merge_kernel", "fo_hc_traj_kernel", "fo_hr_traj_kernel")
    base = {k: count(k) for k in names}
    lines, digest_classes = _trace(tmp_path, "classes")
    assert count("fo_hr_brake_classes_kernel") == 3 and count("fo_hr_brake") == 3 and count("fo_hr_brake_kernel") == 0
    assert {k: count(k) for k in names} == base
    assert digest_classes == digest_clearance
