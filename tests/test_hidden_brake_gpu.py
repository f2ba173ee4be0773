"""Hidden-traffic brake clearance on the device (fo_scene_hidden_brake, DESIGN.md §5.10 "Brake clearance") against the plain
statement of the definition (tests/ref_hidden_brake.py).  The checker is handed what the device was handed -- the arrival map and
``first`` the device's own forecast wrote, the headings and the chord lengths read back from it -- as data.  Every output is an
exact integer: all comparisons are ``==``."""
import glob
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_scenes as SC
import ref_hidden_brake as B
import test_hidden_brake_cpu as BC
import test_hidden_reach_flow_gpu as FG
import test_hidden_reach_gpu as T
import test_hidden_witness_gpu as WG
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
OUTPUTS = ("brake_first", "stop", "commit")


def _parked():
    """the parked-car map; its raster, origin and cell size are the ones tests/hidden_brake_scenes.py wrote down"""
    sm, road = FG._parked()
    assert np.array_equal(road, SC.road_raster()) and tuple(sm.raster_origin) == SC.ORIGIN and sm.cell_size == SC.CS
    assert (T.HL, T.HW, T.WB) == (HL, HW, WB)
    return sm, road


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw_brake(torch, sm, win, r2, A, first, x, y, head, v, arc, a_brake, dt, lens=None, hl=HL, hw=HW, wb=WB, drop=(), **over):
    """fo_scene_hidden_brake on a map and trajectories of the test's own; the output buffers are pre-filled with a pattern.
    ``drop``: names of pointers to hand over as NULL; ``over``: fields of the base structure or of the call to replace.
    Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    M, Tn = x.shape
    tx, ty, th, tv, ta = (up(a, np.float64) for a in (x, y, head, v, arc))
    dA, df, tl = up(A, np.uint8), up(first, np.int32), up(lens, np.int32)
    out = SimpleNamespace(brake_first=torch.full((M, Tn), -7, dtype=torch.int32, device=dev),
                          stop=torch.full((M, Tn), -7, dtype=torch.int32, device=dev),
                          commit=torch.full((M,), -7, dtype=torch.int32, device=dev))
    r2 = np.ascontiguousarray(r2, dtype=np.int32)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    base = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=hl, hw=hw, wb=wb, J=len(r2),
                h_r2=r2.ctypes.data_as(C.POINTER(C.c_int32)), win_ix0=win[0], win_iy0=win[1], win_nx=win[2], win_ny=win[3],
                d_arrival=p(dA), d_first=p(df))
    call = dict(d_v=p(tv), d_arc=p(ta), a_brake=float(a_brake), dt=float(dt), d_brake_first=p(out.brake_first), d_stop=p(out.stop),
                d_commit=p(out.commit))
    for k, val in over.items():
        (base if k in base else call)[k] = val
    for k in drop:
        (base if k in base else call)[k] = None
    args = N.HiddenBrake(base=N.HiddenReach(**base), **call)
    rc = sm.ctx._lib.fo_scene_hidden_brake(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(**{k: _np(getattr(out, k)) for k in OUTPUTS})


def _untouched(out):
    return all((getattr(out, k) == -7).all() for k in OUTPUTS)


def _same(out, ref, what):
    for k, r in zip(OUTPUTS, ref):
        got = getattr(out, k)
        assert got.dtype == r.dtype and got.shape == r.shape, (what, k)
        assert np.array_equal(got, r), (what, k, np.argwhere(got != r)[:4].tolist())


def _forecast(torch, sm, sc, r2=None):
    """the scene's forecast on the device, by the entry the scene names: (A, cells, first) as the device wrote them"""
    from frenetix_occlusion import _native as N
    r2 = sc.r2 if r2 is None else r2
    if sc.entry == "fo_scene_hidden_reach":
        rc, msg, maps = T._raw(torch, sm, sc.cls, sc.win, r2, sc.hidden, sc.x, sc.y, sc.head, sc.lens)
    else:
        assert FG._set_moves(sm, sc.moves) == N.FO_OK
        rc, msg, maps = FG._raw_reach(torch, sm, sc.entry, sc.cls, sc.win, r2, sc.hidden, sc.x, sc.y, sc.head, sc.lens)
    assert rc == 0, msg
    return maps.arrival, maps.cells, maps.first


def _both(torch, sm, road, sc, A, first, what, a_brake=None, v=None, arc=None, stats=None):
    """the device's outputs and the checker's on the same data; asserts that they are equal and returns the device's"""
    a_brake = sc.a_brake if a_brake is None else a_brake
    v = sc.v if v is None else v
    arc = sc.arc if arc is None else arc
    rc, msg, out = _raw_brake(torch, sm, sc.win, sc.r2, A, first, sc.x, sc.y, sc.head, v, arc, a_brake, sc.dt, sc.lens)
    assert rc == 0, msg
    ref = B.brake(A, sc.win, road, first, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, arc, v, HL, HW, WB, a_brake, sc.dt, sc.lens, stats)
    _same(out, ref, what)
    return out


# ------------------------------------------------------------------------------------------------ 1. the random scenes
def test_random_scenes_all_three_forecasts(torch_cuda):
    """tests/hidden_brake_scenes.RANDOM_SCENES (held to their conditions by tests/test_hidden_brake_cpu.py): T in {1, 2, 31, 32, 33,
    64, 65, 254}, M around every trajectories-per-workgroup edge, ragged lengths with 0, 1 and 2, windows over the whole road, a
    part of it and the raster's corner, maps of the Euclidean, the road and the lane-flow forecast"""
    torch = torch_cuda
    sm, road = _parked()
    seen = dict(none=0, later=0, now=0, after_stop=0, hits=0, open_end=0)
    entries = set()
    for spec in SC.RANDOM_SCENES:
        sc = SC.scene(*spec)
        A, _, first = _forecast(torch, sm, sc)
        stats = {}
        out = _both(torch, sm, road, sc, A, first, spec, stats=stats)
        entries.add(sc.entry)
        seen["none"] += int((out.commit < 0).sum())
        seen["later"] += int((out.commit > 0).sum())
        seen["now"] += int((out.commit == 0).sum())
        seen["hits"] += int((out.brake_first >= 0).sum())
        seen["after_stop"] += stats["after_stop"]
        seen["open_end"] += int((out.stop == sc.T).sum())
    print(seen)
    assert entries == set(SC.ENTRIES)
    assert min(seen.values()) > 20


def test_long_horizon(torch_cuda):
    """T = 254: the rows of four trajectories take 48 KB of LDS, a lane walks four brake starts"""
    torch = torch_cuda
    sm, road = _parked()
    for seed, M in ((82, 3), (84, 5)):
        sc = SC.scene(seed, M, 254, entry=seed % 3, ragged=M == 5)
        A, _, first = _forecast(torch, sm, sc)
        out = _both(torch, sm, road, sc, A, first, seed)
        assert (out.stop >= 0).any()


# ------------------------------------------------------------------------------------------------ 2. beyond the window
def test_footprints_across_and_beyond_the_window(torch_cuda):
    """a window over columns 30 .. 99 of the road, all of it seen and empty: the road beyond its right edge is unobserved (A = 0).
    (a) a candidate that drives across that edge, (b) one that is outside the window on the raster all the time, (c) one beside the
    raster, (d) one that drives off the raster's end"""
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
    sc.r2 = np.zeros(31, dtype=np.int64)                         # nothing spreads: the only reached road is the road beyond the window
    A, cells, first = _forecast(torch, sm, sc)
    assert (A[sc.cls == 3] == 255).all()
    out = _both(torch, sm, road, sc, A, first, "edges", a_brake=5.0)
    assert first.tolist() == [int(first[0]), 0, -1, 0] and 12 < first[0] < 22
    # (a): fail-safe until its stopping distance (10 m) reaches the edge; the manoeuvres before that stand clear of it
    assert 0 < out.commit[0] < first[0] and (out.brake_first[0, :out.commit[0]] == -1).all()
    # (b): every manoeuvre is in unobserved road at its first pose
    assert out.commit[1] == 0 and out.brake_first[1].tolist() == list(range(1, 31)) + [-1]
    # (c): nothing beside the raster is road
    assert out.commit[2] == -1 and (out.brake_first[2] == -1).all()
    # (d): it leaves the raster's road at x = 70 (column 162): from then on its footprint holds no road cell at all
    assert out.commit[3] == 0 and out.brake_first[3, -2] == -1 and out.brake_first[3, 0] == 1


# ------------------------------------------------------------------------------------------------ 3. a drive through the model
@pytest.mark.parametrize("metric, flow", [("euclid", "any"), ("road", "any"), ("road", "lanes")])
def test_scenario_drive_through_the_sensor_model(torch_cuda, metric, flow):
    """scenario 1 after five steps with the occlusion memory on, the bench's fan: ``SensorModel.hidden_brake`` on each forecast;
    arc, headings, A and first are read back from the device and handed to the checker"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrake, travelled_arc
    sc = T._scenario("scenario1")
    sm, obs = T._sensor(sc, memory={})
    ego, yaw = T._drive(torch, sm, obs, sc, 5)
    traj = SY.make_trajectories(48, 31, T.DT, seed=20250701, ego_pos=ego, ego_yaw=yaw)
    lens = np.random.default_rng(5).integers(0, 33, 48).astype(np.int32) if metric == "euclid" else None
    hb = sm.hidden_brake(traj["x"], traj["y"], traj["theta"], traj["v"], vehicle=T.VEH, v_max=8.0, dt=T.DT, a_brake=6.0, lengths=lens,
                         metric=metric, flow=flow)
    assert isinstance(hb, HiddenBrake) and hb.reach.metric == metric and hb.reach.flow == flow and hb.reach.from_memory
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    arc = _np(hb.arc)
    assert np.array_equal(arc, travelled_arc(x, y))              # host arrays: be.py's formula, uploaded as it is
    stats = {}
    ref = B.brake(_np(hb.reach.arrival), win, road, _np(hb.reach.first), sm.raster_origin, sm.cell_size, x, y, _np(hb.reach.heading), arc, v,
                  T.HL, T.HW, T.WB, 6.0, T.DT, lens, stats)
    _same(SimpleNamespace(brake_first=_np(hb.brake_first), stop=_np(hb.stop), commit=_np(hb.commit)), ref, (metric, flow))
    commit = _np(hb.commit)
    print(metric, flow, "commit -1 / 0 / later:", int((commit < 0).sum()), int((commit == 0).sum()), int((commit > 0).sum()), stats)
    assert (_np(hb.brake_first) >= 0).any()
    Lm = np.full(48, 31) if lens is None else np.clip(lens, 0, 31)
    stop = _np(hb.stop)
    want = [next((b for b in range(Lm[m]) if stop[m, b] == Lm[m]), Lm[m]) for m in range(48)]
    assert _np(hb.decided_until()).tolist() == want
    # device tensors in: the chord length is made on the device, within 4 ulp of the host's, and is what the launch was handed
    dev = sm.device
    tx, ty = torch.as_tensor(x).to(dev), torch.as_tensor(y).to(dev)
    hb2 = sm.hidden_brake(tx, ty, traj["theta"], torch.as_tensor(v).to(dev), vehicle=T.VEH, v_max=8.0, dt=T.DT, a_brake=6.0, lengths=lens,
                          metric=metric, flow=flow)
    arc2 = _np(hb2.arc)
    assert hb2.arc.device.type == "cuda" and (np.abs(arc2 - arc) <= 4 * np.spacing(np.maximum(arc, 1e-300))).all()
    ref2 = B.brake(_np(hb2.reach.arrival), win, road, _np(hb2.reach.first), sm.raster_origin, sm.cell_size, x, y, _np(hb2.reach.heading), arc2, v,
                   T.HL, T.HW, T.WB, 6.0, T.DT, lens)
    _same(SimpleNamespace(brake_first=_np(hb2.brake_first), stop=_np(hb2.stop), commit=_np(hb2.commit)), ref2, (metric, flow, "device"))


# ------------------------------------------------------------------------------------------------ 4. the tie to cells
def test_without_deceleration_brake_first_follows_cells(torch_cuda):
    """the dyadic fan of the CPU test, constant speed, a_brake = 0: every brake pose is the candidate's own sample, so
    brake_first[m][b] is the first i > b with cells[m][i] > 0 of the device's own forecast"""
    torch = torch_cuda
    sm, road = _parked()
    dt, Tn = 0.125, 32
    sc = SC.scene(5, 0, Tn, entry=0, win=SC.WINDOWS[0])
    sc.x, sc.y, sc.head, sc.v, sc.arc = BC.dyadic_fan(sc.win, Tn, dt)
    sc.dt, sc.M = dt, len(sc.x)
    from ref_hidden_reach import reach_table
    sc.r2 = reach_table(8.0, dt, math.sqrt(2.0) * SC.CS, SC.CS, Tn)
    A, cells, first = _forecast(torch, sm, sc)
    out = _both(torch, sm, road, sc, A, first, "tie", a_brake=0.0)
    assert np.array_equal(out.brake_first, BC.first_hit_after(cells))
    assert (cells > 0).any() and (out.brake_first >= 0).any() and (out.brake_first < 0).any()
    assert np.array_equal(out.stop, np.where(sc.v > 0.0, Tn, np.arange(Tn)[None, :]))


# ------------------------------------------------------------------------------------------------ 5. edited inputs
def test_edited_inputs(torch_cuda):
    """what the kernel is handed as data may hold anything: (a) an arc that is not monotone, (b) NaN in one trajectory's speeds and
    in one arc entry of another -- the rows of every other trajectory are what they were, and all rows are the checker's, (c) a
    deceleration that stops every manoeuvre at b + 1, (d) speeds three times the path's own: the manoeuvres clamp at its end.
    Nothing here can read out of range: the segment index is clamped before every read and moves forward only"""
    torch = torch_cuda
    sm, road = _parked()
    sc = SC.scene(35, 24, 31, entry=1, ragged=True)
    A, _, first = _forecast(torch, sm, sc)
    plain = _both(torch, sm, road, sc, A, first, "plain")
    rng = np.random.default_rng(99)
    # (a)
    arc = sc.arc.copy()
    for m in range(0, 24, 3):
        arc[m] = rng.permutation(arc[m])
    arc[1, 10:20] = arc[1, 10:20][::-1]
    arc[2, :] = arc[2, 7]
    out = _both(torch, sm, road, sc, A, first, "non-monotone arc", arc=arc)
    untouched = [m for m in range(24) if m % 3 and m not in (1, 2)]
    for k in OUTPUTS:
        assert np.array_equal(getattr(out, k)[untouched], getattr(plain, k)[untouched]), k
    assert any(not np.array_equal(out.brake_first[m], plain.brake_first[m]) for m in range(0, 24, 3))
    # (b)
    v, arc = sc.v.copy(), sc.arc.copy()
    v[4, :] = np.nan
    v[5, 3] = np.nan
    arc[7, 12] = np.nan
    arc[8, 0] = np.nan
    arc[9, 30] = np.nan                                          # the end of the path itself
    v[10, 2], v[11, 2] = np.inf, -np.inf
    out = _both(torch, sm, road, sc, A, first, "NaN", v=v, arc=arc)
    others = [m for m in range(24) if m not in (4, 5, 7, 8, 9, 10, 11)]
    for k in OUTPUTS:
        assert np.array_equal(getattr(out, k)[others], getattr(plain, k)[others]), k
    Lm = B.clip_len(31, sc.lens, 4)
    assert out.stop[4, :Lm].tolist() == list(range(Lm))          # fmax(NaN, 0) = 0: such a manoeuvre stands at once
    # (c)
    out = _both(torch, sm, road, sc, A, first, "stops at b + 1", a_brake=1e6)
    for m in range(24):
        Lm = B.clip_len(31, sc.lens, m)
        want = [b if sc.v[m, b] == 0.0 else min(b + 1, Lm) for b in range(Lm)]
        assert out.stop[m, :Lm].tolist() == want, m
    # (d)
    stats = {}
    rc, msg, out = _raw_brake(torch, sm, sc.win, sc.r2, A, first, sc.x, sc.y, sc.head, 3.0 * sc.v, sc.arc, 0.5, sc.dt, sc.lens)
    assert rc == 0, msg
    _same(out, B.brake(A, sc.win, road, first, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, 3.0 * sc.v, HL, HW, WB, 0.5, sc.dt, sc.lens, stats), "clamp")
    clamped = 0
    for m in range(24):
        Lm = B.clip_len(31, sc.lens, m)
        if Lm > 2 and sc.v[m, 0] > 1.0:
            poses = list(B.manoeuvre(sc.x[m].tolist(), sc.y[m].tolist(), sc.head[m].tolist(), sc.arc[m].tolist(), 3.0 * sc.v[m, 0], Lm, 0, 0.5, sc.dt))
            clamped += poses[-1][6] == sc.arc[m, Lm - 1] and abs(poses[-1][1] - sc.x[m, Lm - 1]) < 1e-9
    assert clamped > 5


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, road = _parked()
    lib = sm.ctx._lib
    win = (3, 1, 12, 9)
    A = np.zeros((9, 12), dtype=np.uint8)
    x = np.zeros((2, 4))
    head = np.zeros((2, 4, 2))
    head[..., 0] = 1.0
    first = np.zeros(2, dtype=np.int32)
    r2 = [2, 2, 8, 30]

    def call(table=r2, a_brake=4.0, dt=0.1, **kw):
        return _raw_brake(torch, sm, win, table, A, first, x, x, head, x, x, a_brake, dt, **kw)

    rc, msg, out = call()
    assert rc == N.FO_OK and (out.commit == 0).all() and (out.stop >= 0).all(), msg
    nan, inf = float("nan"), float("inf")
    ext = N.HIDDEN_REACH_MAX_HALF_EXTENT * sm.cell_size
    refused = [
        (dict(table=[2, 9, 8, 30]), "decreases"), (dict(table=[-1, 2, 8, 30]), "negative"),
        (dict(table=[0, (N.HIDDEN_REACH_MAX_HALO + 1) ** 2]), "FO_HIDDEN_REACH_MAX_HALO"),
        (dict(J=0), "J = 0"), (dict(J=255), "J = 255"), (dict(drop=("h_r2",)), "h_r2"),
        (dict(M=-1), "M = -1"), (dict(T=0), "T = 0"), (dict(T=5), "T = 5"),
        (dict(a_brake=-0.5), "a_brake"), (dict(a_brake=nan), "a_brake"), (dict(a_brake=inf), "a_brake"),
        (dict(dt=0.0), "dt"), (dict(dt=-0.1), "dt"), (dict(dt=nan), "dt"), (dict(dt=inf), "dt"),
        (dict(drop=("d_arrival",)), "d_arrival"),
        (dict(drop=("d_x",)), "d_x"), (dict(drop=("d_y",)), "d_x"), (dict(drop=("d_heading",)), "d_heading"),
        (dict(drop=("d_first",)), "d_first"), (dict(drop=("d_v",)), "d_v"), (dict(drop=("d_arc",)), "d_arc"),
        (dict(drop=("d_brake_first",)), "d_brake_first"), (dict(drop=("d_stop",)), "d_stop"), (dict(drop=("d_commit",)), "d_commit"),
        (dict(win_nx=0), "window"), (dict(win_ny=40000), "window"),
        (dict(hl=-0.1), "half extents"), (dict(hw=nan), "half extents"), (dict(wb=ext * 1.01), "half extents"),
    ]
    for kw, text in refused:
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_brake:") and text in msg, (kw, rc, msg)
        assert _untouched(out), kw
    # M = 0: fine, and nothing is written
    e = np.zeros((0, 4))
    rc, msg, out = _raw_brake(torch, sm, win, r2, A, first[:0], e, e, np.zeros((0, 4, 2)), e, e, 4.0, 0.1)
    assert rc == N.FO_OK, msg
    # the lengths are optional, the map of any forecast serves: no move table is asked for
    assert FG._set_moves(sm, None) == N.FO_OK and call()[0] == N.FO_OK
    # no parameters, and a context without a map
    assert lib.fo_scene_hidden_brake(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert lib.fo_scene_hidden_brake(ctx._h, C.byref(N.HiddenBrake()), None) == N.FO_E_STATE
    assert N.load().fo_abi_version() == 12


# ------------------------------------------------------------------------------------------------ 7. through the interface
def test_interface_defaults_on_the_device(torch_cuda, tmp_path):
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenBrake
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    traj = SY.make_trajectories(16, 31, T.DT, seed=3, ego_pos=np.asarray(sc.ego_initial)[:2], ego_yaw=float(sc.ego_initial[2]))
    with pytest.raises(RuntimeError, match="hidden_brake needs a previous evaluate_scenario"):
        fo.hidden_brake(traj)
    ego, yaw = WG._drive(fo, sc, 2)
    traj = SY.make_trajectories(16, 31, T.DT, seed=3, ego_pos=ego, ego_yaw=yaw)
    hb = fo.hidden_brake(traj, metric="road", flow="lanes")
    assert isinstance(hb, HiddenBrake) and hb.a_brake == SY.VEHICLE_BMW320I[4] and hb.dt == T.DT and hb.reach.flow == "lanes"
    sm = fo.sensor_model
    cls, win, road, _ = T._state(torch, sm)
    x, y, v = (np.asarray(traj[k], dtype=np.float64) for k in ("x", "y", "v"))
    ref = B.brake(_np(hb.reach.arrival), win, road, _np(hb.reach.first), sm.raster_origin, sm.cell_size, x, y, _np(hb.reach.heading), _np(hb.arc), v,
                  T.HL, T.HW, T.WB, hb.a_brake, T.DT)
    _same(SimpleNamespace(brake_first=_np(hb.brake_first), stop=_np(hb.stop), commit=_np(hb.commit)), ref, "interface")


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
    if sys.argv[1] == "brake":
        out = fo.hidden_brake(traj, v_max=13.9, metric="road", flow="lanes").reach
    else:
        out = fo.hidden_reach(traj, v_max=13.9, metric="road", flow="lanes")
    ba = fo.trajectory_safety_assessment_batch(traj)
    torch.cuda.synchronize()
    parts = [fo.sensor_model.cell_class, fo.sensor_model.occlusion_memory_hidden, fo.sensor_model.occlusion_memory_hidden_vehicles,
             ba.cost if ba is not None else np.zeros(1), out.first, out.cells, out.slack, out.arrival,
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
    child = tmp_path / "child_brake.py"
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


def test_kernel_trace_one_launch_per_call_and_nothing_else_changes(torch_cuda, tmp_path):
    """three steps of a drive with one forecast each: with ``hidden_reach`` alone no brake kernel is launched, with ``hidden_brake``
    exactly one per call next to the forecast's own; class bytes, H_k, V_k, spawn points, costs and every output of the forecast are
    the same bits with the interleaved calls as without them"""
    lines, digest_reach = _trace(tmp_path, "reach")
    count = lambda k: sum(k in line for line in lines)
    assert count("fo_hr_brake") == 0 and count("fo_hr_traj_kernel") == 3
    base = {k: count(k) for k in ("fo_hr_rows_kernel", "fo_hr_cols_kernel", "fo_hr_flow_band_kernel", "fo_hr_road_arrival_kernel")}
    lines, digest_brake = _trace(tmp_path, "brake")
    assert count("fo_hr_brake_kernel") == 3 and count("fo_hr_brake") == 3 and count("fo_hr_traj_kernel") == 3
    assert {k: count(k) for k in base} == base
    assert digest_brake == digest_reach
