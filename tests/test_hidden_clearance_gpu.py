"""Hidden-traffic clearance on the device (fo_scene_hidden_clearance, DESIGN.md §5.10 "Clearance and critical speed") against the
NumPy statement of its definition (tests/ref_hidden_clearance.py) and against the reach forecast of the same library on the same
device state.  Every output is an exact integer: all comparisons are ``==``."""
import glob
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_clearance as HC
import ref_hidden_reach as HR
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DT, VEH, HL, HW, WB = T.DT, T.VEH, T.HL, T.HW, T.WB
_np = T._np
METRICS = ("euclid", "road")
SPEEDS = (2.0, 7.0, 13.9)


def _raw(torch, sm, cls, win, r2_cap, metric, hidden=None, x=None, y=None, head=None, lens=None, hl=HL, hw=HW, wb=WB, T_=None,
         dist=True, **over):
    """fo_scene_hidden_clearance with class bytes / windows / caps of the test's own; returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_cls, d_hid = up(cls, np.uint8), up(hidden, np.uint8)
    M = 0 if x is None else x.shape[0]
    Tn = (1 if x is None else x.shape[1]) if T_ is None else T_
    tx, ty, th, tl = up(x, np.float64), up(y, np.float64), up(head, np.float64), up(lens, np.int32)
    key = torch.full((win[3], win[2]), -7, dtype=torch.int32, device=dev)
    qmin = torch.full((M, Tn), -7, dtype=torch.int32, device=dev)
    d_dist = torch.full((win[3], win[2]), 7777, dtype=torch.int16, device=dev)      # (the bytes of a uint16 map)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=hl, hw=hw, wb=wb, r2_cap=int(r2_cap),
              metric=N.HIDDEN_CLEARANCE_METRIC.get(metric, metric), d_cls=p(d_cls), d_hidden_or_null=p(d_hid), win_ix0=win[0],
              win_iy0=win[1], win_nx=win[2], win_ny=win[3], d_key=key.data_ptr(), d_qmin=p(qmin),
              d_dist_or_null=d_dist.data_ptr() if dist else None)
    kw.update(over)
    args = N.HiddenClearance(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_clearance(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(key=_np(key), qmin=_np(qmin), dist=_np(d_dist).view(np.uint16))


def _parked():
    lanes, obstacles, _ = T._parked_car_scene()
    sm, _ = T._sensor(lanes, obstacles)
    return sm, sm.road_raster()


# ------------------------------------------------------------------------------------------------ device = checker
def test_key_and_qmin_match_the_checker(torch_cuda):
    """synthetic class maps on the parked-car map.  Windows of 33 x 33 and 70 x 45 (across the 32 x 32 tile of the distance bands
    and the 64-column tile of the column pass) inside the raster and hanging over its edges, h of 0, 3, 17 (more than one tile of
    halo) and 254 (8 x 8 window), M of 1 and 70, T of 1, 5, 33 and 70 (a trajectory longer than a wave), ragged lengths with 0,
    poses in, partly in and far outside the window and off the raster, with and without a hidden mask; both metrics"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    rng = np.random.default_rng(20240612)
    cases = [(33, 33, 0), (33, 33, 3), (33, 33, 17), (70, 45, 0), (70, 45, 3), (70, 45, 17), (8, 8, N.HIDDEN_REACH_MAX_HALO)]
    Ts, Ms = [1, 5, 33, 70], [1, 70]
    later, none_dist, edges = 0, 0, 0
    for case, (nx, ny, h) in enumerate(cases):
        for rep in range(2):
            n = 2 * case + rep
            ix0 = [int(rng.integers(5, rnx - nx - 5)), -nx // 3, rnx - nx // 2][n % 3]
            iy0 = [int(rng.integers(-2, 4)), rny - ny // 2, int(rng.integers(-ny + 2, 2))][n % 3]
            win = (ix0, iy0, nx, ny)
            edges += ix0 < 0 or iy0 < 0 or ix0 + nx > rnx or iy0 + ny > rny
            cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx), p=[0.1, 0.04, 0.62, 0.03, 0.03, 0.18])
            hidden = (rng.random((ny, nx)) < 0.02).astype(np.uint8) if rep else None
            if h > 60:                                  # two sources alone: keys up to the cap in a small window
                hidden = np.zeros((ny, nx), dtype=np.uint8)
                hidden.ravel()[rng.integers(0, nx * ny, 2)] = 1
                win = (rnx + 300, rny + 300, nx, ny)    # (and nothing outside the window: off the raster)
            r2_cap = int(rng.integers(h * h, (h + 1) * (h + 1))) if rep else h * h
            Tn, M = Ts[n % 4], Ms[(n // 2 + n) % 2]
            x, y, head = T._random_poses(rng, sm, win, M, Tn)
            lens = rng.integers(-1, Tn + 2, M).astype(np.int32) if n % 3 != 1 else None
            if lens is not None:
                lens[0] = 0
            for metric in METRICS:
                rc, msg, out = _raw(torch, sm, cls, win, r2_cap, metric, hidden, x, y, head, lens, dist=n % 5 != 4)
                assert rc == 0, msg
                key, D2, d = HC.key_map(cls, win, road, r2_cap, metric, hidden)
                assert np.array_equal(out.key, key), (n, metric, h, win, int((out.key != key).sum()))
                qmin = HC.clearance(key, win, road, sm.raster_origin, sm.cell_size, x, y, head, HL, HW, WB, lens)
                assert np.array_equal(out.qmin, qmin), (n, metric, int((out.qmin != qmin).sum()))
                if metric == "road" and n % 5 != 4:
                    assert np.array_equal(out.dist, d.astype(np.uint16)), (n, int((out.dist != d).sum()))
                    ke = HC.key_map(cls, win, road, r2_cap, "euclid", hidden)[0]
                    later += int(((key > ke) & (key != HC.NONE)).sum())
                    none_dist += int(((key == HC.NONE) & (ke != HC.NONE)).sum())
                else:
                    assert (out.dist == 7777).all()     # euclid, or no buffer handed in: untouched
    assert later > 0 and none_dist > 0 and edges >= 4


# ------------------------------------------------------------------------------------------------ the tie, on the device
@pytest.mark.parametrize("name,M", [("scenario1", 128), ("city_grid", 64)])
def test_reach_from_the_clearance_equals_hidden_reach(torch_cuda, name, M):
    """one visibility stage, then ONE clearance call per metric and hidden_reach per speed on the same device state: what
    .reach(v) derives from qmin is hidden_reach(v_max=v)'s cells > 0, first and slack"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    sc = T._scenario(name)
    sm, obs = T._sensor(sc)
    ego, yaw = T._drive(torch, sm, obs, sc, 1)
    traj = SY.make_trajectories(M, 31, DT, seed=20240612, ego_pos=ego, ego_yaw=yaw)
    hits = 0
    for metric in METRICS:
        hc = sm.hidden_clearance(traj["x"], traj["y"], traj["theta"], vehicle=VEH, v_cap=SPEEDS[-1], dt=DT, metric=metric)
        assert hc.metric == metric and (hc.dist is None) == (metric == "euclid") and hc.qmin.shape == (M, 31)
        assert hc.r2_cap == int(HR.reach_table(SPEEDS[-1], DT, math.sqrt(2.0) * sm.cell_size, sm.cell_size, 31)[-1])
        for v in SPEEDS:
            hr = sm.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=VEH, v_max=v, dt=DT, metric=metric)
            hit, first, slack = hc.reach(v)
            assert hit.is_cuda and first.dtype == torch.int32 and slack.dtype == torch.int32
            assert np.array_equal(_np(hit), _np(hr.cells) > 0), (metric, v)
            assert np.array_equal(_np(first), _np(hr.first)) and np.array_equal(_np(slack), _np(hr.slack)), (metric, v)
            hits += int((_np(hr.first) >= 0).sum())
        with pytest.raises(ValueError, match="beyond r2_cap"):
            hc.reach(14.5)
        vc = _np(hc.critical_speed())
        cls, win, road, hid = T._state(torch, sm)
        key = HC.key_map(cls, win, road, hc.r2_cap, metric, hid)[0]
        assert np.array_equal(_np(hc.key), key)
        want = HC.critical_speed(_np(hc.qmin), sm.cell_size, DT, math.sqrt(2.0) * sm.cell_size)
        assert np.array_equal(np.isinf(vc), np.isinf(want)) and np.allclose(vc, want, rtol=1e-14, atol=0.0)
    assert hits > 0


def test_open_road_equals_euclid_on_the_device(torch_cuda):
    torch = torch_cuda
    sm, road = _parked()
    rows, cols = np.flatnonzero(road.any(axis=1)), np.flatnonzero(road.any(axis=0))
    assert road.sum() == len(rows) * len(cols)              # the raster's road is one rectangle
    rng = np.random.default_rng(11)
    win = (int(cols[0]) + 9, int(rows[0]) + 1, 90, len(rows) - 2)
    cls = rng.choice(np.array([1, 3, 5], dtype=np.uint8), (win[3], win[2]), p=[0.01, 0.98, 0.01])
    r2_cap = int(HR.reach_table(13.9, DT, math.sqrt(2.0) * sm.cell_size, sm.cell_size, 31)[-1])
    x, y, head = T._random_poses(rng, sm, win, 70, 31)
    rc, msg, a = _raw(torch, sm, cls, win, r2_cap, "road", None, x, y, head)
    assert rc == 0, msg
    rc, msg, b = _raw(torch, sm, cls, win, r2_cap, "euclid", None, x, y, head)
    assert rc == 0, msg
    assert ((a.key > 0) & (a.key < HC.NONE)).any()
    assert np.array_equal(a.key, b.key) and np.array_equal(a.qmin, b.qmin)


def test_heading_reuse_is_bit_identical(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    sc = T._scenario("scenario1")
    sm, obs = T._sensor(sc, memory={})
    ego, yaw = T._drive(torch, sm, obs, sc, 3)
    traj = SY.make_trajectories(70, 31, DT, seed=5, ego_pos=ego, ego_yaw=yaw)
    lens = np.random.default_rng(5).integers(0, 33, 70).astype(np.int32)
    hr = sm.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=VEH, v_max=7.0, dt=DT)
    for metric in METRICS:
        a = sm.hidden_clearance(traj["x"], traj["y"], traj["theta"], vehicle=VEH, v_cap=7.0, dt=DT, lengths=lens, metric=metric)
        b = sm.hidden_clearance(traj["x"], traj["y"], None, vehicle=VEH, v_cap=7.0, dt=DT, lengths=lens, metric=metric,
                                heading=hr.heading)
        c = sm.hidden_clearance(traj["x"], traj["y"], None, vehicle=VEH, v_cap=7.0, dt=DT, lengths=lens, metric=metric,
                                heading=a.heading)
        assert a.from_memory and b.heading is hr.heading
        for o in (b, c):
            assert torch.equal(a.key, o.key) and torch.equal(a.qmin, o.qmin) and torch.equal(a.heading, o.heading)
        assert (_np(a.qmin)[np.arange(31)[None, :] >= lens[:, None]] == HC.NONE).all()


# ------------------------------------------------------------------------------------------------ off means off
def _drive_interface(torch, fo, sc_ego, traj, clearance):
    res = []
    for step in range(4):
        ego = np.array([sc_ego[0] + 0.8 * step, sc_ego[1]])
        fo.evaluate_scenario({}, ego, 0.0, (0.8 * step, 0.0), 8.0, step, None)
        if clearance:
            fo.hidden_clearance(traj, v_cap=7.0)
        hr = fo.hidden_reach(traj, metric="road")
        ba = fo.trajectory_safety_assessment_batch(traj)
        if clearance:
            fo.hidden_clearance(traj, metric="road")
        he = fo.hidden_reach(traj)
        torch.cuda.synchronize()
        pts = [(p.agent_type, tuple(np.asarray(p.position, dtype=np.float64).tolist())) for p in fo.spawn_points]
        hid = fo.sensor_model.occlusion_memory_hidden
        res.append((_np(fo.sensor_model.cell_class).copy(), pts, None if ba is None else _np(ba.cost).copy(),
                    None if hid is None else hid.copy(),
                    [_np(t).copy() for o in (hr, he) for t in (o.arrival, o.cells, o.first, o.slack)] + [_np(hr.road_dist).copy()]))
    return res


def test_interleaved_calls_change_nothing(torch_cuda, tmp_path):
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    lanes, obstacles, path = T._parked_car_scene(17.0, -1.9)
    traj = SY.make_trajectories(96, 31, DT, seed=4, ego_pos=(0.0, 1.0), ego_yaw=0.0)
    a = _drive_interface(torch, T._interface(tmp_path, lanes, obstacles, path, (0.0, 1.0), True, "a.yaml"), (0.0, 1.0), traj, False)
    b = _drive_interface(torch, T._interface(tmp_path, lanes, obstacles, path, (0.0, 1.0), True, "b.yaml"), (0.0, 1.0), traj, True)
    for (ca, pa, ka, ha, ra), (cb, pb, kb, hb, rb) in zip(a, b):
        assert np.array_equal(ca, cb) and pa == pb
        assert (ka is None) == (kb is None) and (ka is None or np.array_equal(ka, kb, equal_nan=True))
        assert ha is not None and np.array_equal(ha, hb)
        assert len(ra) == len(rb) == 9 and all(np.array_equal(u, v) for u, v in zip(ra, rb))


_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import numpy as np, torch
import test_hidden_reach_gpu as T
from frenetix_occlusion import synthetic as SY
sc = T._scenario("scenario1")
sm, obs = T._sensor(sc, memory={{}})
ego, yaw = T._drive(torch, sm, obs, sc, 3)
traj = SY.make_trajectories(64, 31, 0.1, seed=1, ego_pos=ego, ego_yaw=yaw)
for metric in ("euclid", "road"):
    sm.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=T.VEH, v_max=13.9, dt=0.1, metric=metric)
    if sys.argv[1] == "with":
        sm.hidden_clearance(traj["x"], traj["y"], traj["theta"], vehicle=T.VEH, v_cap=13.9, dt=0.1, metric=metric)
torch.cuda.synchronize()
print("child ok")
'''


def _kernel_lines(tmp_path, mode):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_clearance.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"),
                                         tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + mode)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), mode],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    return "\n".join(open(f).read() for f in files).splitlines()


def test_kernel_trace_of_a_process_without_the_clearance(torch_cuda, tmp_path):
    """a drive that calls hidden_reach with both metrics and never the clearance launches none of the clearance's kernels (the
    fo_hc_ kernels and the HrKeyOut instantiation of the column pass); with one clearance call per metric each of them runs
    once per call, next to as many band launches as the reach's own call"""
    lines = _kernel_lines(tmp_path, "without")
    count = lambda k: sum(k in line for line in lines)
    assert count("fo_hc_") == 0 and count("HrKeyOut") == 0
    assert count("fo_hr_rows_kernel") == 2 and count("fo_hr_cols_kernel") == 2 and count("fo_hr_traj_kernel") == 2
    bands = count("fo_hr_road_band_kernel")
    assert bands == 6 and count("fo_hr_road_arrival_kernel") == 1
    lines = _kernel_lines(tmp_path, "with")
    assert count("fo_hc_traj_kernel") == 2 and count("fo_hc_road_merge_kernel") == 1
    assert count("fo_hr_cols_kernel") == 4 and count("HrKeyOut") >= 2 and count("fo_hr_rows_kernel") == 4
    assert count("fo_hr_road_band_kernel") == 2 * bands and count("fo_hr_road_arrival_kernel") == 1
    assert count("fo_hr_traj_kernel") == 2


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_the_c_entry(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, _ = _parked()
    cap = N.HIDDEN_REACH_MAX_HALO
    win = (3, 1, 12, 9)
    cls = np.full((9, 12), 5, dtype=np.uint8)
    x = np.zeros((2, 4))
    head = np.zeros((2, 4, 2))
    head[..., 0] = 1.0

    def refused(what, r2_cap=30, metric="road", **kw):
        rc, msg, out = _raw(torch, sm, cls, win, r2_cap, metric, None, x, x, head, **kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_clearance:") and what in msg, (rc, msg)
        # nothing was launched: no output byte was touched
        assert (out.key == -7).all() and (out.qmin == -7).all() and (out.dist == 7777).all()

    for metric in METRICS:
        rc, msg, out = _raw(torch, sm, cls, win, 30, metric, None, x, x, head)
        assert rc == N.FO_OK and (out.key == 0).all(), msg
    refused("negative", r2_cap=-1)
    refused("FO_HIDDEN_REACH_MAX_HALO", r2_cap=(cap + 1) ** 2)
    rc, msg, _ = _raw(torch, sm, cls, win, (cap + 1) ** 2 - 1, "road", None, x, x, head)      # isqrt = cap exactly: served
    assert rc == N.FO_OK, msg
    refused("metric = 2", metric=2)
    refused("metric = -1", metric=-1)
    refused("T = 0", T=0)
    refused("d_key", d_key=None)
    refused("d_cls", d_cls=None)
    refused("d_x", d_x=None)
    refused("d_x", d_y=None)
    refused("d_heading", d_heading=None)
    refused("d_qmin", d_qmin=None)
    refused("window", win_nx=0)
    refused("window", win_ny=-3)
    refused("window", win_nx=32769)
    refused("M = -1", M=-1)
    refused("half extents", hl=-0.1)
    refused("half extents", hw=float("nan"))
    refused("half extents", hw=64 * sm.cell_size + 0.01)
    refused("half extents", wb=float("nan"))
    rc, msg, _ = _raw(torch, sm, cls, win, 30, "euclid", None, x, x, head, hl=64 * sm.cell_size, hw=0.0)     # the bound itself: served
    assert rc == N.FO_OK, msg
    # M = 0: the map alone, trajectory buffers not needed
    rc, msg, out = _raw(torch, sm, cls, win, 30, "road", None, None, None, None, d_qmin=None)
    assert rc == N.FO_OK and (out.key == 0).all() and (out.dist == 0).all()
    # no parameters, and a context without a map
    import ctypes as C
    assert sm.ctx._lib.fo_scene_hidden_clearance(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert ctx._lib.fo_scene_hidden_clearance(ctx._h, C.byref(N.HiddenClearance()), None) == N.FO_E_STATE
    assert N.load().fo_abi_version() == 12
