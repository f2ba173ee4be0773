"""Road metric of the hidden-traffic reach forecast on the device (fo_scene_hidden_reach_road, DESIGN.md §5.10 "Road metric")
against the heap-Dijkstra statement of its definition (tests/ref_hidden_reach_road.py).  Every output is an exact integer: all
comparisons are ``==``."""
import glob
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_reach as HR
import ref_hidden_reach_road as RR
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DT, VEH, HL, HW, WB = T.DT, T.VEH, T.HL, T.HW, T.WB
_np = T._np
TILE, BAND = 32, 192           # the band kernel's tile edge and band width (12 x its halo of 16)


def _raw_road(torch, sm, cls, win, r2, hidden=None, x=None, y=None, head=None, lens=None, hl=HL, hw=HW, wb=WB, T_=None,
              dist=True, **over):
    """fo_scene_hidden_reach_road with class bytes / windows / tables of the test's own; returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_cls, d_hid = up(cls, np.uint8), up(hidden, np.uint8)
    M = 0 if x is None else x.shape[0]
    Tn = (1 if x is None else x.shape[1]) if T_ is None else T_
    tx, ty, th, tl = up(x, np.float64), up(y, np.float64), up(head, np.float64), up(lens, np.int32)
    arrival = torch.full((win[3], win[2]), 77, dtype=torch.uint8, device=dev)
    d_dist = torch.full((win[3], win[2]), 7777, dtype=torch.int16, device=dev)      # (the bytes of a uint16 map)
    cells = torch.full((M, Tn), -7, dtype=torch.int32, device=dev)
    first = torch.full((M,), -7, dtype=torch.int32, device=dev)
    slack = torch.full((M,), -7, dtype=torch.int32, device=dev)
    r2 = np.ascontiguousarray(r2, dtype=np.int32)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=hl, hw=hw, wb=wb, J=len(r2),
              h_r2=r2.ctypes.data_as(C.POINTER(C.c_int32)), d_cls=p(d_cls), d_hidden_or_null=p(d_hid), win_ix0=win[0],
              win_iy0=win[1], win_nx=win[2], win_ny=win[3], d_arrival=arrival.data_ptr(), d_cells=p(cells), d_first=p(first),
              d_slack=p(slack))
    kw.update(over)
    args = N.HiddenReachRoad(base=N.HiddenReach(**kw), d_dist_or_null=d_dist.data_ptr() if dist else None)
    rc = sm.ctx._lib.fo_scene_hidden_reach_road(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(arrival=_np(arrival), dist=_np(d_dist).view(np.uint16), cells=_np(cells), first=_np(first),
                                    slack=_np(slack))


def _parked():
    lanes, obstacles, _ = T._parked_car_scene()
    sm, _ = T._sensor(lanes, obstacles)
    return sm, sm.road_raster()


# ------------------------------------------------------------------------------------------------ raw entry
def test_random_class_maps_windows_and_poses(torch_cuda):
    """40 seeded random class maps on the parked-car map: windows of one cell, one row, one column, exactly one tile, a tile and
    a cell, several tiles, hanging over every edge of the raster; a hidden mask in half of the cases; reaches from 0 to the cap"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    rng = np.random.default_rng(20240131)
    cap = N.HIDDEN_REACH_MAX_HALO
    halos = [0, 1, 3, 13, 34, 64, 65, cap]
    shapes = [(1, 1), (1, 37), (41, 1), (TILE, TILE), (TILE + 1, TILE + 1), (TILE, TILE + 1), (97, 70), (70, 45)]
    edges, later, seen_bands = set(), 0, set()
    for case in range(40):
        h = halos[case % len(halos)]
        nx, ny = shapes[(case // len(halos) + case) % len(shapes)]
        if h > 60:
            nx, ny = min(nx, 24), min(ny, 24)
        corner = case % 5            # the four edges of the raster in turn, then anywhere
        ix0 = [-nx // 2, rnx - (nx + 1) // 2, int(rng.integers(0, max(rnx - nx, 1))), int(rng.integers(0, max(rnx - nx, 1))),
               int(rng.integers(-nx + 1, rnx))][corner]
        iy0 = [int(rng.integers(-1, 3)), int(rng.integers(-1, 3)), -ny // 2, rny - (ny + 1) // 2, int(rng.integers(-ny + 1, rny))][corner]
        win = (ix0, iy0, nx, ny)
        edges |= {e for e, over in zip("lrbt", (ix0 < 0, ix0 + nx > rnx, iy0 < 0, iy0 + ny > rny)) if over}
        cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx), p=[0.12, 0.04, 0.6, 0.03, 0.03, 0.18])
        hidden = (rng.random((ny, nx)) < 0.02).astype(np.uint8) if case % 2 else None
        if hidden is not None and h > 60:                 # two sources alone: distances of several bands in a small window
            hidden[:] = 0
            hidden.ravel()[rng.integers(0, nx * ny, 2)] = 1
        J = [1, 31, 254, 7][case % 4]
        top = int(rng.integers(h * h, (h + 1) * (h + 1)))
        r2 = np.sort(rng.integers(0, top + 1, J))
        r2[-1] = top
        Tn = min([1, 31, J][case % 3], J)
        M = [37, 70, 1, 129][case % 4]
        x, y, head = T._random_poses(rng, sm, win, M, Tn)
        lens = rng.integers(-1, Tn + 2, M).astype(np.int32) if case % 2 else None
        rc, msg, out = _raw_road(torch, sm, cls, win, r2, hidden, x, y, head, lens, dist=case % 7 != 6)
        assert rc == 0, msg
        A, A_e, d, L = RR.arrival_map_road(cls, win, road, r2, hidden)
        if case % 7 != 6:
            assert np.array_equal(out.dist, d), (case, h, win, int((out.dist != d).sum()))
        else:
            assert (out.dist == 7777).all()               # no buffer handed in: the distances stay in the context
        assert np.array_equal(out.arrival, A), (case, h, win)
        cells, first, slack = HR.trajectories(A, win, road, sm.raster_origin, sm.cell_size, x, y, head, HL, HW, WB, lens)
        assert np.array_equal(out.cells, cells), case
        assert np.array_equal(out.first, first) and np.array_equal(out.slack, slack), case
        later += int((A > A_e).sum())
        seen_bands.add(max(-(-int(L[-1]) // BAND), 1))
    assert edges == set("lrbt") and later > 0 and {1, 18} <= seen_bands


def test_serpentine(torch_cuda):
    """walls in every second column, their gaps alternately at the bottom and at the top, one source in a corner: the only path
    runs up and down the columns and crosses the border between the tiles in every one of them"""
    torch = torch_cuda
    sm, road = _parked()
    rny, rnx = road.shape
    n = 40
    cls = np.full((n, n), 3, dtype=np.uint8)
    for c in range(1, n, 2):
        cls[:, c] = 2
        cls[n - 1 if c % 4 == 1 else 0, c] = 3
    cls[0, 0] = 5
    win = (rnx + 7, rny + 3, n, n)                        # off the raster: nothing outside the window is a source
    r2 = [0, 100, 2500, 10000, 40000, 254 ** 2]
    A, A_e, d, L = RR.arrival_map_road(cls, win, road, r2)
    assert L[-1] == 13 * 254 and L[-1] >= 4 * BAND
    is_road = (cls & 1) != 0
    assert (A[is_road] != 255).any() and (A[is_road] == 255).any() and (A[is_road] > A_e[is_road]).any()
    assert d[n - 1, 1] == (n - 2) * 12 + 17               # down the first column, diagonally into the gap
    rc, msg, out = _raw_road(torch, sm, cls, win, r2)
    assert rc == 0, msg
    assert np.array_equal(out.dist, d), int((out.dist != d).sum())
    assert np.array_equal(out.arrival, A)


# ------------------------------------------------------------------------------------------------ scenarios
def _check(torch, sm, out, x, y, hidden="auto"):
    cls, win, road, hid = T._state(torch, sm)
    if hidden != "auto":
        hid = hidden
    assert out.metric == "road" and out.from_memory == (hid is not None)
    A, A_e, d, L = RR.arrival_map_road(cls, win, road, out.r2, hid)
    assert np.array_equal(out.reach, L) and out.reach.dtype == np.int32
    got_d = _np(out.road_dist)
    assert got_d.dtype == np.uint16 and np.array_equal(got_d, d), f"{int((got_d != d).sum())} distances differ"
    assert np.array_equal(_np(out.arrival), A), f"{int((_np(out.arrival) != A).sum())} cells of the arrival map differ"
    cells, first, slack = HR.trajectories(A, win, road, sm.raster_origin, sm.cell_size, x, y, _np(out.heading), HL, HW, WB)
    assert np.array_equal(_np(out.cells), cells)
    assert np.array_equal(_np(out.first), first) and np.array_equal(_np(out.slack), slack)
    return A, A_e, cls


def _scenario_case(torch, sc, memory, steps, start=None):
    """a drive of `steps` stages from `start` (default: the scenario's initial pose), then the road and the euclid call on that
    state with the bench's synthetic fan (T = 31 = J, M not a multiple of 64), everything against the checker; returns the number
    of road cells that arrive later along the road"""
    from frenetix_occlusion import synthetic as SY
    sm, obs = T._sensor(sc, memory=memory)
    ego, yaw = T._drive(torch, sm, obs, sc if start is None else SimpleNamespace(ego_initial=start), steps)
    if memory is not None:
        assert sm.occlusion_memory_reset_reason is None       # the last step was a memory step, not a reset
    traj = SY.make_trajectories(203, 31, DT, seed=20240131, ego_pos=ego, ego_yaw=yaw)
    out = sm.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=VEH, v_max=13.9, dt=DT, metric="road")
    A, A_e, cls = _check(torch, sm, out, traj["x"], traj["y"])
    eu = sm.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=VEH, v_max=13.9, dt=DT, metric="euclid")
    assert eu.metric == "euclid" and eu.road_dist is None and np.array_equal(eu.reach, out.reach)
    got_e = _np(eu.arrival)
    assert np.array_equal(got_e, A_e) and (_np(out.arrival) >= got_e).all()
    later = int(((A > A_e) & ((cls & 1) != 0)).sum())
    print(f"memory={memory} steps={steps} ego={np.round(ego, 2)}: {later} road cells arrive later along the road, "
          f"{int(((A == 255) & (A_e != 255)).sum())} cells never")
    return later


@pytest.mark.parametrize("name", ["scenario1", "scenario2", "scenario3", "city_grid"])
@pytest.mark.parametrize("memory", [False, True])
def test_scenarios_match_the_checker(torch_cuda, name, memory):
    torch = torch_cuda
    sc = T._scenario(name)
    later = _scenario_case(torch, sc, {} if memory else None, 5 if memory else 1)
    if name == "city_grid" and later == 0:
        # After a few steps the memory's hidden set has grown into the occluded cells of the blocks next to hidden road, and
        # those are sources: at the drive's pose the CHECKER finds no road cell that arrives later.  The metrics differ at the
        # corner of a block while the hidden set is still thin: poses beside the block before the central intersection, taken
        # in this order until the checker says that one does (the device is compared with it at every one of them).
        ego0 = np.asarray(sc.ego_initial, dtype=np.float64)
        corner = ego0 + np.array([8.0, 0.0, 0.0, 0.0])           # 12 m before the intersection's centre, 5 m before the corner
        for mem, steps, start in (({}, 2, None), ({}, 2, corner), ({"v_max": 2.0}, 5, corner), ({"v_max": 2.0}, 5, None)):
            later = _scenario_case(torch, sc, mem, steps, start)
            if later:
                break
    if name == "city_grid":
        assert later > 0                                      # road behind a block does not arrive through the block


def test_open_road_equals_euclid_on_the_device(torch_cuda):
    torch = torch_cuda
    sm, road = _parked()
    rows, cols = np.flatnonzero(road.any(axis=1)), np.flatnonzero(road.any(axis=0))
    assert len(rows) >= 10 and len(cols) >= 100 and (np.diff(rows) == 1).all() and (np.diff(cols) == 1).all()
    # the raster's road is this one rectangle: every passable cell, inside the window or not, lies in it
    assert road.sum() == len(rows) * len(cols)
    rng = np.random.default_rng(11)
    win = (int(cols[0]) + 9, int(rows[0]) + 1, 90, len(rows) - 2)
    cls = rng.choice(np.array([1, 3, 5], dtype=np.uint8), (win[3], win[2]), p=[0.01, 0.98, 0.01])
    r2 = HR.reach_table(13.9, DT, math.sqrt(2.0) * sm.cell_size, sm.cell_size, 31)
    x, y, head = T._random_poses(rng, sm, win, 70, 31)
    rc, msg, a = _raw_road(torch, sm, cls, win, r2, None, x, y, head)
    assert rc == 0, msg
    rc, msg, b = T._raw(torch, sm, cls, win, r2, None, x, y, head)
    assert rc == 0, msg
    assert ((a.arrival > 0) & (a.arrival < 255)).any()
    for k in ("arrival", "cells", "first", "slack"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_interface_end_to_end(torch_cuda, tmp_path):
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    lanes, obstacles, path = T._parked_car_scene(17.0, -1.9)
    fo = T._interface(tmp_path, lanes, obstacles, path, (0.0, 1.0), memory=True)
    traj = SY.make_trajectories(70, 31, DT, seed=4, ego_pos=(0.0, 1.0), ego_yaw=0.0)
    for step in range(4):
        fo.evaluate_scenario({}, np.array([0.8 * step, 1.0]), 0.0, (0.8 * step, 0.0), 8.0, step, None)
    with pytest.raises(ValueError, match="metric"):
        fo.hidden_reach(traj, metric="manhattan")
    out = fo.hidden_reach(traj, metric="road")
    assert out.from_memory
    _check(torch, fo.sensor_model, out, np.asarray(traj["x"]), np.asarray(traj["y"]))
    assert fo.hidden_reach(traj).metric == "euclid"


# ------------------------------------------------------------------------------------------------ the kernels of a call
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
out = sm.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=T.VEH, v_max=13.9, dt=0.1, metric=sys.argv[1])
torch.cuda.synchronize()
print("child ok", int(out.reach[-1]))
'''


def _trace(tmp_path, mode):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_road.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"),
                                         tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + mode)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), mode],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    reach = int(r.stdout.split("child ok")[1].split()[0])
    return "\n".join(open(f).read() for f in files).splitlines(), reach


def test_kernel_trace_of_the_two_metrics(torch_cuda, tmp_path):
    """a drive with one euclid call launches none of the road kernels; with one road call the distance bands the reach asks for,
    one merge, and the three kernels of the Euclidean call once each"""
    lines, _ = _trace(tmp_path, "euclid")
    count = lambda k: sum(k in line for line in lines)
    assert count("fo_hr_road_") == 0
    assert count("fo_hr_rows_kernel") == 1 and count("fo_hr_cols_kernel") == 1 and count("fo_hr_traj_kernel") == 1
    lines, reach = _trace(tmp_path, "road")
    assert count("fo_hr_road_band_kernel") == -(-reach // BAND) == 6
    assert count("fo_hr_road_arrival_kernel") == 1
    assert count("fo_hr_rows_kernel") == 1 and count("fo_hr_cols_kernel") == 1 and count("fo_hr_traj_kernel") == 1


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
    ok_r2 = [2, 2, 8, 30]

    def refused(what, r2=ok_r2, **kw):
        rc, msg, out = _raw_road(torch, sm, cls, win, r2, None, x, x, head, **kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_reach_road:") and what in msg, (rc, msg)
        # nothing was launched: no output byte was touched
        assert (out.arrival == 77).all() and (out.cells == -7).all() and (out.first == -7).all() and (out.slack == -7).all()
        assert (out.dist == 7777).all()

    rc, msg, out = _raw_road(torch, sm, cls, win, ok_r2, None, x, x, head)
    assert rc == N.FO_OK and (out.arrival == 0).all() and (out.dist == 0).all()
    refused("J = 0", J=0)
    refused("J = 255", r2=np.arange(255))
    refused("T = 4", r2=[2, 2, 8])                                   # T > J
    refused("T = 0", T=0)
    refused("decreases", r2=[2, 9, 8, 30])
    refused("negative", r2=[-1, 2, 8, 30])
    refused("FO_HIDDEN_REACH_MAX_HALO", r2=[2, 2, 8, (cap + 1) ** 2])
    rc, msg, _ = _raw_road(torch, sm, cls, win, [2, 2, 8, (cap + 1) ** 2 - 1], None, x, x, head)    # isqrt = cap exactly: served
    assert rc == N.FO_OK, msg
    refused("h_r2", h_r2=None)
    refused("d_arrival", d_arrival=None)
    refused("d_cls", d_cls=None)
    refused("d_x", d_x=None)
    refused("d_x", d_y=None)
    refused("d_heading", d_heading=None)
    refused("d_cells", d_cells=None)
    refused("d_cells", d_first=None)
    refused("d_cells", d_slack=None)
    refused("window", win_nx=0)
    refused("window", win_ny=-3)
    refused("M = -1", M=-1)
    refused("half extents", hl=-0.1)
    refused("half extents", hw=float("nan"))
    refused("half extents", hl=float("inf"))
    refused("half extents", hw=64 * sm.cell_size + 0.01)
    refused("half extents", wb=float("nan"))
    rc, msg, _ = _raw_road(torch, sm, cls, win, ok_r2, None, x, x, head, hl=64 * sm.cell_size, hw=0.0)     # the bound itself: served
    assert rc == N.FO_OK, msg
    # M = 0: the maps alone, trajectory buffers not needed
    rc, msg, out = _raw_road(torch, sm, cls, win, ok_r2, None, None, None, None, d_cells=None, d_first=None, d_slack=None)
    assert rc == N.FO_OK and (out.arrival == 0).all() and (out.dist == 0).all()
    # no parameters, and a context without a map
    import ctypes as C
    assert sm.ctx._lib.fo_scene_hidden_reach_road(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert ctx._lib.fo_scene_hidden_reach_road(ctx._h, C.byref(N.HiddenReachRoad()), None) == N.FO_E_STATE
