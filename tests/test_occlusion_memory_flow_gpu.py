"""The vehicle layer of the occlusion memory on the device (fo_scene_set_occlusion_memory_vehicles, DESIGN.md §5.9 "Vehicle
layer") against the checker of its definition (tests/ref_occlusion_memory_flow.py): hand-armed stages on two opposite lanes with
a one-way connector at every reach / window / previous window at which the kernel takes another path, a one-way lane whose
answer is written down by hand, a table of 0xFF against the road kernel, drives through the one-call step and the stage calls,
the case a user sees (the ego's own lane, seen empty, is not refilled from its far end), the refusals, and the kernels a run
launches.  Every output is an exact integer: all comparisons are ``==``."""
import ctypes as C
import glob
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_hidden_reach as HR
import ref_hidden_reach_flow as RF
import ref_occlusion_memory as OM
import ref_occlusion_memory_flow as VR
import ref_occlusion_memory_road as R
import test_hidden_reach_flow_gpu as FG
import test_hidden_reach_gpu as HG
import test_occlusion_memory_gpu as T
import test_occlusion_memory_road_gpu as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = T.DT
ROAD, EUCLID, VEHICLES = G.ROAD, G.EUCLID, "fo_scene_set_occlusion_memory_vehicles"
FREE = 0xFF


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


# ------------------------------------------------------------------------------------------------ hand-armed stages
def _directed(lid, p0, p1, width, n=41):
    """a straight lanelet from p0 to p1 (the driving direction), `width` wide to the RIGHT of that line"""
    from frenetix_occlusion import scenario as S
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    u = (p1 - p0) / np.linalg.norm(p1 - p0)
    left = p0[None, :] + np.linspace(0.0, 1.0, n)[:, None] * (p1 - p0)[None, :]
    return S.Lanelet(lid, left, left + width * np.array([u[1], -u[0]])[None, :])


def _two_lanes_and_a_connector():
    """the ego's lane y in [-3.5, 0] flowing +x, the oncoming lane y in [0, 3.5] flowing -x, and a one-way side road x in
    [30, 33.5] that leaves the oncoming lane towards +y"""
    return [_directed(1, (-10.0, 0.0), (70.0, 0.0), 3.5), _directed(2, (70.0, 0.0), (-10.0, 0.0), 3.5),
            _directed(3, (30.0, 3.5), (30.0, 20.0), 3.5, n=11)]


def _arm(torch, sm, fn, r2, prev, pw, cells, reset=0):
    from frenetix_occlusion import _native as N
    cur = torch.full((cells,), 7, dtype=torch.uint8, device="cuda")
    m = N.OcclusionMemory(r2=r2, reset=reset, d_cur=cur.data_ptr(), cur_bytes=cur.numel())
    keep = None
    if not reset:
        keep = torch.as_tensor(np.ascontiguousarray(prev, dtype=np.uint8)).cuda().reshape(-1)
        m.prev_ix0, m.prev_iy0, m.prev_nx, m.prev_ny = pw
        m.d_prev, m.prev_bytes = keep.data_ptr(), keep.numel()
    return getattr(sm.ctx._lib, fn)(sm.ctx._h, C.byref(m)), cur, keep


def _launch(torch, sm, ego, r2, prev, pw, win=None, main=ROAD, vehicles=True):
    """one visibility stage with the main memory armed by hand (`main`, previous set `prev` over `pw`) and, on top of it, the
    vehicle layer with the same previous set (the sensor model's own memory is off); win replaces the model's window"""
    from frenetix_occlusion import _native as N
    from frenetix_occlusion.sensor_model import CellWindow
    if win is not None:
        (x0, y0), cs = sm.raster_origin, sm.cell_size
        sm._window_for = lambda ego_pos: CellWindow(x0, y0, cs, *win)
    w = sm._window_for(ego)
    rc, cur_h, keep_h = _arm(torch, sm, main, r2, prev, pw, w.nx * w.ny)
    assert rc == N.FO_OK
    cur_v = None
    if vehicles:
        rc, cur_v, keep_v = _arm(torch, sm, VEHICLES, r2, prev, pw, w.nx * w.ny)
        assert rc == N.FO_OK, sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    sm.launch(np.asarray(ego, dtype=np.float64), 0.0)
    torch.cuda.synchronize()
    n = int(sm.n_occluded.item())
    return dict(cls=sm.cell_class.cpu().numpy().copy(), occ=sm.occluded_idx_buffer[:n].cpu().numpy().copy(), n=n,
                H=cur_h.view(w.ny, w.nx).cpu().numpy(), V=None if cur_v is None else cur_v.view(w.ny, w.nx).cpu().numpy(),
                win=(w.ix0, w.iy0, w.nx, w.ny))


def _same_stage(a, b):
    assert np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["occ"], b["occ"]) and a["n"] == b["n"]
    assert np.array_equal(a["H"], b["H"])


@pytest.fixture(scope="module")
def junction(torch_cuda):
    sm = G._sensor(torch_cuda, _two_lanes_and_a_connector(), (17.0, -2.4), -1.0)
    assert sm.lane_moves is not None
    return sm, sm.road_raster()


@pytest.mark.parametrize("nx", [36, 40, 45])
def test_hand_armed_stages_match_the_checker(torch_cuda, junction, nx):
    """windows that are no multiple of the 32 x 32 tile over the shadow of the parked car, the two lanes and the foot of the
    connector, hanging over the raster's lower edge; r2 = 0 (no round), 17 (n = 4, the small shape), 219 and 247 (n = 16 and 17:
    the switch between the shapes), 853 (n = 31) and 1024 (n = 34, the cap); the previous window the window itself, shifted by
    (-7, +3), and one that overlaps it in part and hangs over the raster's edge.  V is the checker's; class bytes, occluded list, count and H are those
    of the same stage without the layer, and the checker's for the road metric"""
    torch = torch_cuda
    sm, road = junction
    moves = sm.lane_moves
    rny, rnx = road.shape
    assert [R.halo(v) for v in (17, 219, 247, 853, 1024)] == [4, 16, 17, 31, 34]
    ny = {36: 40, 40: 37, 45: 33}[nx]
    cx, cy = G._cell(sm, 12.0, -10.0)
    win = (cx, cy, nx, ny)
    ego = (0.0, -1.0)
    base = G._launch(torch, sm, ego, win=win)
    cls0 = base["cls"]
    occ = (cls0 & 4) != 0
    assert base["win"] == win and occ.sum() > 20 and cy < 0
    rng = np.random.default_rng(11 + nx)
    n_less = 0
    for r2 in (0, 17, 219, 247, 853, 1024):
        for pw in (win, (cx - 7, cy + 3, nx, ny), (cx + 20, -9, 58, 40)):
            prev = G._prev(rng, pw, 0.02 if r2 > 100 else 0.2, road)
            got = _launch(torch, sm, ego, r2, prev, pw)
            off = _launch(torch, sm, ego, r2, prev, pw, vehicles=False)
            _same_stage(got, off)
            H = G._check(got, cls0, road, r2, prev, pw)
            want = VR.step(cls0, win, road, moves, r2, prev, pw)
            assert np.array_equal(got["V"], want), (r2, pw, int((got["V"] != want).sum()))
            assert (want <= H).all()
            n_less += int((want != H).sum())
    assert n_less > 0, "the lanes never changed the answer"


def test_under_the_euclidean_memory_and_on_a_reset(torch_cuda, junction):
    """the layer on top of the disc kernel: the same V, inside the Euclidean H; a reset step copies H of a reset step"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = junction
    cx, cy = G._cell(sm, 12.0, -10.0)
    win = (cx, cy, 45, 33)
    ego = (0.0, -1.0)
    cls0 = G._launch(torch, sm, ego, win=win)["cls"]
    prev = G._prev(np.random.default_rng(3), win, 0.2, road)
    got = _launch(torch, sm, ego, 17, prev, win, main=EUCLID)
    _same_stage(got, _launch(torch, sm, ego, 17, prev, win, main=EUCLID, vehicles=False))
    assert np.array_equal(got["V"], VR.step(cls0, win, road, sm.lane_moves, 17, prev, win)) and (got["V"] <= got["H"]).all()
    cells = win[2] * win[3]
    for main in (ROAD, EUCLID):
        rc, cur_h, _ = _arm(torch, sm, main, 17, None, None, cells, reset=1)
        rc_v, cur_v, _ = _arm(torch, sm, VEHICLES, 17, None, None, cells, reset=1)
        assert rc == N.FO_OK and rc_v == N.FO_OK
        sm.launch(np.asarray(ego), 0.0)
        torch.cuda.synchronize()
        want = VR.step(cls0, win, road, sm.lane_moves, 17)
        assert np.array_equal(cur_v.view(win[3], win[2]).cpu().numpy(), want)
        assert np.array_equal(cur_h.cpu().numpy(), cur_v.cpu().numpy()) and np.array_equal(sm.cell_class.cpu().numpy(), cls0)


def test_a_free_table_gives_the_road_kernel(torch_cuda):
    """a table of 0xFF everywhere and the same previous set: V == H of the road kernel, bit for bit, at both shapes"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm = G._sensor(torch, _two_lanes_and_a_connector(), (17.0, -2.4), -1.0)
    road = sm.road_raster()
    assert FG._set_moves(sm, np.full(road.shape, FREE, dtype=np.uint8)) == N.FO_OK
    cx, cy = G._cell(sm, 12.0, -10.0)
    win = (cx, cy, 45, 37)
    rng = np.random.default_rng(17)
    n_hidden = 0
    for r2 in (17, 247, 1024):
        for pw in (win, (cx - 7, cy + 3, 45, 37)):
            prev = G._prev(rng, pw, 0.02 if r2 > 100 else 0.2, road)
            got = _launch(torch, sm, (0.0, -1.0), r2, prev, pw, win=win)
            assert np.array_equal(got["V"], got["H"]), (r2, pw)
            n_hidden += int(((got["cls"] & 4) != 0).sum())
    assert n_hidden > 0


@pytest.mark.parametrize("sources", ["down", "up"])
def test_one_way_lane_by_hand(torch_cuda, sources):
    """one lane, y in [-3.5, 0], flowing +x; the ego at (0, -1.75) behind a car parked in it at x = 10: the lane's rows behind the
    car are occluded across a window 40 cells long, x in [14, 34].  Inside the previous window nothing was hidden; it ends at the
    window's downstream edge ("down": the road beyond, x >= 34, is a source) or at its upstream edge ("up": the road before it,
    x < 14).  r2 = 17: h = 4, L = 53.  "down": a vehicle there drives away, V = 0 on every occluded cell, while the road kernel
    keeps the last 4 columns (12 |dx| <= 53, dx^2 <= 17).  "up": the lane delivers it, V is the road kernel's H, the first 4"""
    torch = torch_cuda
    sm = G._sensor(torch, [_directed(1, (-10.0, 0.0), (70.0, 0.0), 3.5)], (10.0, -1.75), -1.75)
    road, moves = sm.road_raster(), sm.lane_moves
    ego = (0.0, -1.75)
    cx, cy = G._cell(sm, 14.0, -8.0)
    win = (cx, cy, 40, 24)
    base = G._launch(torch, sm, ego, win=win)
    cls0 = base["cls"]
    occ = ((cls0 & 4) != 0) & ((cls0 & 2) == 0)
    rd = OM.previous_p(road, None, None, win, 0) != 0
    lane_rows = np.flatnonzero(rd.any(axis=1))
    assert len(lane_rows) == 7 and rd[lane_rows].all()
    assert (moves[cy + lane_rows[0]:cy + lane_rows[-1] + 1, cx - 20:cx + 60] == RF.sector(0.0)).all()
    assert occ[lane_rows[3]].all(), "the car's shadow does not cover the lane's centre row across the window"
    pw = (cx - 40, cy - 10, 80, 44) if sources == "down" else (cx, cy - 10, 80, 44)
    prev = np.zeros((pw[3], pw[2]), dtype=np.uint8)
    got = _launch(torch, sm, ego, 17, prev, pw)
    G._check(got, cls0, road, 17, prev, pw)
    assert np.array_equal(got["V"], VR.step(cls0, win, road, moves, 17, prev, pw))
    X = np.broadcast_to(np.arange(40)[None, :], occ.shape)
    if sources == "down":
        assert np.array_equal(got["H"][occ] != 0, X[occ] >= 36) and got["H"][occ].sum() >= 4
        assert not got["V"][occ].any()
    else:
        assert np.array_equal(got["H"][occ] != 0, X[occ] <= 3) and got["H"][occ].sum() >= 4
        assert np.array_equal(got["V"], got["H"])


# ------------------------------------------------------------------------------------------------ drives
def _stack(torch, sc, path, inter, ego, yaw, memory, share):
    """``test_occlusion_memory_gpu._stack`` on the static map of the stack `share` (None: a map of its own), so that the six
    stacks of a drive build the map's host tables once"""
    from types import SimpleNamespace
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.step import PlanningStep
    from frenetix_occlusion.sweep import MetricSweep
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    ctx = N.Context(0)
    obs = FOObstacles(sc.obstacles)
    sm = SensorModel(sc.lanelets, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, ctx=ctx, routes=3, intersections=inter,
                     share_map_with=None if share is None else share.sm)
    if memory is not None:
        sm.enable_occlusion_memory(dt=DT, **memory)
    sl = SpawnLocator(None, path, T.CFG, sm, fo_obstacles=obs, dt=DT, horizon=30 * DT)
    sw = MetricSweep(T.VEH, DT, thresholds={"harm": 0.1, "risk": 1}, ctx=ctx)
    traj = SY.make_trajectories(64, 31, DT, seed=11, ego_pos=ego, ego_yaw=yaw)
    tr = [torch.as_tensor(traj[k]).cuda() for k in ("x", "y", "theta", "v", "a")]
    return SimpleNamespace(ctx=ctx, obs=obs, sm=sm, sl=sl, sw=sw, ps=PlanningStep(sm, sl, sw, *tr, mode="reduced"))


@pytest.mark.parametrize("name", ["scenario1", "city_grid"])
def test_drive_matches_the_checker_on_both_paths(torch_cuda, name):
    """12 steps, rule families on, the timestep advancing by 1 and once by 10 (r2 = 853: the large shape).  At every step V is
    the checker's on the classes of a run without memory -- through the one-call step, through the stage calls, and on top of
    the Euclidean memory --, V lies inside H under either main metric, the reset reasons are the memory's, and everything else
    a step computes (class bytes, occluded list, rule points, costs, H) is that of the same step with the layer off"""
    torch = torch_cuda
    sc, ego0, yaw, path = T._scenario(name)
    inter = getattr(sc, "intersections", None)
    off = _stack(torch, sc, path, inter, ego0[:2], yaw, None, None)
    mk = lambda memory: _stack(torch, sc, path, inter, ego0[:2], yaw, memory, off)
    plain = {m: mk({"metric": m}) for m in ("road", "euclid")}
    fused = {m: mk({"metric": m, "vehicles": "lanes"}) for m in ("road", "euclid")}
    staged = mk({"metric": "road", "vehicles": "lanes"})
    assert fused["road"].sm.occlusion_memory_vehicles == "lanes" and plain["road"].sm.occlusion_memory_vehicles == "off"
    assert plain["road"].sm.occlusion_memory_hidden_vehicles is None
    road, moves = off.sm.road_raster(), off.sm.lane_moves
    model = VR.Memory(13.9, DT, off.sm.cell_size)
    ts = [0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 19, 20]
    r2s, n_less = [], {"road": 0, "euclid": 0}
    for step, t in enumerate(ts):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        run = lambda k, **kw: T._run(torch, k, ego, yaw, float(ego0[3]), step, t, **kw)
        a = run(off)
        w = a["win"]
        r2s.append(model.plan(t)[0])
        V, reason = model.advance(a["cls"], (w.ix0, w.iy0, w.nx, w.ny), road, moves, t)
        s = run(staged, staged=True)
        assert np.array_equal(staged.sm.occlusion_memory_hidden_vehicles, V), step
        for m in ("road", "euclid"):
            p, f = run(plain[m]), run(fused[m])
            assert f["reason"] == p["reason"] == s["reason"] == reason == ("first" if step == 0 else None), (step, m)
            got = fused[m].sm.occlusion_memory_hidden_vehicles
            assert np.array_equal(got, V), (step, m, int((got != V).sum()))
            assert (V <= f["H"]).all(), (step, m)
            T._same(f, p)
            assert np.array_equal(f["H"], p["H"]), (step, m)
            n_less[m] += int((V != f["H"]).sum())
            if m == "road":
                T._same(f, s)
                assert np.array_equal(f["H"], s["H"]), step
            if reason is not None:
                assert np.array_equal(V, f["H"]), step
    assert r2s[1] == 17 and r2s[6] == 853
    print(f"{name}: cells in H and not in V, summed over the drive: road {n_less['road']}, euclid {n_less['euclid']}")


# ------------------------------------------------------------------------------------------------ what a user sees
def _own_lane_scene(torch, vehicles):
    """a straight two-way road, 3.5 m lanes, the ego's flowing +x.  The ego drives along its lane's centre at 0.7634 m per step and
    sees it empty up to the 50 m sensor range on steps 0 .. 2; from step 3 on a parked two-wheeler (2.0 x 0.6 m) stands at
    (14, -1.5), across the ego's line of sight, and the rows of the ego's lane behind it from y = -2 upwards are in its shadow.  Timesteps 0 .. 5, then 15 and 16: the jump
    lets the road memory refill the shadow from the lane's unobserved far end by 29 cells at once.  -> (sm, ego, road)"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    lanes = [_directed(1, (-10.0, 0.0), (110.0, 0.0), 3.5, n=61), _directed(2, (110.0, 0.0), (-10.0, 0.0), 3.5, n=61)]
    sm = SensorModel(lanes, None, sensor_radius=50.0, sensor_angle=360.0, n_rays=720)
    sm.enable_occlusion_memory(dt=DT, metric="road", vehicles=vehicles)
    bike = S.Obstacle(5, "static", "parkedVehicle", 2.0, 0.6, 0, np.array([14.0, -1.5, 0.0, 0.0]), np.zeros((0, 4)))
    obs = FOObstacles([bike])
    obs.update(0)
    ego = None
    for step, t in enumerate([0, 1, 2, 3, 4, 5, 15, 16]):
        ego = np.array([0.7634 * step, -1.75])
        sm.upload_obstacles(obs if step >= 3 else None)
        sm.launch(ego, 0.0, timestep=t)
        assert sm.occlusion_memory_reset_reason == ("first" if step == 0 else None)
    torch.cuda.synchronize()
    return sm, ego, sm.road_raster()


def _candidates(ego):
    """[2, 31] samples at 12 m/s: 0 keeps the ego's lane (and swerves 0.9 m to the right around the two-wheeler), 1 crosses
    into the oncoming lane and stays there"""
    s = 12.0 * DT * np.arange(31)
    x = ego[0] + s
    y0 = -1.75 - 0.9 * np.exp(-((x - 14.0) / 4.0) ** 2)
    y1 = -1.75 + 3.5 / (1.0 + np.exp(-(s - 10.0) / 2.0))
    y = np.stack((y0, y1))
    x = np.stack((x, x))
    theta = np.arctan2(np.gradient(y, axis=1), np.gradient(x, axis=1))
    return x, y, theta


def test_own_lane_seen_empty_is_not_refilled_from_its_far_end(torch_cuda):
    """With the road memory alone the shadowed stretch of the ego's own lane is hidden again after the jump, and the lane flow
    forecast that starts there meets the candidate that keeps the lane (first >= 0).  With vehicles="lanes" the forecast starts
    from V, which holds none of those cells: first == -1, and `from_vehicle_memory` says so.  The candidate that crosses into the
    oncoming lane meets hidden traffic either way.  Everything else of the stage is the same"""
    torch = torch_cuda
    kw = dict(vehicle=HG.VEH, dt=DT, metric="road", flow="lanes")
    res = {}
    for vehicles in ("off", "lanes"):
        sm, ego, road = _own_lane_scene(torch, vehicles)
        x, y, theta = _candidates(ego)
        out = sm.hidden_reach(x, y, theta, v_max=13.9, **kw)
        hc = sm.hidden_clearance(x, y, theta, v_cap=13.9, **kw)
        cls, win, _, H = HG._state(torch, sm)
        V = sm.occlusion_memory_hidden_vehicles
        res[vehicles] = dict(sm=sm, out=out, hc=hc, cls=cls, win=win, H=H, V=V, first=HG._np(out.first), road=road,
                             x=x, y=y)
    off, on = res["off"], res["lanes"]
    assert off["V"] is None and not off["out"].from_vehicle_memory and off["out"].from_memory
    assert on["out"].from_vehicle_memory and on["out"].from_memory and on["hc"].from_vehicle_memory
    # the stage itself is untouched by the layer
    assert np.array_equal(off["cls"], on["cls"]) and np.array_equal(off["H"], on["H"]) and off["win"] == on["win"]
    # the comparison shows something: the road memory did re-hide cells of the ego's lane, behind the two-wheeler and within the
    # candidate's 36 m, and V holds none of them
    sm, win = on["sm"], on["win"]
    cs, (x0, y0) = sm.cell_size, sm.raster_origin
    gx = x0 + (win[0] + np.arange(win[2]) + 0.5) * cs
    gy = y0 + (win[1] + np.arange(win[3]) + 0.5) * cs
    own = (gy[:, None] > -3.5) & (gy[:, None] < 0.0) & (gx[None, :] > 16.0) & (gx[None, :] < on["x"][0, -1])
    rehidden = own & ((on["cls"] & 4) != 0) & (on["H"] != 0)
    print(f"own lane ahead: {int(rehidden.sum())} cells hidden again under the road memory, {int((rehidden & (on['V'] != 0)).sum())} of them in V")
    assert rehidden.sum() > 20 and not (rehidden & (on["V"] != 0)).any()
    assert (on["V"] <= on["H"]).all()
    # the forecast
    assert off["first"][0] >= 0 and on["first"][0] == -1
    assert off["first"][1] >= 0 and on["first"][1] >= 0
    # ... is the checker's on V, and the clearance agrees with it
    A, _, d, _ = RF.arrival_map_flow(on["cls"], win, on["road"], sm.lane_moves, on["out"].r2, on["V"])
    assert np.array_equal(HG._np(on["out"].arrival), A) and np.array_equal(HG._np(on["out"].road_dist), d)
    cells, first, slack = HR.trajectories(A, win, on["road"], sm.raster_origin, cs, on["x"], on["y"], HG._np(on["out"].heading),
                                          HG.HL, HG.HW, HG.WB)
    assert np.array_equal(HG._np(on["out"].cells), cells) and np.array_equal(on["first"], first)
    assert np.array_equal(HG._np(on["out"].slack), slack)
    for r in (off, on):
        hit, first, slack = r["hc"].reach(13.9)
        assert np.array_equal(HG._np(first), r["first"]) and np.array_equal(HG._np(slack), HG._np(r["out"].slack))
        assert np.array_equal(HG._np(hit), HG._np(r["out"].cells) > 0)
    # flow="any" never reads V
    anyflow = sm.hidden_reach(on["x"], on["y"], np.zeros_like(on["x"]), vehicle=HG.VEH, v_max=13.9, dt=DT, metric="road")
    assert anyflow.from_memory and not anyflow.from_vehicle_memory


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_null_and_a_later_main_call(torch_cuda, junction):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = junction
    lib, h = sm.ctx._lib, sm.ctx._h
    cap = N.OCCLUSION_MEMORY_MAX_HALO
    cx, cy = G._cell(sm, 12.0, -10.0)
    win = (cx, cy, 45, 33)
    cells = 45 * 33
    ego = np.array([0.0, -1.0])
    cls0 = G._launch(torch, sm, ego, win=win)["cls"]
    prev = G._prev(np.random.default_rng(9), win, 0.2, road)
    buf = torch.zeros(2 * cells, dtype=torch.uint8, device="cuda")
    a, b = buf.data_ptr(), buf.data_ptr() + cells
    veh = lambda m: lib.fo_scene_set_occlusion_memory_vehicles(h, m)
    msg = lambda: lib.fo_last_error(h).decode()
    ok = lambda **kw: N.OcclusionMemory(**dict(dict(r2=17, reset=0, prev_ix0=win[0], prev_iy0=win[1], prev_nx=45, prev_ny=33,
                                                    d_prev=a, prev_bytes=cells, d_cur=b, cur_bytes=cells), **kw))
    main = lambda **kw: _arm(torch, sm, ROAD, kw.pop("r2", 17), prev, win, cells, **kw)
    assert lib.fo_scene_set_occlusion_memory_vehicles(None, None) == N.FO_E_ARG                     # no context
    fresh = N.Context(0)
    assert fresh._lib.fo_scene_set_occlusion_memory_vehicles(fresh._h, ok()) == N.FO_E_STATE       # no scene
    assert veh(ok()) == N.FO_E_STATE and "main memory" in msg()                                     # the main memory is not armed
    rc, cur_h, keep = main()
    assert rc == N.FO_OK
    assert veh(ok(reset=1)) == N.FO_E_ARG and "reset" in msg()                                      # another reset than the main call's
    assert veh(ok(r2=18)) == N.FO_E_ARG and "above" in msg()                                        # r2 above the main call's
    assert veh(ok(r2=cap * cap + 1)) == N.FO_E_ARG and veh(ok(r2=-1)) == N.FO_E_ARG                 # the "reach" cap
    assert veh(ok(d_cur=None)) == N.FO_E_ARG and veh(ok(cur_bytes=0)) == N.FO_E_ARG
    assert veh(ok(d_prev=None)) == N.FO_E_ARG and veh(ok(d_prev=b)) == N.FO_E_ARG                   # one buffer for both steps
    assert veh(ok(prev_bytes=cells - 1)) == N.FO_E_ARG                                              # previous buffer too small
    assert veh(ok(d_cur=cur_h.data_ptr())) == N.FO_E_ARG                                            # the main memory's own buffer
    # a refused call leaves the layer off and the main memory armed: the stage runs as without the layer
    buf.fill_(9)
    sm.launch(ego, 0.0)
    torch.cuda.synchronize()
    Hr, out = R.step(cls0, win, road, 17, prev, win)
    assert np.array_equal(cur_h.view(33, 45).cpu().numpy(), Hr) and np.array_equal(sm.cell_class.cpu().numpy(), out)
    assert (buf == 9).all()
    # a buffer smaller than the window: the stage refuses, and both armings go with it
    assert main()[0] == N.FO_OK and veh(ok(cur_bytes=8)) == N.FO_OK
    with pytest.raises(N.NativeError) as e:
        sm.launch(ego, 0.0)
    assert e.value.code == N.FO_E_ARG
    assert np.array_equal(G._launch(torch, sm, ego)["cls"], cls0) and (buf == 9).all()
    # NULL disarms the layer alone
    rc, cur_h, keep = main()
    assert veh(ok()) == N.FO_OK and veh(None) == N.FO_OK
    sm.launch(ego, 0.0)
    torch.cuda.synchronize()
    assert np.array_equal(cur_h.view(33, 45).cpu().numpy(), Hr) and (buf == 9).all()
    # a later main arming call drops the layer, through either entry and with NULL
    for again in (ROAD, EUCLID):
        assert main()[0] == N.FO_OK and veh(ok()) == N.FO_OK
        rc, cur_h, keep = _arm(torch, sm, again, 17, prev, win, cells)
        sm.launch(ego, 0.0)
        torch.cuda.synchronize()
        assert (buf == 9).all() and not (cur_h == 7).any()
    assert main()[0] == N.FO_OK and veh(ok()) == N.FO_OK and lib.fo_scene_set_occlusion_memory(h, None) == N.FO_OK
    assert np.array_equal(G._launch(torch, sm, ego)["cls"], cls0) and (buf == 9).all()
    # a smaller reach than the main memory's is fine
    rc, cur_h, keep = main()
    prev_v = torch.as_tensor(prev).cuda().reshape(-1)
    assert veh(ok(r2=5, d_prev=prev_v.data_ptr())) == N.FO_OK
    sm.launch(ego, 0.0)
    torch.cuda.synchronize()
    assert np.array_equal(buf[cells:].view(33, 45).cpu().numpy(), VR.step(cls0, win, road, sm.lane_moves, 5, prev, win))
    # no move table on the map (last: the fixture's map loses its table)
    assert FG._set_moves(sm, None) == N.FO_OK
    assert main()[0] == N.FO_OK
    assert veh(ok()) == N.FO_E_STATE and "move table" in msg()
    assert lib.fo_scene_set_occlusion_memory(h, None) == N.FO_OK
    assert FG._set_moves(sm, sm.lane_moves) == N.FO_OK


def test_python_layer_refuses_a_model_without_a_table(torch_cuda):
    from frenetix_occlusion.scenario import MapGeometry
    from frenetix_occlusion.sensor_model import SensorModel
    geo = MapGeometry.from_lanelets(_two_lanes_and_a_connector())
    sm = SensorModel(geo, None, sensor_radius=50.0, sensor_angle=360.0, n_rays=720)
    assert sm.lane_moves is None
    with pytest.raises(ValueError, match="move table"):
        sm.enable_occlusion_memory(metric="road", vehicles="lanes")
    sm.enable_occlusion_memory(metric="road")
    assert sm.occlusion_memory_vehicles == "off" and sm.occlusion_memory_hidden_vehicles is None


# ------------------------------------------------------------------------------------------------ the kernels a run launches
_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import numpy as np, torch
import test_occlusion_memory_gpu as T
import test_occlusion_memory_road_gpu as G
lanes, _, _ = T._parked_car_scene()
sm = G._sensor(torch, lanes, (17.0, -2.4), -1.0)
sm.enable_occlusion_memory(dt=0.1, metric="road", vehicles=sys.argv[1])
reasons = []
for i, t in enumerate((0, 1, 2, 2, 3)):
    sm.launch(np.array([0.8 * i, -1.0]), 0.0, timestep=t)
    torch.cuda.synchronize()
    reasons.append(str(sm.occlusion_memory_reset_reason))
print("child ok", ",".join(reasons))
'''


def _trace(tmp_path, vehicles):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_vehicles.py"
    child.write_text(_TRACE_CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "frenetix-occlusion_amd"),
                                         tests=os.path.join(ROOT, "tests")))
    d = tmp_path / ("trace_" + vehicles)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), vehicles],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    reasons = r.stdout.split("child ok")[1].split()[0].split(",")
    return "\n".join(open(f).read() for f in files).splitlines(), reasons


def test_kernel_trace_with_and_without_the_layer(torch_cuda, tmp_path):
    """five steps, the fourth with a timestep that does not advance: a run with the layer off launches no
    fo_occlusion_memory_flow kernel; a run with it on launches exactly one per step, reset steps included (no step is skipped
    here), next to the main memory's unchanged launches"""
    lines, reasons = _trace(tmp_path, "off")
    count = lambda k: sum(k in line for line in lines)
    assert reasons == ["first", "None", "None", "time", "None"]
    assert count("fo_occlusion_memory_flow") == 0
    assert count("fo_occlusion_memory_road_kernel") == 3 and count("fo_occlusion_memory_kernel") == 2
    lines, reasons = _trace(tmp_path, "lanes")
    assert reasons == ["first", "None", "None", "time", "None"]
    assert count("fo_occlusion_memory_flow") == 5
    assert count("fo_occlusion_memory_road_kernel") == 3 and count("fo_occlusion_memory_kernel") == 2
