"""Occlusion memory on the device (fo_scene_set_occlusion_memory) against the NumPy model of its definition
(tests/ref_occlusion_memory.py): drives over scenario 1 and the city grid through both the one-call step and the stage calls,
reset steps bit-identical to a run without memory, a parked car the ego drives up to, and the argument checks."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ref_occlusion_memory as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = {"spawn_locator": {"spawn_points_behind_turn": True, "spawn_point_behind_static_obstacle": True,
                         "spawn_point_behind_dynamic_obstacle": True, "max_static_spawn_points": 1,
                         "max_dynamic_spawn_points": 1},
       "agent_manager": {"pedestrian": {"width": 0.5, "length": 0.3, "default_velocity": 1.4},
                         "bicycle": {"width": 0.9, "length": 2.0, "default_velocity": 5.0},
                         "car": {"width": 2.0, "length": 4.8, "default_velocity": 10.0},
                         "truck": {"width": 2.5, "length": 9.0, "default_velocity": 8.0},
                         "prediction": {"variance_factor": 1.05, "size_factor_length_s": 1.2, "size_factor_width_s": 1.3,
                                        "size_factor_length_l": 1.4, "size_factor_width_l": 2.5}},
       "accelerator": {"spawn": {"mode": "both", "routes": 3, "max_rule_points": 8, "max_agents": 6}}}
VEH = (4.508, 1.610, 1.4227, 1093.3, 11.5)
DT = 0.1


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


def _stack(torch, lanelets, obstacles, path, intersections, ego, yaw, memory=None, M=64, T=31):
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.step import PlanningStep
    from frenetix_occlusion.sweep import MetricSweep
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    ctx = N.Context(0)
    obs = FOObstacles(obstacles)
    sm = SensorModel(lanelets, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, ctx=ctx, routes=3,
                     intersections=intersections)
    if memory is not None:
        sm.enable_occlusion_memory(dt=DT, **memory)
    sl = SpawnLocator(None, path, CFG, sm, fo_obstacles=obs, dt=DT, horizon=(T - 1) * DT)
    sw = MetricSweep(VEH, DT, thresholds={"harm": 0.1, "risk": 1}, ctx=ctx)
    traj = SY.make_trajectories(M, T, DT, seed=11, ego_pos=ego, ego_yaw=yaw)
    tr = [torch.as_tensor(traj[k]).cuda() for k in ("x", "y", "theta", "v", "a")]
    return SimpleNamespace(ctx=ctx, obs=obs, sm=sm, sl=sl, sw=sw, ps=PlanningStep(sm, sl, sw, *tr, mode="reduced"))


def _run(torch, k, ego, yaw, v, t_obst, timestep, staged=False):
    k.obs.update(t_obst)
    k.sm.upload_obstacles(k.obs)
    if staged:
        os.environ["FO_STEP_STAGES"] = "1"
    try:
        out = k.ps.run(ego, yaw, v, timestep=timestep)
    finally:
        os.environ.pop("FO_STEP_STAGES", None)
    torch.cuda.synchronize()
    b = k.sl.batch
    n_occ = int(k.sm.n_occluded.item())
    return dict(cls=k.sm.cell_class.cpu().numpy().copy(), occ=k.sm.occluded_idx_buffer[:n_occ].cpu().numpy().copy(),
                rule=b.rule_points.cpu().numpy().copy(), rule_n=int(b.rule_n.item()), cost=out.cost.cpu().numpy().copy(),
                H=None if k.sm.occlusion_memory_hidden is None else k.sm.occlusion_memory_hidden.copy(),
                reason=k.sm.occlusion_memory_reset_reason, win=k.sm.window)


def _same(a, b, keys=("cls", "occ", "rule", "rule_n", "cost")):
    for key in keys:
        if key == "cost":
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        elif key == "rule":      # (rows past the count are left over from earlier steps)
            assert np.array_equal(a[key][:a["rule_n"]], b[key][:b["rule_n"]], equal_nan=True), key
        else:
            assert np.array_equal(a[key], b[key]), key


def _scenario(name):
    from frenetix_occlusion import scenario as S
    if name == "scenario1":
        sc = S.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    else:
        sc = S.synthetic_urban_grid()
    ego0 = np.asarray(sc.ego_initial, dtype=np.float64)
    yaw = float(ego0[2])
    path = ego0[None, :2] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    return sc, ego0, yaw, path


@pytest.mark.parametrize("name", ["scenario1", "city_grid"])
def test_drive_matches_the_model_on_both_paths(torch_cuda, name):
    """42 steps; timestep 20 goes backwards (a "time" reset), step 30 follows reset_occlusion_memory() ("explicit"): at
    every step the device's H and masked classes equal the model's on the classes of a run without memory, the one-call
    step equals the stage calls, and a reset step equals the run without memory in every output"""
    torch = torch_cuda
    sc, ego0, yaw, path = _scenario(name)
    inter = getattr(sc, "intersections", None)
    off = _stack(torch, sc.lanelets, sc.obstacles, path, inter, ego0[:2], yaw)
    fused = _stack(torch, sc.lanelets, sc.obstacles, path, inter, ego0[:2], yaw, memory={})
    staged = _stack(torch, sc.lanelets, sc.obstacles, path, inter, ego0[:2], yaw, memory={})
    road = off.sm.road_raster()
    model = R.Memory(13.9, DT, off.sm.cell_size)
    ts = list(range(42))
    ts[20] = 18
    n_cleared, n_mem = 0, 0
    for step, t in enumerate(ts):
        if step == 30:
            fused.sm.reset_occlusion_memory()
            staged.sm.reset_occlusion_memory()
            model.reset()
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        a = _run(torch, off, ego, yaw, float(ego0[3]), step, t)
        f = _run(torch, fused, ego, yaw, float(ego0[3]), step, t)
        s = _run(torch, staged, ego, yaw, float(ego0[3]), step, t, staged=True)
        assert a["H"] is None and a["reason"] is None
        w = f["win"]
        H, out, reason = model.advance(a["cls"], (w.ix0, w.iy0, w.nx, w.ny), road, t)
        assert f["reason"] == s["reason"] == reason, step
        assert reason == {0: "first", 20: "time", 30: "explicit"}.get(step), step
        assert np.array_equal(f["H"], H) and np.array_equal(s["H"], H), step
        assert np.array_equal(f["cls"], out), step
        assert np.array_equal(f["occ"], np.flatnonzero(out.reshape(-1) & 4)), step
        _same(f, s)
        if reason is not None:
            _same(f, a)
        else:
            n_mem += 1
            n_cleared += int(((a["cls"] & 4) != 0).sum() - ((f["cls"] & 4) != 0).sum())
    assert n_mem >= 38
    if name == "city_grid":      # (on scenario 1's first 42 steps no seen cell falls into a shadow beyond the reach)
        assert n_cleared > 0, "the drive never cleared an occluded cell"


def test_memory_off_is_the_plain_step(torch_cuda):
    """a stack whose memory was switched on and off again (and the context's arming cleared with NULL) computes what a
    stack that never heard of it computes"""
    torch = torch_cuda
    sc, ego0, yaw, path = _scenario("scenario1")
    a = _stack(torch, sc.lanelets, sc.obstacles, path, sc.intersections, ego0[:2], yaw)
    b = _stack(torch, sc.lanelets, sc.obstacles, path, sc.intersections, ego0[:2], yaw, memory={})
    b.sm.enable_occlusion_memory(False)
    b.ctx._check(b.ctx._lib.fo_scene_set_occlusion_memory(b.ctx._h, None))
    for step in (0, 1, 2, 8, 9):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        ra = _run(torch, a, ego, yaw, float(ego0[3]), step, step)
        rb = _run(torch, b, ego, yaw, float(ego0[3]), step, step)
        _same(ra, rb)
        assert rb["H"] is None and rb["reason"] is None


def _parked_car_scene(car_y=-2.4, path_y=-1.0):
    from frenetix_occlusion import scenario as S

    def straight(lid, y_lo, y_hi, n=41):
        xs = np.linspace(-10, 70, n)
        return S.Lanelet(lid, np.stack((xs, np.full(n, y_hi)), -1), np.stack((xs, np.full(n, y_lo)), -1))
    lanes = [straight(1, -3.5, 0.0), straight(2, 0.0, 3.5)]
    path = np.stack((np.linspace(-5, 65, 141), np.full(141, path_y)), -1)
    car = S.Obstacle(77, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([17.0, car_y, 0.0, 0.0]), np.zeros((0, 4)))
    return lanes, [car], path


def test_parked_car_cells_seen_stay_free_and_rules_follow_the_masked_classes(torch_cuda):
    """the ego passes a car parked in the next lane at 8 m/s (stage calls: calc_visible_and_occluded_area +
    find_spawn_points): the near edge of the car's shadow sweeps over road the ego saw on the step before, and with a reach
    of zero (v_max 0, margin 0: R2 = 0) none of those cells is occluded; the model agrees at every step, and the device rule
    points are the checker's (oracle/fo_spawn_rules_ref.py) on the masked classes"""
    torch = torch_cuda
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    from oracle.fo_spawn_rules_ref import CellView, SpawnRules
    lanes, obstacles, path = _parked_car_scene(car_y=-1.9, path_y=1.0)
    cs = PolylineCS(path)
    cfg = {k: v for k, v in CFG.items() if k != "accelerator"}

    def stack(memory):
        obs = FOObstacles(obstacles)
        sm = SensorModel(lanes, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720)
        if memory:
            sm.enable_occlusion_memory(v_max=0.0, margin=0.0, dt=DT)
        am = SimpleNamespace(scenario=SimpleNamespace(intersections=[]))
        return obs, sm, SpawnLocator(am, path, cfg, sm, fo_obstacles=obs)

    def lane_yaw_at(xy):
        sm = off[1]
        (x0, y0), (nx, ny) = sm.raster_origin, sm.raster_dims
        ix, iy = int(math.floor((xy[0] - x0) / sm.cell_size)), int(math.floor((xy[1] - y0) / sm.cell_size))
        if not (0 <= ix < nx and 0 <= iy < ny) or np.isnan(sm.lane_yaw[iy, ix]):
            return None
        return float(sm.lane_yaw[iy, ix])

    def lanelet_of(xy):
        for ll in lanes:
            if S.points_in_polygon(np.asarray(xy, float).reshape(1, 2), ll.polygon)[0]:
                return ll
        return None
    off, on = stack(False), stack(True)
    road = off[1].road_raster()
    model = R.Memory(0.0, DT, off[1].cell_size, margin=0.0)
    prev_off, seen_then_hidden, cleared = None, 0, 0
    for step in range(20):
        ego = np.array([0.8 * step, 1.0])
        ego_cl = cs.convert_to_curvilinear_coords(ego[0], ego[1])
        res = []
        for obs, sm, sl in (off, on):
            obs.update(0)
            sm.calc_visible_and_occluded_area(step, ego, 0.0, obs)
            pts = list(sl.find_spawn_points(ego, 0.0, ego_cl, 8.0))
            torch.cuda.synchronize()
            res.append((sm.cell_class.cpu().numpy().copy(), pts, sm.window))
        (c_off, p_off, w), (c_on, p_on, _) = res
        H, out, reason = model.advance(c_off, (w.ix0, w.iy0, w.nx, w.ny), road, step)
        assert np.array_equal(c_on, out) and np.array_equal(on[1].occlusion_memory_hidden, H), step
        if prev_off is not None:
            # the previous step's visible cells in this step's window (windows follow the ego)
            pc, pw = prev_off
            was_seen = np.zeros_like(c_off, dtype=bool)
            dx, dy = w.ix0 - pw.ix0, w.iy0 - pw.iy0
            ys, xs = np.mgrid[0:w.ny, 0:w.nx]
            ok = (ys + dy >= 0) & (ys + dy < pw.ny) & (xs + dx >= 0) & (xs + dx < pw.nx)
            was_seen[ok] = (pc[(ys + dy)[ok], (xs + dx)[ok]] & 2) != 0
            newly = ((c_off & 4) != 0) & was_seen
            seen_then_hidden += int(newly.sum())
            cleared += int((((c_on & 4) == 0) & newly).sum())
            assert not (((c_on & 4) != 0) & newly).any(), step      # R2 = 0: only cells hidden before stay hidden
        prev_off = (c_off, w)
        # the rule families on the masked classes: the checker's points
        view = CellView(c_on, w)
        rules = SpawnRules(cfg, path, cs, lane_yaw_at, lanelet_of, on[0], lanelets=lanes, intersections=[])
        ref = rules.find(view, ego, ego_cl, 8.0, 0.0)
        assert [(p.agent_type, p.source) for p in p_on] == [(p.agent_type, p.source) for p in ref], step
        for a, b in zip(p_on, ref):
            np.testing.assert_allclose(a.position, b.position, rtol=0, atol=1e-9)
    assert seen_then_hidden > 0, "the shadow never took in a cell seen on the step before"
    assert cleared > 0, "no cell seen on the step before was kept out of the occluded area"


def test_argument_checks_and_backward_time(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    lanes, obstacles, path = _parked_car_scene()
    k = _stack(torch, lanes, obstacles, path, None, np.array([0.0, -1.0]), 0.0, memory={})
    buf = torch.zeros(8, dtype=torch.uint8, device="cuda")
    call = lambda m: k.ctx._lib.fo_scene_set_occlusion_memory(k.ctx._h, m)
    cap = N.OCCLUSION_MEMORY_MAX_HALO
    assert call(N.OcclusionMemory(r2=cap * cap + 1, reset=1, d_cur=buf.data_ptr(), cur_bytes=8)) == N.FO_E_ARG
    assert call(N.OcclusionMemory(r2=-1, reset=1, d_cur=buf.data_ptr(), cur_bytes=8)) == N.FO_E_ARG
    assert call(N.OcclusionMemory(r2=4, reset=0, prev_nx=4, prev_ny=4, d_prev=buf.data_ptr(), prev_bytes=8,
                                  d_cur=buf.data_ptr() + 4, cur_bytes=4)) == N.FO_E_ARG          # previous buffer too small
    assert call(N.OcclusionMemory(r2=cap * cap, reset=1, d_cur=buf.data_ptr(), cur_bytes=8)) == N.FO_OK
    # armed with an 8-byte buffer: the next visibility stage refuses the window ... (the sensor model's own memory off, so
    # that it does not arm the context itself)
    k.sm.enable_occlusion_memory(False)
    with pytest.raises(N.NativeError) as e:
        k.sm.launch(np.array([0.0, -1.0]), 0.0)
    assert e.value.code == N.FO_E_ARG
    # ... and the arming went with it
    k.sm.launch(np.array([0.0, -1.0]), 0.0)
    assert call(None) == N.FO_OK
    # timesteps going backwards: a reset, not an error
    k.sm.enable_occlusion_memory(True, dt=DT)
    ego, v = np.array([0.0, -1.0]), 8.0
    r = [_run(torch, k, ego + [0.8 * i, 0.0], 0.0, v, 0, t)["reason"] for i, t in enumerate((5, 6, 4, 5, 5))]
    assert r == ["first", None, "time", None, "time"]
