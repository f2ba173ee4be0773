"""``accelerator.spawn.frame: caller`` on the device: the rule families project through a table sampled from the caller's
frame object (csrc/fo_spawn_rules.hpp, rl_cf_*), checked against the rule checker (oracle/fo_spawn_rules_ref.py) run with
the same object -- tests/test_caller_frame_cpu.py's InterpolatedNormalFrame, the model the device promises.  Curved paths
with coarse vertices, where that frame and the polyline frame disagree; seeded cases on scenarios 1-3; the one-call step;
the table's cache; a straight path; a bad frame code."""
import copy
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from test_caller_frame_cpu import InterpolatedNormalFrame, bend_path
from test_spawn_rules_gpu import CFG, _random_case, _same

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


def _cfg(frame):
    cfg = copy.deepcopy(CFG)
    cfg["accelerator"]["spawn"]["frame"] = frame
    return cfg


def _run(torch, lanelets, obstacles, path, ego, yaw, v, cosy, frame="caller", intersections=None, timestep=0, n_rays=720):
    """device rule points (locator with cosy_cl = cosy and the given frame) and the checker's with the same object"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    from oracle.fo_spawn_rules_ref import CellView, SpawnRules
    obs = FOObstacles(obstacles)
    obs.update(timestep)
    sm = SensorModel(lanelets, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=n_rays, intersections=intersections)
    sm.calc_visible_and_occluded_area(timestep, ego, yaw, obs)
    am = SimpleNamespace(scenario=SimpleNamespace(intersections=intersections or []))
    sl = SpawnLocator(am, path, _cfg(frame), sm, cosy_cl=cosy, fo_obstacles=obs)
    ego_cl = cosy.convert_to_curvilinear_coords(ego[0], ego[1])
    dev = list(sl.find_spawn_points(ego, yaw, ego_cl, v))
    torch.cuda.synchronize()
    view = CellView(sm.cell_class.cpu().numpy(), sm.window)

    def lane_yaw_at(xy):
        (x0, y0), (nx, ny) = sm.raster_origin, sm.raster_dims
        ix, iy = int(math.floor((xy[0] - x0) / sm.cell_size)), int(math.floor((xy[1] - y0) / sm.cell_size))
        if not (0 <= ix < nx and 0 <= iy < ny) or np.isnan(sm.lane_yaw[iy, ix]):
            return None
        return float(sm.lane_yaw[iy, ix])

    def lanelet_of(xy):
        for ll in lanelets:
            if S.points_in_polygon(np.asarray(xy, float).reshape(1, 2), ll.polygon)[0]:
                return ll
        return None
    rules = SpawnRules(CFG, path, cosy, lane_yaw_at, lanelet_of, obs, lanelets=lanelets, intersections=intersections or [])
    ref = rules.find(view, ego, ego_cl, v, yaw)
    assert sl.last_intention == rules.last_intention
    return dev, ref, view, sl


def _bend_lanes(S, radius=9.0, left=True):
    """a two-lane road along bend_path's geometry (sampled finely): lane 1 the ego's (|d| <= 1.75 about the path), lane 2
    the oncoming one beside it (its left neighbour), d on the side of the bend's inside"""
    th = np.radians(np.linspace(0.0, 90.0, 46))
    lead = np.stack((np.linspace(-40.0, 0.0, 41)[:-1], np.zeros(40)), -1)
    arc = np.stack((radius * np.sin(th), radius * (1.0 - np.cos(th))), -1)
    tail = np.stack((np.full(40, radius), radius + np.linspace(0.0, 40.0, 41)[1:]), -1)
    c = np.concatenate((lead, arc, tail))
    tn = np.concatenate((np.tile([[1.0, 0.0]], (40, 1)), np.stack((np.cos(th), np.sin(th)), -1), np.tile([[0.0, 1.0]], (40, 1))))
    nrm = np.stack((-tn[:, 1], tn[:, 0]), -1)
    off = lambda d: c + d * nrm
    l1 = S.Lanelet(1, off(1.75), off(-1.75))
    l2 = S.Lanelet(2, off(1.75)[::-1].copy(), off(5.25)[::-1].copy())
    l1.adj_left, l1.adj_left_same_direction = 2, False
    l2.adj_left, l2.adj_left_same_direction = 1, False
    if not left:
        m = lambda a: a * np.array([1.0, -1.0])
        l1, l2 = (S.Lanelet(ll.lanelet_id, m(ll.right), m(ll.left)) for ll in (l1, l2))
        l1.adj_left, l1.adj_left_same_direction = 2, False
        l2.adj_left, l2.adj_left_same_direction = 1, False
    return [l1, l2]


def _on_bend(radius, deg, d, left=True):
    t = math.radians(deg)
    sg = 1.0 if left else -1.0
    x, y = radius * math.sin(t) - d * math.sin(t), sg * (radius * (1.0 - math.cos(t)) + d * math.cos(t))
    return x, y, sg * t


def _bend_obstacles(S, radius, left, car_deg=25.0, car_d=-0.9, truck_deg=None):
    """a car parked on the ego's lane at car_deg into the bend (its right half on the shoulder) and, with truck_deg, an
    oncoming truck in the other lane"""
    x, y, h = _on_bend(radius, car_deg, car_d, left)
    out = [S.Obstacle(77, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([x, y, h, 0.0]), np.zeros((0, 4)))]
    if truck_deg is not None:
        x, y, h = _on_bend(radius, truck_deg, 3.5, left)
        out.append(S.Obstacle(31, "dynamic", "truck", 9.0, 3.2, 0, np.array([x, y, h + math.pi, 8.0]), np.zeros((0, 4))))
    return out


class _OffsetFrame:
    """a frame whose s counts from `off` metres before the path's first vertex (the frame of a path extended at its start):
    the reference asks it for the left-turn line at the POLYLINE arc lengths of the window (spawn_locator.py:513-515, 683)"""

    def __init__(self, f, off=5.0):
        self.f, self.off = f, off

    def convert_to_curvilinear_coords(self, x, y):
        s, d = self.f.convert_to_curvilinear_coords(x, y)
        return np.array([s + self.off, d])

    def convert_to_cartesian_coords(self, s, d):
        return self.f.convert_to_cartesian_coords(s - self.off, d)

    def convert_list_of_points_to_curvilinear_coords(self, points, num_threads=1):
        return [self.convert_to_curvilinear_coords(*np.asarray(q, dtype=np.float64).reshape(-1)[:2]) for q in points]


def _differs(a, b, view):
    """two record lists differ by at least a cell somewhere (same length) or in length"""
    if len(a) != len(b):
        return True
    return any(view._cell(p.position) != view._cell(q.position) for p, q in zip(a, b))


def test_turn_rule_on_a_curved_path(torch_cuda):
    """left and right turns on a bend of 9 m radius with a vertex every 45 deg: device == checker in the caller's frame, and
    the pedestrian stands elsewhere than in the polyline frame.  A frame whose s starts 5 m before the path: the left-turn
    line is the reference's -- the frame asked at the polyline arc lengths of the window, not at its own s"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    n_turn, n_diff, n_off = 0, 0, 0
    for left in (True, False):
        path = bend_path(radius=9.0, step_deg=45.0, left=left)
        lanes = _bend_lanes(S, 9.0, left)
        f = InterpolatedNormalFrame(path)
        for x in (-16.0, -12.0, -8.0):
            ego = np.array([x, 0.0])
            dev, ref, view, _ = _run(torch_cuda, lanes, [], path, ego, 0.0, 6.0, f)
            _same(dev, ref, view)
            n_turn += sum(p.source in ("left turn", "right turn") for p in ref)
            dev_p, ref_p, view_p, _ = _run(torch_cuda, lanes, [], path, ego, 0.0, 6.0, PolylineCS(path), frame="polyline")
            _same(dev_p, ref_p, view_p)
            n_diff += _differs(dev, dev_p, view)
            if left:
                dev_o, ref_o, view_o, sl = _run(torch_cuda, lanes, [], path, ego, 0.0, 6.0, _OffsetFrame(f))
                _same(dev_o, ref_o, view_o)
                assert sl.frame_fit_m < 1e-9
                n_off += sum(p.source == "left turn" for p in ref_o)
    assert n_turn >= 2 and n_diff >= 1 and n_off >= 1, (n_turn, n_diff, n_off)


def test_static_and_dynamic_rules_beside_a_bend(torch_cuda):
    """a car parked in the bend (and an oncoming truck): the static rule's cross lines and s windows are the caller frame's
    -- device == checker in both frames, pedestrians behind the parked car in every scene, a Car and a Bicycle behind the
    truck, and the static rule's points are not the polyline frame's (other cells, or a point only one frame finds)"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    # (left bend?, car at deg, truck at deg or None, ego x)
    scenes = [(True, 25.0, None, -12.0), (True, 15.0, None, -12.0), (True, 25.0, 5.0, -6.0), (False, 25.0, None, -12.0),
              (False, 15.0, 20.0, -12.0)]
    n_static, n_dynamic, n_diff = 0, 0, 0
    static = lambda pts: [p for p in pts if p.source.startswith("behind static")]
    for left, car, truck, x in scenes:
        path = bend_path(radius=9.0, step_deg=45.0, left=left)
        lanes = _bend_lanes(S, 9.0, left)
        obst = _bend_obstacles(S, 9.0, left, car_deg=car, truck_deg=truck)
        ego = np.array([x, 0.0])
        dev, ref, view, _ = _run(torch_cuda, lanes, obst, path, ego, 0.0, 6.0, InterpolatedNormalFrame(path))
        _same(dev, ref, view)
        dev_p, ref_p, view_p, _ = _run(torch_cuda, lanes, obst, path, ego, 0.0, 6.0, PolylineCS(path), frame="polyline")
        _same(dev_p, ref_p, view_p)
        assert len(static(ref)) == 1, (left, car, truck, x, [p.source for p in ref])
        n_static += 1
        n_dynamic += sum(p.source == "behind_dynamic_obstacle" for p in ref)
        n_diff += _differs(static(dev), static(dev_p), view)
    assert n_dynamic >= 2 and n_diff >= 3, (n_dynamic, n_diff)


def test_seeded_cases_on_the_three_scenarios(torch_cuda):
    """40 seeded poses of scenarios 1-3 (tests/test_spawn_rules_gpu.py's random cases), the frame built from each case's own
    reference path: device == checker"""
    from frenetix_occlusion import scenario as S
    scs = [S.load_geometry_npz(os.path.join(GOLDEN, f"scenario{i}_geometry.npz")) for i in (1, 2, 3)]
    rng = np.random.default_rng(7)
    done, n_pts, seen = 0, 0, set()
    while done < 40:
        si, sc, path, ego, yaw, step, v = _random_case(rng, scs)
        if len(path) < 4:
            continue
        f = InterpolatedNormalFrame(path)
        try:
            f.convert_to_curvilinear_coords(ego[0], ego[1])
        except ValueError:          # ego outside the path's projection domain: nothing to compare
            continue
        dev, ref, view, _ = _run(torch_cuda, sc.lanelets, sc.obstacles, path, ego, yaw, v, f, intersections=sc.intersections,
                                 timestep=step, n_rays=360)
        _same(dev, ref, view)
        done += 1
        n_pts += len(ref)
        seen.add(si)
    assert seen == {0, 1, 2} and n_pts > 0


def test_straight_path_gives_the_polyline_records(torch_cuda):
    """unit normals on a straight path: the caller's frame is the polyline frame, the records agree to 1e-9"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    from test_spawn_rules_gpu import _straight
    lanes = [_straight(S, 1, -10, 70, -3.5, 0.0), _straight(S, 2, -10, 70, 0.0, 3.5)]
    path = np.stack((np.linspace(-5, 65, 141), np.full(141, -1.0)), -1)
    car = S.Obstacle(77, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([17.0, -2.4, 0.0, 0.0]), np.zeros((0, 4)))
    ego = np.array([0.0, -1.0])
    dev_c, ref_c, view, sl = _run(torch_cuda, lanes, [car], path, ego, 0.0, 8.0, InterpolatedNormalFrame(path))
    assert sl.rule_inputs(ego, 0.0, None, 8.0)[1] is sl._d_frame6
    dev_p, _, _, _ = _run(torch_cuda, lanes, [car], path, ego, 0.0, 8.0, PolylineCS(path), frame="polyline")
    _same(dev_c, ref_c, view)
    _same(dev_c, dev_p, view)
    assert len(dev_c) == 1


def _stack(torch, lanelets, obstacles, path, cosy, M=128, T=31, ego=None, yaw=0.0):
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.step import PlanningStep
    from frenetix_occlusion.sweep import MetricSweep
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    cfg = _cfg("caller")
    cfg["agent_manager"]["truck"] = {"width": 2.5, "length": 9.0, "default_velocity": 8.0}
    cfg["accelerator"]["spawn"].update(routes=3, max_rule_points=8)
    ctx = N.Context(0)
    obs = FOObstacles(obstacles)
    sm = SensorModel(lanelets, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, ctx=ctx, routes=3)
    sl = SpawnLocator(None, path, cfg, sm, cosy_cl=cosy, fo_obstacles=obs, dt=0.1, horizon=(T - 1) * 0.1)
    sw = MetricSweep((4.508, 1.610, 1.4227, 1093.3, 11.5), 0.1, thresholds={"harm": 0.1, "risk": 1}, ctx=ctx)
    traj = SY.make_trajectories(M, T, 0.1, seed=3, ego_pos=ego, ego_yaw=yaw)
    tr = [torch.as_tensor(traj[k]).cuda() for k in ("x", "y", "theta", "v", "a")]
    return SimpleNamespace(ctx=ctx, obs=obs, sm=sm, sl=sl, sw=sw, tr=tr, step=lambda: PlanningStep(sm, sl, sw, *tr, mode="pair"))


def test_one_call_step_equals_the_stage_calls(torch_cuda):
    """fo_step_run through PlanningStep with frame: caller against the stage calls (queue_rules and the sweep) with the same
    object: cost, flags, pair scalars and rule records bit for bit; then frame = 2 in the step's structure is FO_E_ARG"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import scenario as S
    path = bend_path(radius=9.0, step_deg=45.0)
    lanes = _bend_lanes(S, 9.0)
    f = InterpolatedNormalFrame(path)
    got = {}
    for how in ("stages", "one-call"):
        k = _stack(torch, lanes, _bend_obstacles(S, 9.0, True), path, f, ego=np.array([-12.0, 0.0]))
        ps = k.step() if how == "one-call" else None
        res = []
        for x in (-14.0, -9.0, -5.0):
            ego = np.array([x, 0.0])
            k.obs.update(0)
            k.sm.upload_obstacles(k.obs)
            if ps is not None:
                out = ps.run(ego, 0.0, 6.0)
            else:
                k.sm.launch(ego, 0.0)
                k.sl.find_spawn_points(ego, 0.0, None, 6.0, lazy=True)
                k.sw.set_agents(*k.sl.batch.sweep_args(), check=False)
                out = k.sw.run(*k.tr, mode="pair")
            torch.cuda.synchronize()
            b = k.sl.batch
            assert k.sl.rule_inputs(ego, 0.0, None, 6.0)[1] is k.sl._d_frame6
            res.append([t.cpu().numpy().copy() for t in (out.cost, out.safe, out.pair_f, out.pair_i, b.rule_points, b.rule_n, b.pos,
                                                          b.len, b.head)])
        got[how] = res
    n_rule = 0
    for a, b in zip(got["stages"], got["one-call"]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
        n_rule += int(a[5][0])
    assert n_rule > 0
    s = ps._s
    s.rule.frame = 2
    rc = k.ctx._lib.fo_step_run(k.ctx._h, C.byref(s), N.current_stream(0))
    assert rc == N.FO_E_ARG and b"frame" in k.ctx._lib.fo_last_error(k.ctx._h)
    s.rule.frame = 1


def test_bad_frame_code_is_refused(torch_cuda):
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import scenario as S
    path = bend_path(radius=9.0, step_deg=45.0)
    f = InterpolatedNormalFrame(path)
    _, _, _, sl = _run(torch_cuda, _bend_lanes(S, 9.0), [], path, np.array([-12.0, 0.0]), 0.0, 6.0, f)
    pr = sl.rule_params(np.array([-12.0, 0.0]), 0.0, None, 6.0)
    assert pr.frame == 1
    pr.frame = 2
    O, corn, cen, oyaw, odims, ofl, ovis = sl.rule_obstacle_ptrs()
    sm, b, w = sl.sensor_model, sl.batch, sl.sensor_model.window
    with pytest.raises(N.NativeError, match="frame = 2"):
        sl.ctx.call("fo_scene_spawn_rules", sm.cell_class.data_ptr(), w.ix0, w.iy0, w.nx, w.ny, int(sl._d_frame6.shape[0]),
                    sl._d_frame6.data_ptr(), O, corn, cen, oyaw, odims, ofl, ovis, C.byref(pr), b.n_rule_points,
                    b.rule_points.data_ptr(), b.rule_n.data_ptr(), N.current_stream(0))


class _Counting:
    def __init__(self, f):
        self.f, self.calls = f, 0

    def __getattr__(self, name):
        m = getattr(self.f, name)

        def call(*a, **k):
            self.calls += 1
            return m(*a, **k)
        return call


def test_interface_builds_the_table_once_per_object(torch_cuda, tmp_path):
    """FOInterface with frame: caller -- evaluate_scenario twice with the same cosy_cl makes no call on it the second time
    (and uploads nothing); a new object rebuilds the table"""
    import yaml
    from frenetix_occlusion import interface
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion import synthetic as SY
    sc = S.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["accelerator"]["spawn"]["frame"] == "polyline"
    cfg["accelerator"]["spawn"]["frame"] = "caller"
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    ego0 = sc.ego_initial
    yaw = float(ego0[2])
    path = ego0[None, :2] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    v = SY.VEHICLE_BMW320I
    veh = SimpleNamespace(length=v[0], width=v[1], wb_rear_axle=v[2], mass=v[3], a_max=v[4])
    fo = interface.FOInterface(sc, path, veh, 0.1, config_path=str(cfg_path))
    raw = InterpolatedNormalFrame(path)
    c = _Counting(raw)
    tables = []
    for step in (0, 8):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        fo.evaluate_scenario({}, ego, yaw, raw.convert_to_curvilinear_coords(ego[0], ego[1]), float(ego0[3]), step, cosy_cl=c)
        list(fo.spawn_points)
        tables.append(fo.spawn_locator._d_frame6)
        if step == 0:
            n = c.calls
            assert n > 0
    assert c.calls == n and tables[0] is tables[1]
    c2 = _Counting(raw)
    ego = ego0[:2] + 0.7634 * 9 * np.array([math.cos(yaw), math.sin(yaw)])
    fo.evaluate_scenario({}, ego, yaw, raw.convert_to_curvilinear_coords(ego[0], ego[1]), float(ego0[3]), 9, cosy_cl=c2)
    assert c2.calls > 0 and fo.spawn_locator._d_frame6 is not tables[0]
    assert fo.spawn_locator.frame_fit_m < 1e-12
