"""The reference's spawn rule families on the device (fo_scene_spawn_rules, csrc/fo_spawn_rules.hpp) against their
independent NumPy restatement (oracle/fo_spawn_rules_ref.py) -- the three known-answer scenes of tests/test_spawn_rules.py
and the scenario-1 fixture at several time steps: same spawn points (type, source, cell, orientation), positions to 1e-9."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = {"spawn_locator": {"spawn_points_behind_turn": True, "spawn_point_behind_static_obstacle": True,
                         "spawn_point_behind_dynamic_obstacle": True, "max_static_spawn_points": 1,
                         "max_dynamic_spawn_points": 1},
       "agent_manager": {"pedestrian": {"width": 0.5, "length": 0.3, "default_velocity": 1.4},
                         "bicycle": {"width": 0.9, "length": 2.0, "default_velocity": 5.0},
                         "car": {"width": 2.0, "length": 4.8, "default_velocity": 10.0},
                         "prediction": {"variance_factor": 1.05, "size_factor_length_s": 1.2, "size_factor_width_s": 1.3,
                                        "size_factor_length_l": 1.4, "size_factor_width_l": 2.5}},
       "accelerator": {"spawn": {"mode": "rules"}}}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


def _both(torch, lanelets, obstacles, path, ego, yaw, v, intersections=None, timestep=0, n_rays=720, cell_size=0.5):
    """device rule points and checker rule points for one scene"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    from oracle.fo_spawn_rules_ref import CellView, SpawnRules
    obs = FOObstacles(obstacles)
    obs.update(timestep)
    sm = SensorModel(lanelets, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=n_rays, intersections=intersections,
                     cell_size=cell_size)
    sm.calc_visible_and_occluded_area(timestep, ego, yaw, obs)
    am = SimpleNamespace(scenario=SimpleNamespace(intersections=intersections or []))
    sl = SpawnLocator(am, path, CFG, sm, fo_obstacles=obs)
    cs = PolylineCS(path)
    ego_cl = cs.convert_to_curvilinear_coords(ego[0], ego[1])
    dev = [p for p in sl.find_spawn_points(ego, yaw, ego_cl, v)]
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
    rules = SpawnRules(CFG, path, cs, lane_yaw_at, lanelet_of, obs, lanelets=lanelets, intersections=intersections or [])
    ref = rules.find(view, ego, ego_cl, v, yaw)
    assert sl.last_intention == rules.last_intention
    return dev, ref, view


def _same(dev, ref, view):
    assert [(p.agent_type, p.source) for p in dev] == [(p.agent_type, p.source) for p in ref]
    for a, b in zip(dev, ref):
        assert view._cell(a.position) == view._cell(b.position)
        np.testing.assert_allclose(a.position, b.position, rtol=0, atol=1e-9)
        assert (a.orientation is None) == (b.orientation is None)
        if a.orientation is not None:
            assert a.orientation == pytest.approx(b.orientation, abs=1e-12)
        assert (a.cl_pos is None) == (b.cl_pos is None)
        if a.cl_pos is not None:
            np.testing.assert_allclose(a.cl_pos, b.cl_pos, rtol=0, atol=1e-9)


def _straight(S, lid, x0, x1, y_lo, y_hi, n=41):
    xs = np.linspace(x0, x1, n)
    return S.Lanelet(lid, np.stack((xs, np.full(n, y_hi)), -1), np.stack((xs, np.full(n, y_lo)), -1))


def test_pedestrian_behind_a_parked_car(torch_cuda):
    from frenetix_occlusion import scenario as S
    lanes = [_straight(S, 1, -10, 70, -3.5, 0.0), _straight(S, 2, -10, 70, 0.0, 3.5)]
    path = np.stack((np.linspace(-5, 65, 141), np.full(141, -1.0)), -1)
    ego = np.array([0.0, -1.0])
    for x, want in ((17.0, 1), (45.0, 0), (-6.0, 0)):
        car = S.Obstacle(77, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([x, -2.4, 0.0, 0.0]), np.zeros((0, 4)))
        dev, ref, view = _both(torch_cuda, lanes, [car], path, ego, 0.0, 8.0)
        assert len(ref) == want
        _same(dev, ref, view)
    # two parked cars 4 m apart in s: the 5 m rule between pedestrians drops the second one's point
    cars = [S.Obstacle(70 + i, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([14.0 + 6.5 * i, -2.4, 0.0, 0.0]), np.zeros((0, 4)))
            for i in range(2)]
    dev, ref, view = _both(torch_cuda, lanes, cars, path, ego, 0.0, 8.0)
    _same(dev, ref, view)


def test_pedestrian_behind_a_right_and_a_left_turn(torch_cuda):
    from frenetix_occlusion import scenario as S
    main = [_straight(S, 1, -40, 40, -3.5, 0.0), _straight(S, 2, -40, 40, 0.0, 3.5)]
    ys = np.linspace(-3.5, -43.5, 41)
    side = [S.Lanelet(3, np.stack((np.full(41, 13.5), ys), -1), np.stack((np.full(41, 10.0), ys), -1)),
            S.Lanelet(4, np.stack((np.full(41, 17.0), ys), -1), np.stack((np.full(41, 13.5), ys), -1))]
    ego = np.array([-5.0, -1.75])
    ang = np.linspace(0, math.pi / 2, 30)
    path = np.concatenate((np.stack((np.linspace(-30, 7.75, 76), np.full(76, -1.75)), -1),
                           np.stack((7.75 + 4.0 * np.sin(ang), -5.75 + 4.0 * np.cos(ang)), -1)[1:],
                           np.stack((np.full(60, 11.75), np.linspace(-6.25, -36.0, 60)), -1)))
    dev, ref, view = _both(torch_cuda, main + side, [], path, ego, 0.0, 6.0)
    assert len(ref) == 1 and ref[0].source == "right turn"
    _same(dev, ref, view)
    # mirrored: a left turn into a side street on the other side
    mirror = lambda a: a * np.array([1.0, -1.0])
    lanes_l = [S.Lanelet(ll.lanelet_id, mirror(ll.right), mirror(ll.left)) for ll in main + side]
    dev, ref, view = _both(torch_cuda, lanes_l, [], mirror(path), mirror(ego), 0.0, 6.0)
    assert all(p.source == "left turn" for p in ref)
    _same(dev, ref, view)
    # straight on: no turn rule
    straight = np.stack((np.linspace(-30, 40, 141), np.full(141, -1.75)), -1)
    dev, ref, view = _both(torch_cuda, main + side, [], straight, ego, 0.0, 6.0)
    assert dev == [] and ref == []


def test_table_space_of_the_rules_is_enough_or_refused(torch_cuda):
    """A reference path sampled every 6 cm puts 640 vertices into the 40 m window (the turn rule held 256 until round 6 and left
    silently: tools/spawn_rules_fuzz.py with subdivided lanelets found it); 1 900 vertices are refused by the entry point, and a
    line of more samples than the rule's table (cells of 0.25 m: 1 281 over 40 m) comes back as a refused count, not as a
    shorter list."""
    from frenetix_occlusion import scenario as S
    main = [_straight(S, 1, -40, 40, -3.5, 0.0), _straight(S, 2, -40, 40, 0.0, 3.5)]
    ys = np.linspace(-3.5, -43.5, 41)
    side = [S.Lanelet(3, np.stack((np.full(41, 13.5), ys), -1), np.stack((np.full(41, 10.0), ys), -1)),
            S.Lanelet(4, np.stack((np.full(41, 17.0), ys), -1), np.stack((np.full(41, 13.5), ys), -1))]
    ego = np.array([-5.0, -1.75])
    ang = np.linspace(0, math.pi / 2, 30)
    path = np.concatenate((np.stack((np.linspace(-30, 7.75, 76), np.full(76, -1.75)), -1),
                           np.stack((7.75 + 4.0 * np.sin(ang), -5.75 + 4.0 * np.cos(ang)), -1)[1:],
                           np.stack((np.full(60, 11.75), np.linspace(-6.25, -36.0, 60)), -1)))

    def subdivided(k):
        t = np.arange(k)[None, :, None] / k
        return np.concatenate(((path[:-1, None, :] + t * (path[1:, None, :] - path[:-1, None, :])).reshape(-1, 2), path[-1:]))
    dev, ref, view = _both(torch_cuda, main + side, [], subdivided(8), ego, 0.0, 6.0)
    assert len(ref) == 1 and ref[0].source == "right turn"
    _same(dev, ref, view)
    with pytest.raises(RuntimeError, match="turn rule"):
        _both(torch_cuda, main + side, [], subdivided(24), ego, 0.0, 6.0)
    import warnings
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError, match="table space"):
            _both(torch_cuda, main + side, [], path, ego, 0.0, 6.0, cell_size=0.25)
    from frenetix_occlusion import spawn_locator as SL      # (and the locator said so when it was set up, in the check's own numbers)
    said = [str(w.message) for w in rec if "SpawnLocator: cells of 0.25 m" in str(w.message)]
    assert said and all(f"{SL.turn_line_min_cell():.4f} m" in t and f"{SL.cross_line_limit(0.25):g} m" in t for t in said)
    assert all("turn rule" in t and "static-obstacle rule" in t for t in said)


def test_car_and_bicycle_behind_an_oncoming_truck(torch_cuda):
    from frenetix_occlusion import scenario as S
    xs = np.linspace(-10, 70, 41)
    lane1 = S.Lanelet(1, np.stack((xs, np.zeros(41)), -1), np.stack((xs, np.full(41, -3.5)), -1))
    lane2 = S.Lanelet(2, np.stack((xs[::-1], np.zeros(41)), -1), np.stack((xs[::-1], np.full(41, 3.5)), -1))
    lane1.adj_left, lane1.adj_left_same_direction = 2, False
    lane2.adj_left, lane2.adj_left_same_direction = 1, False
    path = np.stack((np.linspace(-5, 65, 141), np.full(141, -1.75)), -1)
    ego = np.array([0.0, -1.75])
    for typ, yaw in (("truck", math.pi), ("bicycle", math.pi), ("truck", 0.0), ("car", math.pi + 0.2)):
        ob = S.Obstacle(31, "dynamic", typ, 9.0, 3.2 if typ == "truck" else 2.0, 0, np.array([20.0, 1.75, yaw, 8.0]), np.zeros((0, 4)))
        dev, ref, view = _both(torch_cuda, [lane1, lane2], [ob], path, ego, 0.0, 8.0)
        if typ == "truck" and yaw == math.pi:
            assert [p.agent_type for p in ref] == ["Car", "Bicycle"]
        _same(dev, ref, view)


def test_both_labelling_forms_of_the_dynamic_rule(torch_cuda, monkeypatch):
    """The candidate region's connected parts are labelled on the runs of the lattice rows (round 6); the node form of rounds
    4-5 stays as the fallback for more runs than the arrays hold.  FO_SCENE_RULE_NODES=1 sends every case through it: both forms
    against the checker -- and therefore against each other -- on the oncoming-truck scenes and on the scenario-1 steps at which
    the rule fires (20, 25, 33: one and three phantom vehicles)."""
    from frenetix_occlusion import scenario as S
    xs = np.linspace(-10, 70, 41)
    lane1 = S.Lanelet(1, np.stack((xs, np.zeros(41)), -1), np.stack((xs, np.full(41, -3.5)), -1))
    lane2 = S.Lanelet(2, np.stack((xs[::-1], np.zeros(41)), -1), np.stack((xs[::-1], np.full(41, 3.5)), -1))
    lane1.adj_left, lane1.adj_left_same_direction = 2, False
    lane2.adj_left, lane2.adj_left_same_direction = 1, False
    path = np.stack((np.linspace(-5, 65, 141), np.full(141, -1.75)), -1)
    sc = S.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    ego0 = sc.ego_initial
    yaw = float(ego0[2])
    path1 = ego0[None, :2] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    n_vehicles = {}
    for form in ("runs", "nodes"):
        if form == "nodes":
            monkeypatch.setenv("FO_SCENE_RULE_NODES", "1")
        n = 0
        ob = S.Obstacle(31, "dynamic", "truck", 9.0, 3.2, 0, np.array([20.0, 1.75, math.pi, 8.0]), np.zeros((0, 4)))
        dev, ref, view = _both(torch_cuda, [lane1, lane2], [ob], path, np.array([0.0, -1.75]), 0.0, 8.0)
        assert [p.agent_type for p in ref] == ["Car", "Bicycle"]
        _same(dev, ref, view)
        n += len(dev)
        for step in (20, 25, 33):
            ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
            dev, ref, view = _both(torch_cuda, sc.lanelets, sc.obstacles, path1, ego, yaw, float(ego0[3]),
                                   intersections=sc.intersections, timestep=step)
            _same(dev, ref, view)
            n += sum(p.agent_type in ("Car", "Bicycle") for p in dev)
        n_vehicles[form] = n
    assert n_vehicles["runs"] == n_vehicles["nodes"] >= 5


def test_scenario1_steps(torch_cuda):
    """the scenario-1 fixture (12 lanelets, an intersection, parked and moving obstacles) at time steps 0 / 8 / 25 / 60"""
    from frenetix_occlusion import scenario as S
    sc = S.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    ego0 = sc.ego_initial
    yaw = float(ego0[2])
    path = ego0[None, :2] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    n_pts = 0
    for step in (0, 8, 25, 60):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        dev, ref, view = _both(torch_cuda, sc.lanelets, sc.obstacles, path, ego, yaw, float(ego0[3]),
                               intersections=sc.intersections, timestep=step)
        _same(dev, ref, view)
        n_pts += len(ref)
    assert n_pts > 0


def test_device_returns_the_reference_decisions_on_every_recorded_scene(torch_cuda):
    """tests/golden/spawn_rule_bodies.npz (the reference's own, unmodified rule methods over the build's discretisation,
    ``gen_golden.py rules``) through ``SpawnLocator.find_spawn_points`` -> ``fo_scene_spawn_rules`` on every recorded scene,
    the caller-frame cases with ``accelerator.spawn.frame: caller``: the device's cell classes reproduce the recorded counts of
    road / visible / occluded cells, and the list is the reference's -- the same ordered (agent type, source), the same cell,
    positions and cl_pos to 1e-9, orientations to 1e-12 (``_same``'s tolerances).  Scenes in which the reference raises are
    only required to give a list.  Reads tests/golden/ only."""
    import spawn_rule_cases as SC
    from test_spawn_rule_bodies_cpu import compare
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    from oracle.fo_spawn_rules_ref import CellView
    cases, _ = SC.load_fixture()
    assert len(cases) >= 200
    models, bad, worst, n_caller = {}, [], 0.0, 0
    for k, (case, rec) in enumerate(cases):
        key = (case.map_index, case.n_rays, case.cell_size)
        if key not in models:
            models[key] = SensorModel(case.lanelets, None, sensor_radius=SC.SENSOR_RADIUS, sensor_angle=360.0, n_rays=case.n_rays,
                                      intersections=case.intersections, cell_size=case.cell_size)
        sm = models[key]
        obs = FOObstacles(case.obstacles)
        obs.update(case.step)
        sm.calc_visible_and_occluded_area(case.step, case.ego, case.yaw, obs)
        cosy = SC.frame_of(case)
        ego_cl = cosy.convert_to_curvilinear_coords(case.ego[0], case.ego[1])
        am = SimpleNamespace(scenario=SimpleNamespace(intersections=case.intersections))
        sl = SpawnLocator(am, case.path, case.cfg, sm, cosy_cl=cosy if case.frame else None, fo_obstacles=obs)
        n_caller += case.frame
        dev = list(sl.find_spawn_points(case.ego, case.yaw, ego_cl, case.v))
        torch_cuda.cuda.synchronize()
        view = CellView(sm.cell_class.cpu().numpy(), sm.window)
        if not np.array_equal(SC.class_counts(view.cls), rec["counts"]):
            bad.append(f"case {k}: class counts {SC.class_counts(view.cls)} != {rec['counts']}")
        if rec["intention"] is not None and sl.last_intention != rec["intention"]:
            bad.append(f"case {k}: intention {sl.last_intention} != {rec['intention']}")
        if rec["calls"]["find"][0] == SC.RAISES:
            continue                     # the reference raises here: the device continues and gave a list
        why = compare(rec["calls"]["find"], dev, view)
        if why:
            bad.append(f"case {k} find: {why}")
        for a, b in zip(SC.points_of(dev), rec["calls"]["find"][2]):
            if a[:2] == b[:2]:
                worst = max(worst, float(np.abs(a[2] - b[2]).max()))
    print(f"recorded scenes {len(cases)}, through a caller's frame {n_caller}, largest position difference {worst:.3g} m")
    assert n_caller >= 10
    assert not bad, f"{len(bad)} differences, cases {sorted({int(b.split()[1].rstrip(':')) for b in bad})}:\n" + "\n".join(bad[:40])


def _random_case(rng, scs):
    """one random case of tools/spawn_rules_fuzz.py: a scenario, an ego pose near a lanelet centre line, a reference path
    straight ahead or along the centre lines of the lanelet and its successors, a time step, a speed"""
    si = int(rng.integers(len(scs)))
    sc = scs[si]
    by = {l.lanelet_id: l for l in sc.lanelets}
    ll = sc.lanelets[int(rng.integers(len(sc.lanelets)))]
    c = ll.center
    i = int(rng.integers(0, max(len(c) - 2, 1)))
    ego = c[i] + rng.normal(0.0, 0.3, 2)
    yaw = math.atan2(c[i + 1, 1] - c[i, 1], c[i + 1, 0] - c[i, 0]) + float(rng.normal(0.0, 0.05))
    if rng.random() < 0.5:
        path = ego[None] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    else:
        parts, cur = [c[max(i - 3, 0):]], ll
        for _ in range(3):
            if not cur.successors:
                break
            cur = by.get(cur.successors[int(rng.integers(len(cur.successors)))])
            if cur is None:
                break
            parts.append(cur.center[1:])
        path = np.concatenate(parts)
        path = path[np.concatenate(([True], np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1])) > 1e-6))]
    return si, sc, path, ego, yaw, int(rng.integers(0, 80)), float(rng.uniform(2.0, 12.0))


def test_fifty_seeded_random_cases_on_the_three_scenarios(torch_cuda):
    """50 seeded cases of tools/spawn_rules_fuzz.py (random poses, paths with and without turns, time steps of scenario 1 / 2 / 3):
    device == checker on every one; the seed is chosen so that all three rule families fire"""
    from frenetix_occlusion import scenario as S
    scs = [S.load_geometry_npz(os.path.join(GOLDEN, f"scenario{i}_geometry.npz")) for i in (1, 2, 3)]
    rng = np.random.default_rng(3)
    kinds, done, seen = {}, 0, set()
    while done < 50:
        si, sc, path, ego, yaw, step, v = _random_case(rng, scs)
        if len(path) < 4:
            continue
        try:
            dev, ref, view = _both(torch_cuda, sc.lanelets, sc.obstacles, path, ego, yaw, v, intersections=sc.intersections,
                                   timestep=step, n_rays=360)
        except ValueError:          # ego outside the path's projection domain: nothing to compare
            continue
        _same(dev, ref, view)
        done += 1
        seen.add(si)
        for p in ref:
            key = p.source.split(" ")[0] + ":" + p.agent_type
            kinds[key] = kinds.get(key, 0) + 1
    assert seen == {0, 1, 2}
    assert any(k.startswith("behind_dynamic") for k in kinds) and any(k.startswith("behind:") for k in kinds)
    assert any(k.startswith(("left", "right")) for k in kinds), kinds


@pytest.mark.parametrize("k", [4, 12])
def test_seeded_random_cases_with_subdivided_lanelet_bounds(torch_cuda, k):
    """the same kind of cases on maps whose lanelet bounds are subdivided k-fold (tools/spawn_rules_fuzz.py's third argument):
    polygons of up to 550 vertices -- the dynamic rule's per-band edge lists run over many chunks at 4; at 12 the candidate
    polygons no longer fit its LDS table (read from HBM), a centre-line reference path puts > 256 vertices into the 40 m window
    (the turn rule's capacity until round 6) and the window's every-fifth-vertex query asks > 64 points"""
    from frenetix_occlusion import scenario as S
    scs = [S.load_geometry_npz(os.path.join(GOLDEN, f"scenario{i}_geometry.npz")) for i in (1, 2, 3)]
    t = np.arange(k)[None, :, None] / k
    sub = lambda b: np.concatenate(((b[:-1, None, :] + t * (b[1:, None, :] - b[:-1, None, :])).reshape(-1, 2), b[-1:]))
    for sc in scs:
        for ll in sc.lanelets:
            ll.left, ll.right = sub(ll.left), sub(ll.right)
    rng = np.random.default_rng(106)
    done, n_pts, long_windows = 0, 0, 0
    while done < 24:
        si, sc, path, ego, yaw, step, v = _random_case(rng, scs)
        if len(path) < 4:
            continue
        try:
            dev, ref, view = _both(torch_cuda, sc.lanelets, sc.obstacles, path, ego, yaw, v, intersections=sc.intersections,
                                   timestep=step, n_rays=360)
        except ValueError:          # ego outside the path's projection domain: nothing to compare
            continue
        _same(dev, ref, view)
        done += 1
        n_pts += len(ref)
        arc = np.concatenate(([0.0], np.cumsum(np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1])))))
        i0 = int(np.argmin(np.hypot(path[:, 0] - ego[0], path[:, 1] - ego[1])))
        long_windows += int(np.searchsorted(arc, arc[i0] + 40.0) - i0 > 256)
    assert n_pts > 0
    if k == 12:
        assert long_windows > 0      # (a path along subdivided centre lines: more window vertices than the turn rule used to hold)


def test_urban_grid_rule_cases(torch_cuda):
    """the BASELINE configs[2] city grid (9 360 boundary pieces, 64 parked cars, ~600 lanelets): the rule families at the
    bench's ego pose and at poses along two streets -- pedestrians behind parked cars, device == checker"""
    from frenetix_occlusion import scenario as S
    sc = S.synthetic_urban_grid()
    ego0 = sc.ego_initial
    n_pts = 0
    for k, (dx, dyaw) in enumerate(((0.0, 0.0), (14.0, 0.0), (31.0, 0.0), (-12.0, 0.0), (6.0, 0.03))):
        yaw = float(ego0[2]) + dyaw
        ego = ego0[:2] + dx * np.array([math.cos(ego0[2]), math.sin(ego0[2])])
        path = ego[None] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
        dev, ref, view = _both(torch_cuda, sc.lanelets, sc.obstacles, path, ego, yaw, 8.0, intersections=getattr(sc, "intersections", None),
                               timestep=0, n_rays=720)
        _same(dev, ref, view)
        n_pts += len(ref)
    assert n_pts > 0


def test_interface_with_the_default_yaml_spawns_what_the_reference_rules_spawn(torch_cuda):
    """``FOInterface(..., config_path=None)`` -- the packaged YAML, untouched -- runs the reference's spawn semantics
    (interface.py:186-198: find_spawn_points = the three rule families): on scenario 1 at steps 0 / 8 / 25 / 60 its
    ``spawn_points`` are the checker's (oracle/fo_spawn_rules_ref.py) for the same visibility, and one phantom agent per point
    reaches the registry.  The spawn-point list is a ``list`` that reads the device when first looked at; one kept past the
    next planning step still holds ITS step's points."""
    from frenetix_occlusion import interface
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.spawn_locator import LazySpawnPoints
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    from oracle.fo_spawn_rules_ref import CellView, SpawnRules
    sc = S.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    ego0 = sc.ego_initial
    yaw = float(ego0[2])
    path = ego0[None, :2] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    v = SY.VEHICLE_BMW320I
    veh = SimpleNamespace(length=v[0], width=v[1], wb_rear_axle=v[2], mass=v[3], a_max=v[4])
    fo = interface.FOInterface(sc, path, veh, 0.1)                       # config_path=None: the defaults
    assert fo.config["accelerator"]["spawn"]["mode"] == "rules" and fo.spawn_locator.mode == "rules"
    assert fo.spawn_locator.n_cell_agents == 0 and fo.spawn_locator.max_rule_points >= 6
    cs = PolylineCS(path)
    sm = fo.sensor_model

    def lane_yaw_at(xy):
        (x0, y0), (nx, ny) = sm.raster_origin, sm.raster_dims
        ix, iy = int(math.floor((xy[0] - x0) / sm.cell_size)), int(math.floor((xy[1] - y0) / sm.cell_size))
        if not (0 <= ix < nx and 0 <= iy < ny) or np.isnan(sm.lane_yaw[iy, ix]):
            return None
        return float(sm.lane_yaw[iy, ix])

    def lanelet_of(xy):
        for ll in sc.lanelets:
            if S.points_in_polygon(np.asarray(xy, float).reshape(1, 2), ll.polygon)[0]:
                return ll
        return None
    n_pts, kept = 0, []
    for step in (0, 8, 25, 60):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        ego_cl = cs.convert_to_curvilinear_coords(ego[0], ego[1])
        fo.evaluate_scenario({}, ego, yaw, ego_cl, float(ego0[3]), step, None)
        pts = fo.spawn_points
        assert isinstance(pts, list) and isinstance(pts, LazySpawnPoints) and not pts.materialised    # nothing read back yet
        kept.append((step, pts))
        if step != 8:              # (step 8's list stays unread until the NEXT step has been queued, see below)
            dev = list(pts)
            torch_cuda.cuda.synchronize()
            view = CellView(sm.cell_class.cpu().numpy(), sm.window)
            rules = SpawnRules(fo.config, path, cs, lane_yaw_at, lanelet_of, fo.fo_obstacles, lanelets=sc.lanelets,
                               intersections=sc.intersections or [])
            ref = rules.find(view, ego, ego_cl, float(ego0[3]), yaw)
            _same(dev, ref, view)
            assert len(fo.agent_manager.phantom_agents) == len(ref)
            assert [a.agent_type for a in fo.agent_manager.phantom_agents] == [p.agent_type for p in ref]
            n_pts += len(ref)
            assert pts + [] == dev and [] + pts == dev and (len(pts) > 0) == bool(pts)              # list semantics
    assert n_pts > 0
    # the list of step 8 was first read after step 25 (and 60) had been queued on the same buffers: it was read back when
    # step 25 began, and holds the points of step 8 -- those of a fresh interface driven to step 8 only
    late = [p for st, p in kept if st == 8][0]
    assert late.materialised
    fo2 = interface.FOInterface(sc, path, veh, 0.1)
    ego = ego0[:2] + 0.7634 * 8 * np.array([math.cos(yaw), math.sin(yaw)])
    fo2.evaluate_scenario({}, ego, yaw, cs.convert_to_curvilinear_coords(ego[0], ego[1]), float(ego0[3]), 8, None)
    want = list(fo2.spawn_points)
    assert [(p.agent_type, p.source) for p in late] == [(p.agent_type, p.source) for p in want]
    for a, b in zip(late, want):
        assert np.array_equal(a.position, b.position)


def test_rule_point_capacity_follows_the_yaml_maxima(torch_cuda):
    """max_dynamic / max_static = 3 allow (3 + 2) + (3 + 1) + 1 = 10 rule points (the maxima are compared before appending,
    Q11): the locator sizes its buffers for that whatever ``max_rule_points`` says, and the C entry refuses a smaller one"""
    import copy
    import ctypes as C
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    cfg = copy.deepcopy(CFG)
    cfg["spawn_locator"].update(max_static_spawn_points=3, max_dynamic_spawn_points=3)
    cfg["accelerator"]["spawn"]["max_rule_points"] = 8
    lanes = [_straight(S, 1, -10, 120, -3.5, 0.0), _straight(S, 2, -10, 120, 0.0, 3.5)]
    path = np.stack((np.linspace(-5, 115, 241), np.full(241, -1.0)), -1)
    cars = [S.Obstacle(70 + i, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([12.0 + 7.0 * i, -2.4, 0.0, 0.0]), np.zeros((0, 4)))
            for i in range(6)]
    obs = FOObstacles(cars)
    obs.update(0)
    sm = SensorModel(lanes, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720)
    sm.calc_visible_and_occluded_area(0, np.array([0.0, -1.0]), 0.0, obs)
    sl = SpawnLocator(None, path, cfg, sm, fo_obstacles=obs)
    assert sl.max_rule_points == 10
    pts = sl.find_spawn_points(np.array([0.0, -1.0]), 0.0, None, 12.0)
    torch_cuda.cuda.synchronize()
    assert 1 <= len(pts) <= 4 and all(p.agent_type == "Pedestrian" for p in pts)
    b = sl.batch
    pr = sl.rule_params(np.array([0.0, -1.0]), 0.0, None, 12.0)
    O, corn, cen, oyaw, odims, ofl, ovis = sl.rule_obstacle_ptrs()
    w = sm.window
    with pytest.raises(N.NativeError):
        sl.ctx.call("fo_scene_spawn_rules", sm.cell_class.data_ptr(), w.ix0, w.iy0, w.nx, w.ny, int(sl._d_path6.shape[0]),
                    sl._d_path6.data_ptr(), O, corn, cen, oyaw, odims, ofl, ovis, C.byref(pr), 8, b.rule_points.data_ptr(),
                    b.rule_n.data_ptr(), N.current_stream(0))
