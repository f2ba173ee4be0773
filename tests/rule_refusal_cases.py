"""Scenes on both sides of every table limit of the spawn rule kernels (csrc/fo_rule_pedestrian.hpp, fo_rule_dynamic.hpp:
a rule line of more than RL_MAXSAMP samples, an obstacle's centre on more than sixteen lanelets or on more than seven relevant
ones), the host statement of the sample count they are placed by, and the small stack the refusal tests run them through.

Every scene is a variation of a known-answer scene of tests/test_spawn_rules_gpu.py (right turn, parked car, oncoming truck),
built with that file's helpers.  No GPU is touched on import; the functions that need one take ``torch``."""
import copy
import math
from types import SimpleNamespace

import numpy as np

import test_spawn_rules_gpu as TS

MAXSAMP = 1024            # written out on purpose: tests/test_rule_refusal_cpu.py ties it to the header and to _native
MAX_DIST_OBST = 30.0      # spawn_locator.py:69 -- an obstacle farther away is skipped BEFORE its cross line is measured
VEH = (4.508, 1.610, 1.4227, 1093.3, 11.5)
M, T = 130, 16            # two full reduce workgroups and a ragged tail of two; a short horizon


def samples(total, cell_size):
    """ns of a rule line of ``total`` metres: one sample every cell / 8, half a step beyond the end (fo_rule_pedestrian.hpp:38,154)"""
    step = cell_size / 8.0
    return int(math.ceil((total + 0.5 * step) / step))


def total_for(ns_plus, cell_size):
    """a line length whose sample count is ceil(ns_plus): ns_plus = 1023.5 sits in the middle of the lengths that give 1 024"""
    return (ns_plus - 0.5) * cell_size / 8.0


def scene(lanelets, obstacles, path, ego, yaw, v, intersections=None, cell_size=0.5):
    return SimpleNamespace(lanelets=lanelets, obstacles=obstacles, path=path, ego=np.asarray(ego, float), yaw=yaw, v=v,
                           intersections=intersections, cell_size=cell_size)


# ------------------------------------------------------------------------------------------------ the turn rule's window
def turn_path():
    ang = np.linspace(0, math.pi / 2, 30)
    return np.concatenate((np.stack((np.linspace(-30, 7.75, 76), np.full(76, -1.75)), -1),
                           np.stack((7.75 + 4.0 * np.sin(ang), -5.75 + 4.0 * np.cos(ang)), -1)[1:],
                           np.stack((np.full(60, 11.75), np.linspace(-6.25, -36.0, 60)), -1)))


TURN_EGO = np.array([-5.0, -1.75])


def turn_window_length(path=None, ego=TURN_EGO, distance=40.0):
    """polyline length of the reference window [i0, i1) the turn rule samples (spawn_locator.py:678-693: the vertices nearest
    to the ego's arc length and to 40 m beyond; the window leaves the second one out)"""
    path = turn_path() if path is None else path
    s = np.concatenate(([0.0], np.cumsum(np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1])))))
    k = int(np.argmin(np.hypot(path[:, 0] - ego[0], path[:, 1] - ego[1])))     # (the ego stands on the straight part: s = s[k] + dx)
    s_ego = s[k] + (ego[0] - path[k, 0])
    i0, i1 = int(np.argmin(np.abs(s - s_ego))), int(np.argmin(np.abs(s - (s_ego + distance))))
    return float(s[i1 - 1] - s[i0])


def turn_scene(cell_size):
    """the right turn of test_pedestrian_behind_a_right_and_a_left_turn"""
    from frenetix_occlusion import scenario as S
    main = [TS._straight(S, 1, -40, 40, -3.5, 0.0), TS._straight(S, 2, -40, 40, 0.0, 3.5)]
    ys = np.linspace(-3.5, -43.5, 41)
    side = [S.Lanelet(3, np.stack((np.full(41, 13.5), ys), -1), np.stack((np.full(41, 10.0), ys), -1)),
            S.Lanelet(4, np.stack((np.full(41, 17.0), ys), -1), np.stack((np.full(41, 13.5), ys), -1))]
    return scene(main + side, [], turn_path(), TURN_EGO, 0.0, 6.0, cell_size=cell_size)


def turn_cell_size(ns_plus):
    """the cell size at which the turn scene's window takes ceil(ns_plus) samples"""
    return 8.0 * turn_window_length() / (ns_plus - 0.5)


# ------------------------------------------------------------------------------------------------ the static rule's cross line
STATIC_CELL = 0.25
WALL_TOP, WALL_THICK = -1.5, 4.5      # the parked car of test_pedestrian_behind_a_parked_car, grown away from the road


def wall(x, total, oid=77):
    """a static obstacle turned 90 degrees to the straight path, its d-extent = total - 1.6 m (the cross line adds 0.8 m at
    either end), its upper side where the parked car's is: the ego looks past it into the other lane"""
    from frenetix_occlusion import scenario as S
    length = total - 1.6
    return S.Obstacle(oid, "static", "parkedVehicle", length, WALL_THICK, 0,
                      np.array([x, WALL_TOP - 0.5 * length, math.pi / 2, 0.0]), np.zeros((0, 4)))


def parked_car(x, oid=70):
    from frenetix_occlusion import scenario as S
    return S.Obstacle(oid, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([x, -2.4, 0.0, 0.0]), np.zeros((0, 4)))


def static_lanes():
    """the two lanes of test_pedestrian_behind_a_parked_car, the ego's 35 m wide (a yard the road runs along): the rule takes
    the pedestrian's heading from the lanelet under the obstacle's CENTRE and drops the point without one, and the centre of
    a 30 m obstacle across the path is 15 m from its end"""
    from frenetix_occlusion import scenario as S
    lanes = [TS._straight(S, 1, -10, 70, -35.0, 0.0), TS._straight(S, 2, -10, 70, 0.0, 3.5)]
    return lanes, np.stack((np.linspace(-5, 65, 141), np.full(141, -1.0)), -1), np.array([0.0, -1.0])


def static_scene(obstacles, cell_size=STATIC_CELL):
    lanes, path, ego = static_lanes()
    return scene(lanes, obstacles, path, ego, 0.0, 8.0, cell_size=cell_size)


def cross_line_total(ob, path):
    """d-extent of the obstacle's corners over a straight path along x, + 1.6 m (fo_rule_pedestrian.hpp:141-152)"""
    c, s = math.cos(ob.initial[2]), math.sin(ob.initial[2])
    hl, hw = 0.5 * ob.length, 0.5 * ob.width
    ys = [ob.initial[1] + sx * hl * s + sy * hw * c for sx in (-1, 1) for sy in (-1, 1)]
    return max(ys) - min(ys) + 1.6


class FanFrame:
    """a caller's frame over the straight path of the static scenes whose d-lines fan out: s = x - x0, one unit of d is
    1 + k s metres.  In the polyline frame both cross lines of an obstacle have one length; in this frame the rear line (larger
    s) is the longer one -- the table the device projects through is exact for it (normals linear in s, include/fo_hip.h)"""

    def __init__(self, x0=-5.0, y0=-1.0, k=0.002):
        self.x0, self.y0, self.k = x0, y0, k

    def convert_to_curvilinear_coords(self, x, y):
        s = x - self.x0
        return np.array([s, (y - self.y0) / (1.0 + self.k * s)])

    def convert_to_cartesian_coords(self, s, d):
        return np.array([self.x0 + s, self.y0 + d * (1.0 + self.k * s)])

    def convert_list_of_points_to_curvilinear_coords(self, points, num_threads=1):
        return [self.convert_to_curvilinear_coords(*np.asarray(q, dtype=np.float64).reshape(-1)[:2]) for q in points]


def corners_of(ob):
    c, s = math.cos(ob.initial[2]), math.sin(ob.initial[2])
    hl, hw = 0.5 * ob.length, 0.5 * ob.width
    return np.array([[ob.initial[0] + a * hl * c - b * hw * s, ob.initial[1] + a * hl * s + b * hw * c] for a, b in ((1, 1), (1, -1), (-1, -1), (-1, 1))])


def frame_cross_lines(cosy, corners):
    """lengths of the static rule's two cross lines (at s_min - 0.8 and s_max + 0.8, from d_min - 0.8 to d_max + 0.8:
    fo_spawn_rules_ref.py:292-302) through the frame object"""
    ccl = np.array([cosy.convert_to_curvilinear_coords(x, y) for x, y in corners])
    d_min, d_max = ccl[:, 1].min() - 0.8, ccl[:, 1].max() + 0.8
    return [float(np.linalg.norm(cosy.convert_to_cartesian_coords(s, d_max) - cosy.convert_to_cartesian_coords(s, d_min)))
            for s in (ccl[:, 0].min() - 0.8, ccl[:, 0].max() + 0.8)]


def fan_wall_totals(cosy, cell_size, x=17.0):
    """(total of a wall whose two lines both fit, total of one whose first line fits and whose second does not), each at least
    three samples from the table's edge -- searched in centimetres, asserted by the caller"""
    fit = over = None
    for total in np.arange(29.0, 33.0, 0.01):
        n = [samples(t, cell_size) for t in frame_cross_lines(cosy, corners_of(wall(x, float(total))))]
        if 1000 < n[0] and n[1] <= MAXSAMP - 3:
            fit = float(total)
        if over is None and n[0] <= MAXSAMP - 3 and n[1] >= MAXSAMP + 4:
            over = float(total)
    return fit, over


# ------------------------------------------------------------------------------------------------ lanelets under a truck's centre
def truck(x=20.0, oid=31):
    from frenetix_occlusion import scenario as S
    return S.Obstacle(oid, "dynamic", "truck", 9.0, 3.2, 0, np.array([x, 1.75, math.pi, 8.0]), np.zeros((0, 4)))


def oncoming_lanes(copies, x0=-10.0, x1=70.0):
    """the two lanes of test_car_and_bicycle_behind_an_oncoming_truck, the oncoming one (id 2) with ``copies`` - 1 further
    lanelets of its own shape over x in [x0, x1] laid on top of it (ids 100 ...): a centre there lies on ``copies`` lanelets"""
    from frenetix_occlusion import scenario as S
    xs = np.linspace(-10, 70, 41)
    lane1 = S.Lanelet(1, np.stack((xs, np.zeros(41)), -1), np.stack((xs, np.full(41, -3.5)), -1))
    lane2 = S.Lanelet(2, np.stack((xs[::-1], np.zeros(41)), -1), np.stack((xs[::-1], np.full(41, 3.5)), -1))
    lane1.adj_left, lane1.adj_left_same_direction = 2, False
    lane2.adj_left, lane2.adj_left_same_direction = 1, False
    out = [lane1, lane2]
    xc = np.linspace(x1, x0, 21)
    for i in range(copies - 1):
        ll = S.Lanelet(100 + i, np.stack((xc, np.zeros(21)), -1), np.stack((xc, np.full(21, 3.5)), -1))
        ll.adj_left, ll.adj_left_same_direction = 1, False
        out.append(ll)
    return out


TRUCK_PATH = np.stack((np.linspace(-5, 65, 141), np.full(141, -1.75)), -1)
TRUCK_EGO = np.array([0.0, -1.75])


def truck_scene(copies, relevant=None, trucks=None, x0=-10.0, x1=70.0):
    """``relevant`` None: no intersection -- the only relevant lanelet is the ego lane's oncoming neighbour, id 2
    (fo_spawn_rules_ref.py:405-410).  A number r: an intersection whose incomings are the ego's lanelet and the first r of the
    oncoming lanelets in list order -- those r are the relevant ones (:397-404)"""
    lanes = oncoming_lanes(copies, x0, x1)
    inter = None
    if relevant is not None:
        inter = [{"id": 1, "incomings": [{"incoming": [1] + [ll.lanelet_id for ll in lanes[1:1 + relevant]], "right": [], "straight": [],
                                          "left": []}]}]
    return scene(lanes, trucks or [truck()], TRUCK_PATH, TRUCK_EGO, 0.0, 8.0, intersections=inter)


# ------------------------------------------------------------------------------------------------ running a scene
def checker(sc, sm, obs, cfg=None, cosy=None):
    """(SpawnRules, CellView, ego_cl) of the scene on the cell classes the device computed: the checker of ``TS._both``
    (``cosy``: through a caller's frame instead of the path's polyline frame)"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    from oracle.fo_spawn_rules_ref import CellView, SpawnRules
    cs = cosy if cosy is not None else PolylineCS(sc.path)
    view = CellView(sm.cell_class.cpu().numpy(), sm.window)

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
    rules = SpawnRules(cfg or TS.CFG, sc.path, cs, lane_yaw_at, lanelet_of, obs, lanelets=sc.lanelets, intersections=sc.intersections or [])
    return rules, view, cs.convert_to_curvilinear_coords(sc.ego[0], sc.ego[1])


def stage(torch, sc, cfg=None, cosy=None):
    """the scene through SensorModel + SpawnLocator.find_spawn_points(lazy=True): nobody reads the list.  Returns the raw
    device count, the unread list, the checker's list, and the parts.  ``cosy``: the caller's frame both sides project through
    (``accelerator.spawn.frame: caller``)"""
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    cfg = copy.deepcopy(cfg or TS.CFG)
    if cosy is not None:
        cfg["accelerator"]["spawn"]["frame"] = "caller"
    obs = FOObstacles(sc.obstacles)
    obs.update(0)
    sm = SensorModel(sc.lanelets, sc.path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, intersections=sc.intersections,
                     cell_size=sc.cell_size)
    sm.calc_visible_and_occluded_area(0, sc.ego, sc.yaw, obs)
    am = SimpleNamespace(scenario=SimpleNamespace(intersections=sc.intersections or []))
    sl = SpawnLocator(am, sc.path, cfg, sm, cosy_cl=cosy, fo_obstacles=obs)
    rules, view, ego_cl = checker(sc, sm, obs, cfg, cosy)
    pts = sl.find_spawn_points(sc.ego, sc.yaw, ego_cl, sc.v, lazy=True)
    torch.cuda.synchronize()
    raw = int(sl.batch.rule_n.cpu().item())
    ref = rules.find(view, sc.ego, ego_cl, sc.v, sc.yaw)
    return SimpleNamespace(raw=raw, pts=pts, ref=ref, view=view, rules=rules, sm=sm, sl=sl, obs=obs, ego_cl=ego_cl)


def both(torch, sc):
    """device list and checker list through the helper of tests/test_spawn_rules_gpu.py"""
    return TS._both(torch, sc.lanelets, sc.obstacles, sc.path, sc.ego, sc.yaw, sc.v, intersections=sc.intersections,
                    cell_size=sc.cell_size)


STEP_CFG = {"spawn_locator": dict(TS.CFG["spawn_locator"]),
            "agent_manager": dict(TS.CFG["agent_manager"], truck={"width": 2.5, "length": 9.0, "default_velocity": 8.0}),
            "accelerator": {"spawn": {"mode": "rules", "routes": 3, "max_rule_points": 8, "max_agents": 6}}}


def stack(torch, sc, spawn_mode="rules", metrics=None, ctx=None, seed=3):
    """sensor model + spawn locator + sweep on one context, and M = 130 candidates of T = 16 samples in front of the ego"""
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.sweep import MetricSweep
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    cfg = copy.deepcopy(STEP_CFG)
    cfg["accelerator"]["spawn"]["mode"] = spawn_mode
    ctx = ctx or N.Context(0)
    obs = FOObstacles(sc.obstacles)
    obs.update(0)
    sm = SensorModel(sc.lanelets, sc.path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, ctx=ctx, routes=3,
                     intersections=sc.intersections, cell_size=sc.cell_size)
    sl = SpawnLocator(None, sc.path, cfg, sm, fo_obstacles=obs, dt=0.1, horizon=(T - 1) * 0.1 + 0.05)
    assert sl.T == T
    kw = {} if metrics is None else {"metrics": metrics}
    sw = MetricSweep(VEH, 0.1, thresholds={"harm": 0.1, "risk": 1}, ctx=ctx, **kw)
    traj = SY.make_trajectories(M, T, 0.1, seed=seed, ego_pos=sc.ego, ego_yaw=sc.yaw)
    tr = [torch.as_tensor(traj[k]).cuda() for k in ("x", "y", "theta", "v", "a")]
    sm.upload_obstacles(obs)
    return SimpleNamespace(ctx=ctx, obs=obs, sm=sm, sl=sl, sw=sw, tr=tr, traj=traj, cfg=cfg, sc=sc)
