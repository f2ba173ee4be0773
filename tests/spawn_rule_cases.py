"""The scenes of tests/golden/spawn_rule_bodies.npz, rebuilt from the numbers the fixture stores: shared by the generator
(tests/golden/gen_golden.py rules), the CPU replay (tests/test_spawn_rule_bodies_cpu.py) and the GPU replay
(tests/test_spawn_rules_gpu.py).  Nothing here knows what the spawn rules decide: maps, obstacles, the curvilinear frame and
-- on the CPU -- the cell classes of the step exactly as the device computes them (the scene oracle with the sensor model's
raster origin, 1.5 r window, 64-gon footprint, transparent enclosed holes and exact cell visibility)."""
import math
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "spawn_rule_bodies.npz")
MAPS = ("scenario1", "scenario2", "scenario3", "straight", "t_right", "t_left", "two_way", "urban", "bend_42", "bend_47", "hook_left")
TYPES = ("car", "truck", "bus", "bicycle", "pedestrian", "parkedVehicle", "motorcycle")
INTENTIONS = ("straight ahead", "left turn", "right turn")
SLOTS = ("find", "dynamic", "static", "turn")             # the call a recorded result belongs to
NONE, POINTS, RAISES, NOT_RUN = 0, 1, 2, 3                # status of a recorded call
SENSOR_RADIUS = 50.0
AGENT_MANAGER = {"pedestrian": {"width": 0.5, "length": 0.3, "default_velocity": 1.4},
                 "bicycle": {"width": 0.9, "length": 2.0, "default_velocity": 5.0},
                 "car": {"width": 2.0, "length": 4.8, "default_velocity": 10.0},
                 "prediction": {"variance_factor": 1.05, "size_factor_length_s": 1.2, "size_factor_width_s": 1.3,
                                "size_factor_length_l": 1.4, "size_factor_width_l": 2.5}}


def _straight(S, lid, x0, x1, y_lo, y_hi, n=41):
    xs = np.linspace(x0, x1, n)
    return S.Lanelet(lid, np.stack((xs, np.full(n, y_hi)), -1), np.stack((xs, np.full(n, y_lo)), -1))


def synthetic_map(name):
    """the maps of the known-answer tests (tests/test_spawn_rules.py): (lanelets, intersections)"""
    from frenetix_occlusion import scenario as S
    if name == "straight":
        return [_straight(S, 1, -10, 120, -3.5, 0.0), _straight(S, 2, -10, 120, 0.0, 3.5)], []
    if name in ("t_right", "t_left"):
        main = [_straight(S, 1, -40, 40, -3.5, 0.0), _straight(S, 2, -40, 40, 0.0, 3.5)]
        ys = np.linspace(-3.5, -43.5, 41)
        side = [S.Lanelet(3, np.stack((np.full(41, 13.5), ys), -1), np.stack((np.full(41, 10.0), ys), -1)),
                S.Lanelet(4, np.stack((np.full(41, 17.0), ys), -1), np.stack((np.full(41, 13.5), ys), -1))]
        if name == "t_left":
            m = np.array([1.0, -1.0])
            return [S.Lanelet(ll.lanelet_id, ll.right * m, ll.left * m) for ll in main + side], []
        return main + side, []
    if name == "two_way":
        xs = np.linspace(-10, 70, 41)
        lane1 = S.Lanelet(1, np.stack((xs, np.zeros(41)), -1), np.stack((xs, np.full(41, -3.5)), -1))
        lane2 = S.Lanelet(2, np.stack((xs[::-1], np.zeros(41)), -1), np.stack((xs[::-1], np.full(41, 3.5)), -1))
        lane1.adj_left, lane1.adj_left_same_direction = 2, False
        lane2.adj_left, lane2.adj_left_same_direction = 1, False
        return [lane1, lane2], []
    if name.startswith("bend_"):
        bounds = [bend_line(BEND_DEG[name], v) for v in (-3.5, 0.0, 3.5)]
        return [S.Lanelet(1, bounds[1], bounds[0]), S.Lanelet(2, bounds[2], bounds[1])], []
    if name == "hook_left":
        # a mitred 90 degree left bend: lanelet 1 (3.5 m) on the outside, the oncoming lanelet 2 (HOOK_WIDTH) on the inside, and
        # no lanelet in the angle between the two legs of lanelet 2
        mir = np.array([1.0, -1.0])
        axis, outer, inner = (bend_line(90.0, v) * mir for v in (0.0, 3.5, -HOOK_WIDTH))
        lane1, lane2 = S.Lanelet(1, axis, outer), S.Lanelet(2, axis[::-1].copy(), inner[::-1].copy())
        lane1.adj_left, lane1.adj_left_same_direction = 2, False
        lane2.adj_left, lane2.adj_left_same_direction = 1, False
        return [lane1, lane2], []
    raise KeyError(name)


HOOK_WIDTH = 2.0
BEND_DEG = {"bend_42": 42.5, "bend_47": 47.5}       # either side of the turn rule's 45 degrees


def bend_line(deg, v, n=21, leg=40.0):
    """a line v metres left of a road axis that runs along +x to the origin and on at a heading of -deg degrees (a right bend
    with a mitred corner): a vertex every leg / (n - 1) metres"""
    b = math.radians(deg)
    dir_b, n_b = np.array([math.cos(b), -math.sin(b)]), np.array([math.sin(b), math.cos(b)])
    corner = v * (np.array([0.0, 1.0]) + n_b) / (1.0 + math.cos(b))
    t = np.linspace(-leg, 0.0, n)
    return np.concatenate((corner[None] + t[:, None] * np.array([[1.0, 0.0]]), corner[None] + (-t[::-1][1:, None]) * dir_b[None]))


def bend_path(deg, v=-1.75, rho=4.0):
    """a reference path along bend_line(deg, v) with the corner rounded at radius rho (curvature 1 / rho: a right turn)"""
    b = math.radians(deg)
    dir_b = np.array([math.cos(b), -math.sin(b)])
    corner = v * (np.array([0.0, 1.0]) + np.array([math.sin(b), math.cos(b)])) / (1.0 + math.cos(b))
    tan_len = rho * math.tan(b / 2.0)
    start = corner - np.array([tan_len, 0.0])
    phi = np.linspace(0.0, b, 12)
    arc = np.stack((start[0] + rho * np.sin(phi), start[1] - rho + rho * np.cos(phi)), -1)
    lead = np.stack((np.linspace(start[0] - 35.0, start[0], 71), np.full(71, start[1])), -1)
    tail = arc[-1][None] + np.linspace(0.5, 35.0, 70)[:, None] * dir_b[None]
    return np.concatenate((lead[:-1], arc, tail))


_MAP_CACHE = {}


def load_map(index):
    """(lanelets, intersections, obstacles of the scenario or None) of MAPS[index], cached"""
    from frenetix_occlusion import scenario as S
    if index not in _MAP_CACHE:
        name = MAPS[index]
        if name.startswith("scenario"):
            sc = S.load_geometry_npz(os.path.join(GOLDEN, name + "_geometry.npz"))
            _MAP_CACHE[index] = (sc.lanelets, sc.intersections or [], sc.obstacles)
        elif name == "urban":
            sc = S.synthetic_urban_grid()
            _MAP_CACHE[index] = (sc.lanelets, getattr(sc, "intersections", None) or [], sc.obstacles)
            _MAP_CACHE["urban ego"] = sc.ego_initial
        else:
            _MAP_CACHE[index] = synthetic_map(name) + (None,)
    return _MAP_CACHE[index]


def urban_ego_initial():
    load_map(MAPS.index("urban"))
    return _MAP_CACHE["urban ego"]


def make_case(map_index, ego, yaw, v, step, path, obstacle_rows=(), switches=(True, True, True), max_static=1, max_dynamic=1,
              frame=0, n_rays=720, cell_size=0.5):
    """one scene.  obstacle_rows (synthetic maps only): id, role (0 static, 1 dynamic), index into TYPES, length, width, x, y,
    yaw, v; frame 0 = the polyline frame of the path, 1 = a caller's frame with interpolated normals"""
    from frenetix_occlusion import scenario as S
    lanelets, intersections, obstacles = load_map(map_index)
    rows = np.asarray(obstacle_rows, dtype=np.float64).reshape(-1, 9)
    if obstacles is None:
        obstacles = [S.Obstacle(int(r[0]), "dynamic" if r[1] else "static", TYPES[int(r[2])], float(r[3]), float(r[4]), 0,
                                np.array([r[5], r[6], r[7], r[8]]), np.zeros((0, 4))) for r in rows]
    cfg = {"spawn_locator": {"spawn_point_behind_dynamic_obstacle": bool(switches[0]),
                             "spawn_point_behind_static_obstacle": bool(switches[1]),
                             "spawn_points_behind_turn": bool(switches[2]),
                             "max_static_spawn_points": int(max_static), "max_dynamic_spawn_points": int(max_dynamic)},
           "agent_manager": AGENT_MANAGER,
           "accelerator": {"spawn": {"mode": "rules", "frame": "caller" if frame else "polyline"}}}
    return SimpleNamespace(map_index=int(map_index), lanelets=lanelets, intersections=intersections, obstacles=obstacles,
                           obstacle_rows=rows, ego=np.asarray(ego, dtype=np.float64), yaw=float(yaw), v=float(v), step=int(step),
                           path=np.asarray(path, dtype=np.float64), switches=tuple(bool(x) for x in switches),
                           max_static=int(max_static), max_dynamic=int(max_dynamic), frame=int(frame), n_rays=int(n_rays),
                           cell_size=float(cell_size), cfg=cfg)


def frame_of(case):
    """the curvilinear frame object of a case"""
    if case.frame:
        from test_caller_frame_cpu import InterpolatedNormalFrame
        return InterpolatedNormalFrame(case.path)
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    return PolylineCS(case.path)


_GEO_CACHE = {}


def _geometry(oracle, case):
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import HoleIndex
    key = (case.map_index, case.cell_size)
    if key not in _GEO_CACHE:
        g = S.MapGeometry.from_lanelets(case.lanelets)
        cs, margin, xy = case.cell_size, 2.0 * case.cell_size, g.poly_xy
        x0 = math.floor((xy[:, 0].min() - margin) / cs) * cs
        y0 = math.floor((xy[:, 1].min() - margin) / cs) * cs
        nx = int(math.ceil((xy[:, 0].max() + margin - x0) / cs))
        ny = int(math.ceil((xy[:, 1].max() + margin - y0) / cs))
        raster = oracle.road_raster(g.poly_off, g.poly_xy, x0, y0, cs, nx, ny)
        _GEO_CACHE[key] = (g, HoleIndex(g), x0, y0, nx, ny, raster, S.lane_yaw_raster(case.lanelets, x0, y0, cs, nx, ny))
    return _GEO_CACHE[key]


def lane_queries(case, x0, y0, nx, ny, lane_yaw):
    """(lane_yaw_at, lanelet_of) as the checker takes them: the lane-yaw raster at the cell of a point (None off the road), the
    first lanelet of the list that holds a point"""
    from oracle.fo_spawn_rules_ref import points_in_polygon
    cs = case.cell_size

    def lane_yaw_at(xy):
        ix, iy = int(math.floor((xy[0] - x0) / cs)), int(math.floor((xy[1] - y0) / cs))
        if not (0 <= ix < nx and 0 <= iy < ny) or np.isnan(lane_yaw[iy, ix]):
            return None
        return float(lane_yaw[iy, ix])

    def lanelet_of(xy):
        for ll in case.lanelets:
            if points_in_polygon(np.asarray(xy, float).reshape(1, 2), ll.polygon)[0]:
                return ll
        return None
    return lane_yaw_at, lanelet_of


def cpu_scene(oracle, case):
    """the step's cell classes, obstacle visibility and lane queries on the CPU: (CellView, FOObstacles, lane_yaw_at,
    lanelet_of)"""
    from frenetix_occlusion.sensor_model import CellWindow, footprint_ranges, half_fan_dirs, ray_dirs
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    from oracle.fo_spawn_rules_ref import CellView
    g, holes, x0, y0, nx, ny, raster, lane_yaw = _geometry(oracle, case)
    cs, r, ego, yaw = case.cell_size, SENSOR_RADIUS, case.ego, case.yaw
    obs = FOObstacles(case.obstacles)
    obs.update(case.step)
    corn, cen, flags = obs.arrays() if len(obs) else (np.zeros((0, 4, 2)), np.zeros((0, 2)), np.zeros(0, np.uint8))
    reach = 1.5 * r
    ix0, iy0 = int(math.floor((ego[0] - reach - x0) / cs)), int(math.floor((ego[1] - reach - y0) / cs))
    n = int(math.ceil(2.0 * reach / cs)) + 1
    dirs, rmax = ray_dirs(case.n_rays, yaw, 360.0), footprint_ranges(case.n_rays, yaw, 360.0, r)
    rings = holes.enclosed(ego, yaw, 360.0, r)
    skip = holes.edge_skip(rings) if rings else None
    rng, hid, _ = oracle.raycast(g.edges, corn, flags, ego, dirs, r, rmax=rmax, edge_skip=skip)
    cls, _ = oracle.grid(raster, x0, y0, cs, ix0, iy0, n, n, ego, np.array([math.cos(yaw), math.sin(yaw)]), r, True, dirs, rng,
                         exact=dict(hit_id=hid, edges=g.edges, ocorn=corn, oflags=flags, rmax=rmax, edge_skip=skip,
                                    half_dirs=half_fan_dirs(yaw), edge_line=g.edge_line))
    if len(obs):
        vis = oracle.obstacle_visibility(g.edges, corn, cen, flags, ego, r, True, dirs, edge_skip=skip, hit_id=hid)
        for o, vflag in zip(obs, vis):
            o.current_visible = bool(vflag)
    lane_yaw_at, lanelet_of = lane_queries(case, x0, y0, nx, ny, lane_yaw)
    return CellView(cls, CellWindow(x0, y0, cs, ix0, iy0, n, n)), obs, lane_yaw_at, lanelet_of


def class_counts(cls):
    """the fixture's checksum of a step's cell classes: cells with the road / visible / occluded bit"""
    cls = np.asarray(cls)
    return np.array([int(((cls & b) != 0).sum()) for b in (1, 2, 4)], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the fixture
def save_fixture(path, cases, records, lines_hit, lines_executable):
    """cases: list of make_case(); records: per case dict(intention=, counts=, calls={slot: (status, exception name, points)})
    with points = list of (agent_type, source, position, cl_pos or None, orientation or None)"""
    paths, path_id, seen = [], [], {}
    for c in cases:
        key = c.path.tobytes()
        if key not in seen:
            seen[key] = len(paths)
            paths.append(c.path)
        path_id.append(seen[key])
    out = {"n_cases": np.int64(len(cases)),
           "path_off": np.cumsum([0] + [len(p) for p in paths]), "path_xy": np.concatenate(paths),
           "case": np.array([[c.map_index, c.step, *c.ego, c.yaw, c.v, pid, *[float(s) for s in c.switches], c.max_static,
                              c.max_dynamic, c.frame, c.n_rays, c.cell_size] for c, pid in zip(cases, path_id)], dtype=np.float64),
           "obst_off": np.cumsum([0] + [len(c.obstacle_rows) for c in cases]),
           "obst_rows": np.concatenate([c.obstacle_rows for c in cases]).reshape(-1, 9),
           "class_counts": np.array([r["counts"] for r in records], dtype=np.int64),
           "took_multipoint": np.array([bool(r["multipoint"]) for r in records]),
           "took_multilinestring": np.array([bool(r["multiline"]) for r in records]),
           "intention": np.array([INTENTIONS.index(r["intention"]) if r["intention"] in INTENTIONS else -1 for r in records]),
           "lines_hit": np.array(sorted(lines_hit), dtype=np.int64),
           "lines_executable": np.array(sorted(lines_executable), dtype=np.int64)}
    status, exc, rows, types, sources = [], [], [], [], []
    for k, r in enumerate(records):
        st_row, ex_row = [], []
        for j, slot in enumerate(SLOTS):
            st, name, pts = r["calls"][slot]
            st_row.append(st)
            ex_row.append(name or "")
            for t, src, pos, cl, ori in pts:
                rows.append([k, j, pos[0], pos[1], *(cl if cl is not None else (np.nan, np.nan)), np.nan if ori is None else ori])
                types.append(t)
                sources.append(src)
        status.append(st_row)
        exc.append(ex_row)
    out["status"] = np.array(status, dtype=np.int64)
    out["exception"] = np.array(exc, dtype="U24")
    out["points"] = np.array(rows, dtype=np.float64).reshape(-1, 7)
    out["point_type"] = np.array(types, dtype="U12")
    out["point_source"] = np.array(sources, dtype="U40")
    np.savez_compressed(path, **out)
    return out


def load_fixture(path=FIXTURE):
    """list of (case, record) in the fixture's order, plus the raw arrays"""
    z = np.load(path, allow_pickle=False)
    out = []
    for k in range(int(z["n_cases"])):
        row = z["case"][k]
        pid = int(row[6])
        case = make_case(int(row[0]), row[2:4], row[4], row[5], int(row[1]), z["path_xy"][z["path_off"][pid]:z["path_off"][pid + 1]],
                         z["obst_rows"][z["obst_off"][k]:z["obst_off"][k + 1]], row[7:10] != 0.0, int(row[10]), int(row[11]),
                         int(row[12]), int(row[13]), float(row[14]))
        calls = {}
        for j, slot in enumerate(SLOTS):
            sel = np.nonzero((z["points"][:, 0] == k) & (z["points"][:, 1] == j))[0]
            pts = [(str(z["point_type"][i]), str(z["point_source"][i]), z["points"][i, 2:4],
                    None if np.isnan(z["points"][i, 4]) else z["points"][i, 4:6],
                    None if np.isnan(z["points"][i, 6]) else float(z["points"][i, 6])) for i in sel]
            calls[slot] = (int(z["status"][k, j]), str(z["exception"][k, j]), pts)
        inten = int(z["intention"][k])
        out.append((case, dict(intention=INTENTIONS[inten] if inten >= 0 else None, counts=z["class_counts"][k], calls=calls,
                              multipoint=bool(z["took_multipoint"][k]), multiline=bool(z["took_multilinestring"][k]))))
    return out, z


def points_of(result):
    """a rule method's return value (None, a SpawnPoint or a list with Nones) as the fixture's point tuples"""
    if result is None:
        return []
    seq = result if isinstance(result, list) else [result]
    return [(p.agent_type, p.source, np.asarray(p.position, dtype=np.float64),
             None if p.cl_pos is None else np.asarray(p.cl_pos, dtype=np.float64).reshape(-1)[:2],
             None if p.orientation is None else float(p.orientation)) for p in seq if p is not None]
