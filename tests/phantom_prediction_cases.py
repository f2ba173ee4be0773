"""The cases of the phantom prediction tests, built once and shared by tests/test_phantom_predictions_cpu.py (reference against
oracle and host path) and tests/test_phantom_predictions_gpu.py (fo_scene_spawn_rule_agents / fo_scene_spawn against the
reference): synthetic maps in the form the C ABI takes (lanelet polygons, route table, centre lines) and point records.

Three maps:
  LONG    14 lanelets (rectangles 64 m apart), routes of 2 .. 600 vertices on a 1/8 m grid with 0.5 m segments: straight pieces, one
          90 degree bend with its corner at vertex 64, three hairpins whose legs put segment i opposite segment i + 64 (same lane of
          the wave), 9 opposite 70 (the higher index in the lower lane) and 198 opposite 262 (beyond the 256 vertices staged in LDS);
          route tables [nv, 0, nv'], [nv, 1, 0], [1, 0, 0] and a lanelet without routes
  MANY    130 thin strips; 3 and 70 overlap, 64 and 100 overlap
  RANDOM  12 lanelets with three routes of 2 .. 300 vertices each, all curving to one side, points on the inner side (no point
          sits in the wedge behind a vertex, where two segments tie at the vertex in rationals but not in float64)
A launch = (map, records, path, T, dt, per-type speeds): what one call of fo_scene_spawn_rule_agents gets."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

import ref_phantom_predictions as R

H = 0.5                      # segment length of the designed routes (a power of two: arc lengths, feet and ties are exact)
PITCH = 64.0                 # lanelet p of LONG: baseline y = PITCH p, polygon y in [-16, 40] around it, x in [-128, 336]
CAR, BIKE, PED = R.TYPE_CAR, R.TYPE_BICYCLE, R.TYPE_PED
NAN = float("nan")
VAR0, FACTOR = 0.1, 1.05
TYPES = dict(speed=(10.0, 5.0, 1.4), raw_l=(4.8, 2.0, 0.3), raw_w=(2.0, 0.9, 0.5),
             infl_l=(4.8 * 1.2, 2.0 * 1.4, 0.3 * 1.2), infl_w=(2.0 * 1.3, 0.9 * 2.5, 0.5 * 1.3))
TYPES_EXACT = dict(TYPES, speed=(8.0, 4.0, 1.0))       # with dt = 0.125: whole metres / half metres per sample


# ------------------------------------------------------------------------------------------------ polylines
def straight_line(nv, x0, y0, h=H):
    return np.stack((x0 + h * np.arange(nv), np.full(nv, y0)), -1)


def bend_line(nv, corner, x0, y0):
    """+x for `corner` segments, then +y: segments corner - 1 and corner meet at the corner vertex"""
    i = np.arange(nv)
    return np.stack((x0 + H * np.minimum(i, corner), y0 + H * np.maximum(i - corner, 0)), -1)


def hairpin_line(nv, a, n_conn, x0, y0, w=4.0):
    """out along +x for `a` segments, up by w in n_conn segments, back along -x: the outbound segment i lies under the return
    segment 2 a + n_conn - 1 - i"""
    pts = [(x0 + H * i, y0) for i in range(a + 1)]
    pts += [(x0 + H * a, y0 + w * (c + 1) / n_conn) for c in range(n_conn - 1)]
    j = 0
    while len(pts) < nv:
        pts.append((x0 + H * (a - j), y0 + w))
        j += 1
    return np.array(pts)


def arc_length(p):
    return np.concatenate(([0.0], np.cumsum(np.hypot(np.diff(p[:, 0]), np.diff(p[:, 1])))))


def rect(x0, x1, y0, y1):
    return np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], dtype=np.float64)


def make_scene(polys, routes, centers):
    """routes[p] = list of R polylines (None = no such route); centers[p] = polyline ([n, 2], n may be 0 or 1)"""
    Rn = 3
    first, count = np.zeros(len(polys) * Rn, dtype=np.int32), np.zeros(len(polys) * Rn, dtype=np.int32)
    xy, ss, nv = [], [], 0
    for p, rs in enumerate(routes):
        for r, line in enumerate(rs):
            if line is None:
                continue
            first[p * Rn + r], count[p * Rn + r] = nv, len(line)
            xy.append(np.asarray(line, dtype=np.float64))
            ss.append(arc_length(xy[-1]))
            nv += len(line)
    coff = np.zeros(len(polys) + 1, dtype=np.int32)
    coff[1:] = np.cumsum([len(c) for c in centers])
    cxy = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 2) for c in centers])
    return R.Scene([np.asarray(p, dtype=np.float64) for p in polys], Rn, first, count, np.concatenate(xy), np.concatenate(ss), coff, cxy)


@dataclass
class Launch:
    name: str
    map: str                 # LONG / MANY / RANDOM
    points: np.ndarray       # [max_points, 8]
    n_points: int
    tags: list               # per live point
    path: np.ndarray
    T: int
    dt: float
    types: dict = field(default_factory=lambda: TYPES)
    designed: bool = True


def rec(typ, x, y, orientation=NAN, src=0):
    return [float(typ), float(x), float(y), orientation, 0.0, 0.0, float(src), -1.0]


# ------------------------------------------------------------------------------------------------ LONG
LONG_ROUTES = {1: 64, 2: 65, 3: 66, 4: 129, 5: 256, 6: 257, 7: 600}      # lanelet -> vertices of its straight route 0
L_BEND, L_HAIR1, L_HAIR2, L_ONE, L_NONE, L_HAIR3 = 8, 9, 10, 11, 12, 13
HAIRPINS = {L_HAIR1: (129, 40, 1, 8, 72), L_HAIR2: (129, 39, 2, 9, 70), L_HAIR3: (470, 230, 1, 198, 262)}   # nv, a, n_conn, i, partner


@functools.lru_cache(None)
def long_scene():
    P = 14
    y = lambda p: PITCH * p
    routes = [[None] * 3 for _ in range(P)]
    routes[0][0] = straight_line(2, 0.0, y(0))
    for p, nv in LONG_ROUTES.items():
        routes[p][0] = straight_line(nv, 0.0, y(p))
    routes[3][2] = bend_line(129, 64, -40.125, y(3) - 6.125)     # [66, 0, 129]: off the grid of the points, its legs far from them
    routes[4][1] = np.array([[1.0, y(4) + 3.0]])                  # [129, 1, 0]
    routes[L_BEND][0] = bend_line(600, 64, 0.0, y(L_BEND))       # (600: no sample from the corner lands on the route's end)
    for p, (nv, a, nc, _, _) in HAIRPINS.items():
        routes[p][0] = hairpin_line(nv, a, nc, 0.0, y(p))
    routes[L_ONE][0] = np.array([[5.0, y(L_ONE)]])                # [1, 0, 0]
    polys = [rect(-128.0, 336.0, y(p) - 16.0, y(p) + 40.0) for p in range(P)]
    centers = [routes[p][0] if routes[p][0] is not None else np.zeros((0, 2)) for p in range(P)]
    return make_scene(polys, routes, centers)


PATH_Y = -40.0


@functools.lru_cache(None)
def long_paths():
    """reference paths of 2, 65, 66, 129 and 300 vertices below lanelet 0 (y = -40): one segment, a straight piece, a bend with its
    corner at vertex 64, the hairpins 8 | 72 and 9 | 70"""
    return {2: np.array([[-10.0, PATH_Y], [300.0, PATH_Y]]), 65: straight_line(65, 0.0, PATH_Y), 66: bend_line(66, 64, 0.0, PATH_Y),
            129: hairpin_line(129, 40, 1, 0.0, PATH_Y), 300: hairpin_line(300, 39, 2, 0.0, PATH_Y)}


def _above(line, i, d):
    """the point at distance d to the left of the middle of segment i"""
    a, b = line[i], line[i + 1]
    e = (b - a) / np.hypot(*(b - a))
    return 0.5 * (a + b) + d * np.array([-e[1], e[0]])


def long_points(path):
    """(records, tags, core mask): the designed points of LONG against `path`"""
    sc = long_scene()
    y = lambda p: PITCH * p
    out, veh = [], [CAR, BIKE]
    add = lambda tag, r, core=False: out.append((tag, r, core))
    route = lambda p, r=0: sc.xy[sc.first[3 * p + r]:sc.first[3 * p + r] + sc.count[3 * p + r]]
    add("nv=2", rec(CAR, 0.25, y(0) + 1.0), True)
    for p, nv in LONG_ROUTES.items():                              # closest segment at the lane / pass boundaries
        idx = sorted({i for i in (0, 63, 64, 127, 128, 255, 256, 320, nv - 2) if i <= nv - 2})
        for n, i in enumerate(idx):
            q = _above(route(p), i, 1.0 if n % 2 == 0 else -1.0)
            add(f"nv={nv} seg={i}", rec(veh[(n + p) % 2], q[0], q[1]), (nv, i) in ((257, 128), (600, 598), (66, 63)))
    for d in (-2.0, -0.5, -0.25, 0.0, 0.25, 0.5, 2.0):             # lateral target, on the 66-vertex route (and its bend route 2)
        add(f"d0={d}", rec(CAR, 10.25, y(3) + d), d in (2.0, -0.25, 0.25))
    add("before start", rec(CAR, -3.0, y(5) + 1.0), True)
    add("beyond end", rec(BIKE, 32.0 + 3.0, y(2) - 1.0), True)
    add("ends inside", rec(CAR, 10.25, y(2) + 0.125), True)
    add("[129,1,0]", rec(CAR, 20.25, y(4) - 0.125), True)
    b = route(L_BEND)
    add("bend tie 63|64", rec(CAR, b[64, 0] + 2.0, b[64, 1] - 1.0), True)
    add("bend tie 63|64 mirrored", rec(BIKE, b[64, 0] + 1.0, b[64, 1] - 2.0))
    for i in (0, 63, 64, 127):
        q = _above(b, i, -1.0)                                     # (outside the bend: the other leg is farther)
        add(f"bend seg={i}", rec(CAR, q[0], q[1]), i == 64)
    for p, (nv, a, nc, i, j) in HAIRPINS.items():
        add(f"hairpin tie {i}|{j}", rec(CAR, H * (i + 0.5), y(p) + 2.0), True)
        add(f"hairpin seg={j}", rec(BIKE, H * (i + 0.5), y(p) + 3.0), True)
        add(f"hairpin seg={i}", rec(BIKE, H * (i + 0.5), y(p) + 1.0))
    add("route table [1,0,0]", rec(CAR, 7.0, y(L_ONE) + 2.0), True)
    add("lanelet without routes", rec(BIKE, 7.0, y(L_NONE) + 2.0), True)
    add("vehicle off every lanelet", rec(CAR, 30.25, PATH_Y - 12.0), True)
    # pedestrians: heading towards the path (closest segment at the same boundaries, ties between the legs of a hairpin)
    n = len(path)
    for i in sorted({i for i in (0, 63, 64, 127, 128, n - 2) if i <= n - 2}):
        q = _above(path, i, -1.0 if (n == 66 and i >= 64) else 1.0)
        add(f"ped path seg={i}", rec(PED, q[0], q[1]), True)
    add("ped between the legs", rec(PED, H * 8.5, PATH_Y + 2.0), True)
    add("ped between the legs 9|70", rec(PED, H * 9.5, PATH_Y + 2.0), True)
    add("ped on the curve", rec(PED, 4.25, PATH_Y), True)
    add("ped above the path: lower half plane", rec(PED, 4.25, PATH_Y + 1.5), True)
    add("ped below the path", rec(PED, 4.25, PATH_Y - 3.0), True)
    add("ped with its own orientation", rec(PED, 3.0, PATH_Y + 7.0, orientation=1.25), True)
    add("ped lane_center", rec(PED, 20.25, y(6) + 3.0, src=R.SRC_LEFT), True)
    add("ped lane_center on the hairpin", rec(PED, H * 8.5, y(L_HAIR1) + 2.0, src=R.SRC_RIGHT), True)
    add("ped lane_center, one-vertex centre", rec(PED, 9.0, y(L_ONE) + 3.0, src=R.SRC_LEFT), True)
    add("ped lane_center, empty centre", rec(PED, 9.0, y(L_NONE) + 3.0, src=R.SRC_RIGHT), True)
    add("ped lane_center off every lanelet", rec(PED, 50.25, PATH_Y - 9.0, src=R.SRC_LEFT), True)
    add("ped on a lanelet, mode ref_path", rec(PED, 20.25, y(0) + 3.0), True)
    return out


def long_end_points(T):
    """with dt = 0.125 and 8 m/s (one metre per sample) on the 129-vertex straight route (s_end = 64): the route ends exactly on
    the last sample (len = T), one sample earlier (len = T - 1), and at once (len = 1); bicycles (0.5 m per sample) likewise"""
    y0, s_end = PITCH * 4, 64.0
    out = []
    for typ, step in ((CAR, 1.0), (BIKE, 0.5)):
        for L in (T, T - 1, 1):
            s0 = s_end - step * (L - 1)
            if s0 >= 0.0:
                out.append((f"end on sample: len={L} T={T}", rec(typ, s0, y0 + 1.0), True))
    out.append((f"end: beyond T={T}", rec(CAR, s_end + 2.0, y0 - 1.0), True))
    out.append((f"whole horizon on the 600-vertex route T={T}", rec(CAR, 100.25, PITCH * 7 + 0.125), True))
    return out


def _launch(name, mp_, pts, path, T, dt, types=TYPES, extra=3, designed=True):
    recs = np.array([p[1] for p in pts] + [rec(CAR, 1.0, 1.0)] * extra)      # `extra` records beyond *d_n_points: never read as points
    return Launch(name, mp_, recs, len(pts), [p[0] for p in pts], np.ascontiguousarray(path, dtype=np.float64), T, dt, types, designed)


# ------------------------------------------------------------------------------------------------ MANY
@functools.lru_cache(None)
def many_scene():
    polys, routes = [], []
    for p in range(130):
        if p == 70:
            polys.append(rect(40.0, 41.0, 0.0, 20.0))
            line = np.array([[40.5, 0.0], [40.5, 10.0], [40.5, 20.0]])
        elif p == 100:
            polys.append(rect(44.0, 45.0, 120.0, 140.0))
            line = np.array([[44.5, 120.0], [44.5, 130.0], [44.5, 140.0]])
        else:
            x1 = 64.0 if p in (3, 64) else 32.0
            polys.append(rect(0.0, x1, 2.0 * p, 2.0 * p + 1.0))
            xs = np.arange(0.0, x1 + 1.0, 8.0)
            line = np.stack((xs if p % 2 == 0 else xs[::-1], np.full(len(xs), 2.0 * p + 0.5)), -1)
        routes.append([line, None, None])
    return make_scene(polys, routes, [r[0] for r in routes])


MANY_PATH = np.array([[-5.0, -10.0], [-5.0, 100.0], [-5.0, 300.0]])


def many_points():
    s = lambda p: 2.0 * p + 0.625
    pts = [("lanelet 0", rec(CAR, 4.25, s(0))), ("lanelet 63", rec(BIKE, 12.25, s(63))), ("lanelet 64", rec(CAR, 4.25, s(64))),
           ("lanelet 129", rec(BIKE, 20.25, s(129))), ("overlap 3|70 -> 3", rec(CAR, 40.5, s(3))),
           ("overlap 64|100 -> 64", rec(CAR, 44.5, s(64))), ("70 alone", rec(BIKE, 40.625, 1.625)), ("100 alone", rec(CAR, 44.375, 121.5)),
           ("on none", rec(CAR, 36.0, 1.5)), ("ped lane_center 64|100", rec(PED, 44.5, s(64) + 0.25, src=R.SRC_LEFT)),
           ("ped lane_center 129", rec(PED, 20.25, s(129) + 0.25, src=R.SRC_RIGHT)),
           ("ped lane_center on none", rec(PED, 36.0, 1.5, src=R.SRC_LEFT))]
    return [(t, r, True) for t, r in pts]


# ------------------------------------------------------------------------------------------------ RANDOM
RANDOM_SEED = 20241


def _curved(rng, nv, x0, y0, th0, kappa, sign):
    th = th0 + np.concatenate(([0.0], np.cumsum(sign * kappa * rng.uniform(0.5, 1.0, nv - 2)))) if nv > 2 else np.array([th0])
    l = rng.uniform(0.5, 1.5, nv - 1)
    p = np.zeros((nv, 2))
    p[0] = (x0, y0)
    p[1:] = p[0] + np.cumsum(l[:, None] * np.stack((np.cos(th), np.sin(th)), -1), axis=0)
    return p


@functools.lru_cache(None)
def random_block():
    """(scene, path, [(tag, record, T)]): 12 lanelets 1 000 m apart, three routes each from one start pose, route r turning (r + 1)
    times as fast as route 0, always to the same side; the points lie on that side of the tightest route"""
    rng = np.random.default_rng(RANDOM_SEED)
    polys, routes, pts = [], [], []
    forced = {0: (2, 40, 300), 1: (270, 257, 256), 2: (65, 64, 129)}
    for L in range(12):
        x0, sign, th0 = 1000.0 * L, (1.0 if L % 2 == 0 else -1.0), rng.uniform(-math.pi, math.pi)
        nvs = forced.get(L, tuple(int(v) for v in rng.integers(2, 301, 3)))
        rs = [_curved(rng, nv, x0, 0.0, th0, 0.0012 * (r + 1), sign) for r, nv in enumerate(nvs)]
        polys.append(rect(x0 - 450.0, x0 + 450.0, -450.0, 450.0))
        routes.append(rs)
        tight = rs[2]
        st = arc_length(tight)
        reach = 0.9 * min(arc_length(r)[-1] for r in rs)          # (beyond the end of a route the clamped foot IS its last vertex:
        for _ in range(6):                                         #  s0 against s_end is then a matter of the last bit)
            sa = rng.uniform(0.05, 1.0) * reach
            i = min(int(np.searchsorted(st, sa, side="right")) - 1, len(tight) - 2)
            a, b = tight[i], tight[i + 1]
            e = (b - a) / np.hypot(*(b - a))
            side = sign if len(tight) > 2 else 1.0
            q = a + (sa - st[i]) * e + side * rng.choice([rng.uniform(0.05, 1.0), rng.uniform(1.0, 3.0)]) * np.array([-e[1], e[0]])
            pts.append((f"random lanelet {L}", rec(CAR if rng.random() < 0.6 else BIKE, q[0], q[1])))
    path = _curved(rng, 150, -300.0, -600.0, 0.3, 0.004, 1.0)
    for k in range(8):                                               # pedestrians on the inner side of the path
        i = int(rng.integers(0, 148))
        a, b = path[i], path[i + 1]
        e = (b - a) / np.hypot(*(b - a))
        q = a + rng.uniform(0.1, 0.9) * (b - a) + rng.uniform(0.5, 6.0) * np.array([-e[1], e[0]])
        pts.insert(9 * k, (f"random pedestrian {k}", rec(PED, q[0], q[1])))
    scene = make_scene(polys, routes, [r[0] for r in routes])
    return scene, path, [(t, r, (31, 65)[n % 2]) for n, (t, r) in enumerate(pts)]


# ------------------------------------------------------------------------------------------------ all launches
SCENES = {"LONG": long_scene, "MANY": many_scene, "RANDOM": lambda: random_block()[0]}
HORIZONS = ((1, 2), (2, 65), (31, 129), (41, 300), (64, 66), (65, 300), (130, 129))       # T, vertices of the launch's path (dt = 0.1)


@functools.lru_cache(None)
def launches():
    out = []
    paths = long_paths()
    for T, npath in HORIZONS:
        pts = long_points(paths[npath])
        if T not in (31, 65):
            pts = [p for p in pts if p[2]]
        out.append(_launch(f"LONG T={T} dt=0.1 path={npath}", "LONG", pts, paths[npath], T, 0.1))
    for T, npath in ((41, 65), (65, 129)):
        pts = long_end_points(T) + [p for p in long_points(paths[npath]) if p[2]]
        out.append(_launch(f"LONG T={T} dt=0.125 path={npath}", "LONG", pts, paths[npath], T, 0.125, TYPES_EXACT))
    for T in (31, 65):
        out.append(_launch(f"MANY T={T}", "MANY", many_points(), MANY_PATH, T, 0.1))
    _, rpath, rpts = random_block()
    for T in (31, 65):
        out.append(_launch(f"RANDOM T={T}", "RANDOM", [(t, r, True) for t, r, tt in rpts if tt == T], rpath, T, 0.1, designed=False))
    return out


_REF = {}


def reference(launch):
    """the reference's results of a launch (computed once per process)"""
    if launch.name not in _REF:
        t = launch.types
        _REF[launch.name] = R.predict(SCENES[launch.map](), launch.points, launch.n_points, launch.path, launch.T, launch.dt, VAR0, FACTOR,
                                      t["speed"], t["raw_l"], t["raw_w"], t["infl_l"], t["infl_w"])
    return _REF[launch.name]


# ------------------------------------------------------------------------------------------------ rasters, the cell sampler's cells
# origin, cell size, cells of the road raster handed to fo_scene_set_map.  The cell centres sit 3/8 m (LONG, in y: 7/16 m) off the
# routes' 1/8 m grid: no sample of a phantom spawned there comes within the last bits of a vertex or of a route's end.
RASTERS = {"LONG": (-128.125, -64.0625, 1.0, 470, 1000), "MANY": (-16.125, -16.125, 1.0, 100, 300), "RANDOM": (0.0, 0.0, 1.0, 4, 4)}
PATTERN = (CAR, BIKE, PED, CAR)                                     # agent j of the cell sampler is of type PATTERN[j % 4]


def lanelet_raster(name):
    """first lanelet (list order) holding the cell centre, -1 for none: [ny, nx] int32.  The maps' lanelets are rectangles"""
    x0, y0, cs, nx, ny = RASTERS[name]
    out = np.full((ny, nx), -1, dtype=np.int32)
    if name == "RANDOM":
        return out
    cx, cy = x0 + (np.arange(nx) + 0.5) * cs, y0 + (np.arange(ny) + 0.5) * cs
    for p, poly in reversed(list(enumerate(SCENES[name]().polys))):
        assert len(poly) == 4 and len(set(poly[:, 0])) == 2 and len(set(poly[:, 1])) == 2
        inx, iny = (cx > poly[:, 0].min()) & (cx < poly[:, 0].max()), (cy > poly[:, 1].min()) & (cy < poly[:, 1].max())
        out[np.ix_(iny, inx)] = p
    return out


def occluded_cells(name):
    """the hand-written class array of the cell sampler's test: window cells (ix, iy) marked occluded, four in a row at each place
    (so that each place gets vehicles and a pedestrian of the pattern)"""
    x0, y0, cs, nx, ny = RASTERS[name]
    y = lambda p: PITCH * p
    if name == "LONG":
        places = [(10.0, y(3) + 0.5), (288.0, y(7) + 0.5), (4.0, y(L_HAIR1) + 2.5), (98.0, y(L_HAIR3) + 3.5), (30.0, y(L_BEND) - 1.5),
                  (7.0, y(L_ONE) + 2.5), (7.0, y(L_NONE) + 2.5), (124.0, y(6) - 0.5), (30.0, PATH_Y + 2.5), (20.0, y(4) + 1.5)]
    else:
        places = [(4.0, 0.5), (12.0, 126.5), (4.0, 128.5), (20.0, 258.5), (39.0, 6.5), (43.0, 128.5), (39.0, 1.5), (39.0, 15.5)]   # (the overlaps get vehicles)
    cells = []
    for px, py in places:
        ix, iy = int(math.floor((px - x0) / cs)), int(math.floor((py - y0) / cs))
        cells += [(ix + k, iy) for k in range(4)]
    return sorted(set(cells), key=lambda c: (c[1], c[0]))


# ------------------------------------------------------------------------------------------------ the rule of comparison
TOL = {"pos": 1e-9, "yaw": 1e-12, "v": 1e-12}          # the project's own (tests/test_scene_gpu.py); cov: rtol 1e-13
COV_RTOL = 1e-13


def compare(launch, ref, got, who, slots, worst=None):
    """`got` (pos [S, T, 2], yaw, v [S, T], cov [S, T, 4], len [S]) against the reference on `slots`: settled and exact slots have
    the reference's length, values within TOL, exact zeros behind the length; an open slot may differ by one sample in length and
    its values are not compared.  -> the largest deviation per quantity (also folded into `worst`)"""
    total, worst = ({} if worst is None else worst), {}
    R_ = 3
    for s_ in slots:
        i, r = divmod(s_, R_)
        tag = (who, launch.name, launch.tags[i] if i < launch.n_points else "inactive", r)
        L = int(ref["len"][s_])
        if ref["status"][s_] == "open":
            assert abs(int(got["len"][s_]) - L) <= 1, tag
            continue
        assert int(got["len"][s_]) == L, (tag, int(got["len"][s_]), L)
        for k, tol in TOL.items():
            d = np.abs(got[k][s_, :L] - ref[k][s_, :L])
            dev = float(d.max()) if L else 0.0
            worst[k] = max(worst.get(k, 0.0), dev)
            assert dev <= tol, (tag, k, dev)
            assert np.all(got[k][s_, L:] == 0.0), (tag, k, "not zero behind len")
        if "cov" in got:
            c, c0 = got["cov"][s_].reshape(-1, 4), ref["cov"][s_]
            assert np.all(c[:, 1:3] == 0.0), tag
            rel = float(np.abs(c[:, (0, 3)] / c0[:, (0, 3)] - 1.0).max())
            worst["cov"] = max(worst.get("cov", 0.0), rel)
            assert rel <= COV_RTOL, (tag, "cov", rel)
    for k, v in worst.items():
        total[k] = max(total.get(k, 0.0), v)
    return worst
