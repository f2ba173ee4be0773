"""Scenes that put the scene stage (csrc/fo_scene.hip) on each of its switch points, and the host rules that pick the
kernel form, restated.  Shared by tests/test_scene_forms_cpu.py (the oracle alone: is every scene what it is meant to be)
and tests/test_scene_forms_gpu.py (device == oracle in every form).  Nothing here touches a GPU.

The switches (ray_waves and compact_two_launches in csrc/fo_scene_plan.hpp, taken by scene_visibility in fo_scene.hip through
launch_rays / launch_settle / compact of fo_scene_rays.hpp / fo_scene_grid.hpp / fo_scene_compact.hpp):
  NW    fo_rays_kernel / fo_settle_kernel<SKIP, NW>: one wave per workgroup iff the map has at most 64 chunks of 64 boundary
        pieces (E <= 4096) and at most 16 obstacles and FO_SCENE_FIVE_WAVES is unset; five waves otherwise
  SKIP  a hole-skip table was passed (a hole ring of the road union enclosed by the sensor footprint)
  two-launch compaction  more than 2048 blocks of 256 window cells (a window edge of 725 cells: sensor radius > 120.5 m at
        the 0.5 m cell)
"""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np

from frenetix_occlusion import scenario as S

SCENE_FORMS = [("library", {}), ("five_waves", {"FO_SCENE_FIVE_WAVES": "1"})]
CHUNK = 64                 # boundary pieces per chunk box
ONE_WAVE_CHUNKS = 64       # a single wave culls 64 chunk boxes in one round trip
ONE_WAVE_OBSTACLES = 16    # 4 sides each: 64 lanes
COMPACT_BLOCK = 256
ONE_LAUNCH_BLOCKS = 2048


def n_chunks(E):
    return (E + CHUNK - 1) // CHUNK


def n_blocks(cells):
    return (cells + COMPACT_BLOCK - 1) // COMPACT_BLOCK


def expected_form(E, O, skip, cells, forced):
    """(NW, SKIP, two_launch) of a scene-stage call: E boundary pieces, O obstacles, skip = a hole-skip table is passed,
    cells = window cells, forced = FO_SCENE_FIVE_WAVES is set"""
    one_wave = n_chunks(E) <= ONE_WAVE_CHUNKS and 4 * O <= 64 and not forced
    return (1 if one_wave else 5, bool(skip), n_blocks(cells) > ONE_LAUNCH_BLOCKS)


def window_edge(radius, cell_size=0.5):
    """SensorModel._window_for: cells per side of the window about the 1.5 r disc"""
    return int(math.ceil(2.0 * 1.5 * radius / cell_size)) + 1


# ------------------------------------------------------------------------------------------------ maps
def _rect(lid, x0, x1, y0, y1, n):
    xs = np.linspace(x0, x1, n)
    return S.Lanelet(lid, np.stack((xs, np.full(n, y1)), -1), np.stack((xs, np.full(n, y0)), -1))


@functools.lru_cache(maxsize=None)
def l_road(n_main, arm_x1=16.0, n_arm=21):
    """The L-shaped road of tests/test_scene_kat.py with the arm pointing down (-y): a main road x in [-30, 30], |y| <= 3, whose
    bounds are cut into n_main - 1 pieces each, and a side arm x in [10, arm_x1], y in [-43, -3], hidden from the main road
    behind the corner (10, -3).  The Z-order of the pieces has y as its high bits, so the main road's upper bound holds the
    highest indices, ascending in x: the last chunk is the far end of that wall.  Returns the MapGeometry (the union drops
    the pieces the two lanelets share, so E is whatever len(edges) says)."""
    main = _rect(1, -30.0, 30.0, -3.0, 3.0, n_main)
    ys = np.linspace(-3.0, -43.0, n_arm)
    arm = S.Lanelet(2, np.stack((np.full(n_arm, arm_x1), ys), -1), np.stack((np.full(n_arm, 10.0), ys), -1))
    return S.MapGeometry.from_lanelets([main, arm])


# piece counts on the one-wave rule's boundary: name -> (n_main, E, chunks, ego pose).  Each pose has a ray that ends on the
# last chunk (the far end of the upper wall), asserted on the oracle's hit ids.
L_ROADS = {
    "64 full chunks": (2134, 4096, 64, (-15.0, 0.0, 0.007)),
    "64 chunks, last partial": (2126, 4081, 64, (-5.0, 0.3, 0.0)),
    "65 chunks": (2141, 4110, 65, (-5.0, 0.0, math.atan2(3.0, 34.9))),
    # 601 chunks: waves 0..4 hold chunks [64 w, 64 w + 64) and, on their second trip, [320 + 64 w, ...) -- all of them non-empty
    "601 chunks": (20200, 38422, 601, (-5.0, 0.0, math.atan2(3.0, 34.96))),
}


@functools.lru_cache(maxsize=None)
def frame_lanelets():
    """A square road x, y in [-30, 30] around a block |x|, |y| <= 4 (four lanelets, bounds cut every 2 m): the union's boundary is
    an exterior ring and one hole ring, the nested squares of tests/test_scene_pointwise.py as a road.  A footprint that
    encloses the block makes it transparent (hole-skip table); a smaller one leaves it an occluder."""
    def strip(lid, x0, x1, y0, y1):
        return _rect(lid, x0, x1, y0, y1, int(round((x1 - x0) / 2.0)) + 1)
    return (strip(1, -30.0, 30.0, -30.0, -4.0), strip(2, -30.0, 30.0, 4.0, 30.0), strip(3, -30.0, -4.0, -4.0, 4.0),
            strip(4, 4.0, 30.0, -4.0, 4.0))


@functools.lru_cache(maxsize=None)
def frame_map():
    """the MapGeometry of frame_lanelets()"""
    return S.MapGeometry.from_lanelets(list(frame_lanelets()))


def _ob(i, typ, x, y, l, w, yaw=0.0, role="static", t0=0):
    return S.Obstacle(i, role, typ, l, w, t0, np.array([x, y, yaw, 0.0]), np.zeros((0, 4)))


FRAME_EGO = np.array([-14.0, -12.0, 0.3, 5.0])
FRAME_RAYS = 97            # 3.7 degrees between rays: a small obstacle slips between two of them and is seen by its probes only


def frame_obstacles(O):
    """O obstacles in the frame road, ego at FRAME_EGO.  Cell centres sit at k / 2 + 1 / 4: obstacles 1 and 2 overlap each other
    and show the ego one common front at y = -6.747, 3 mm above the cell centres y = -6.75 -- those centres lie in both 5 mm
    skins.  3 is a bicycle (casts no shadow), 4 is absent at time step 0 (a dynamic obstacle that starts later), 5 a wall
    that hides 6, 7 a long vehicle 0.3 m off the ego's right side: seen from so close its 100 m shadow polygon ends inside
    the sensor range (the shadow length matters).  The rest alternate between cars and pedestrian-sized boxes the 97-ray
    fan can miss."""
    c, s = math.cos(FRAME_EGO[2]), math.sin(FRAME_EGO[2])
    side = FRAME_EGO[:2] + 1.3 * np.array([s, -c])
    obs = [_ob(1, "car", -9.0, -5.747, 4.0, 2.0), _ob(2, "car", -6.5, -5.747, 4.0, 2.0),
           _ob(3, "bicycle", -10.0, -10.5, 2.0, 0.9, 0.4), _ob(4, "car", -5.0, -14.0, 4.5, 1.8, 0.0, "dynamic", 5),
           _ob(5, "truck", 2.0, -10.0, 2.5, 9.0, 0.2), _ob(6, "car", 9.0, -9.0, 4.5, 1.8, 1.0),
           _ob(7, "truck", side[0], side[1], 6.0, 2.0, FRAME_EGO[2])]
    rng = np.random.default_rng(1617)
    k = 8
    while len(obs) < O:
        ang, rad = rng.uniform(0.0, 2.6), rng.uniform(6.0, 40.0)
        x, y = FRAME_EGO[0] + rad * math.cos(ang), FRAME_EGO[1] + rad * math.sin(ang)
        if max(abs(x), abs(y)) > 28.0 or max(abs(x), abs(y)) < 6.0:
            continue
        if k % 2:
            obs.append(_ob(k, "pedestrian", x, y, 0.4, 0.4, rng.uniform(0, 3)))
        else:
            obs.append(_ob(k, "car", x, y, 4.5, 1.8, rng.uniform(0, 3)))
        k += 1
    return obs[:O]


# radius -> does the footprint enclose the block (hole-skip table passed)
FRAME_RADII = {50.0: True, 18.0: False}
# the frame in the first two-launch window (725 cells per side, see LARGE_WINDOWS): a hole-skip table and the scan + scatter
# compaction in one call
FRAME_LARGE_RADIUS = 120.6


def second_trip_waves(hit_id, E):
    """the waves of a five-wave workgroup whose SECOND trip through the chunk loop (cb += 5 * 64) holds a piece some ray ends
    on: piece -> chunk of 64 pieces -> wave trip of 64 chunks; trips 0..4 are the waves' first, 5..9 their second"""
    pieces = hit_id[(hit_id >= 0) & (hit_id < E)]        # (ids from E on are obstacles)
    chunk = pieces // CHUNK
    trip = chunk // ONE_WAVE_CHUNKS
    return {int(t) - 5 for t in trip if t >= 5}


def in_skin(corn, px, py, grow=0.005):
    """cell centres (px, py) within `grow` of the rectangle corn [4,2] (the 5 mm skin of sensor_model.py:183)"""
    sg = 1.0 if S._signed_area(corn) >= 0 else -1.0
    inside = np.ones(np.shape(px), dtype=bool)
    for k in range(4):
        a, b = corn[k], corn[(k + 1) % 4]
        e = b - a
        inside &= ~(-(sg * (e[0] * (py - a[1]) - e[1] * (px - a[0]))) > grow * math.hypot(*e))
    return inside


# ------------------------------------------------------------------------------------------------ large windows
# sensor radius -> window edge n (cells) and 256-cell blocks nb: the top of the one-launch compaction, the first two-launch
# window, and a clearly larger one (four 1024-entry rounds of the scan kernel)
LARGE_WINDOWS = {120.5: (724, 2048), 120.6: (725, 2054), 150.0: (901, 3172)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def avenue():
    """A straight two-lane road x in [-4, 4], y in [-100, 100] with parked cars 25 m and 40 m ahead of an ego at (2, 0) that
    looks along +y (cells behind the ego are never classed occluded).  In the 901-cell window of a 150 m sensor the scan
    kernel's third round begins at block 2048, row 582, 66 m ahead of the ego: the cars' shadows run along the road to its
    end, across that row.  (Scenario 2 is about 100 m tall: at 150 m all its occluded cells fall into one round, and a lost
    carry would not show.)"""
    ys = np.linspace(-100.0, 100.0, 21)
    col = lambda x: np.stack((np.full(len(ys), x), ys), -1)
    up = S.Lanelet(1, col(0.0), col(4.0))                        # heading +y: left bound x = 0
    down = S.Lanelet(2, col(0.0)[::-1].copy(), col(-4.0)[::-1].copy())
    cars = [_ob(1, "car", 2.0, 25.0, 4.5, 1.8, math.pi / 2), _ob(2, "car", -2.0, 40.0, 4.5, 1.8, -math.pi / 2)]
    return SimpleNamespace(lanelets=[up, down], obstacles=cars, ego_initial=np.array([2.0, 0.0, math.pi / 2, 5.0]))


@functools.lru_cache(maxsize=None)
def large_window_scene(radius):
    """the scene of a LARGE_WINDOWS radius: scenario 2 on either side of the switch, the avenue at 150 m"""
    return avenue() if radius >= 150.0 else S.load_geometry_npz(os.path.join(GOLDEN, "scenario2_geometry.npz"))


def scan_rounds(occluded, min_cells=100):
    """the 1024-block rounds of fo_flag_scan_kernel that hold more than min_cells of the occluded cell indices: with two or
    more of them the carry from one round into the next decides where the later round's indices land"""
    rounds, counts = np.unique(np.asarray(occluded) // (COMPACT_BLOCK * 1024), return_counts=True)
    return {int(r) for r, c in zip(rounds, counts) if c > min_cells}


def scene(geo_or_lanelets, obstacles=()):
    """what tests/test_scene_gpu.py::_check_step reads of a scenario"""
    return SimpleNamespace(lanelets=geo_or_lanelets, obstacles=list(obstacles))


# ------------------------------------------------------------------------------------------------ the oracle alone
def raster_frame(geo, cs=0.5):
    """SensorModel._set_map: origin and size of the road raster"""
    margin, xy = 2.0 * cs, geo.poly_xy
    x0 = math.floor((xy[:, 0].min() - margin) / cs) * cs
    y0 = math.floor((xy[:, 1].min() - margin) / cs) * cs
    nx = int(math.ceil((xy[:, 0].max() + margin - x0) / cs))
    ny = int(math.ceil((xy[:, 1].max() + margin - y0) / cs))
    return x0, y0, nx, ny


def oracle_step(oracle, geo, obstacles, ego, timestep=0, n_rays=720, radius=50.0, sensor_angle=360.0, shadow_length=100.0,
                cs=0.5, fan=None):
    """One step of the scene stage by the CPU oracle alone, with the host logic of SensorModel restated (raster frame, window,
    fan, hole-skip table).  fan = (dirs, rmax, half) as the device wrote them replaces the host statement of the fan (equal to
    4e-15; the same bits are what makes everything downstream comparable exactly).  Returns the facts the form tests assert."""
    from frenetix_occlusion.sensor_model import HoleIndex, footprint_ranges, half_fan_dirs, ray_dirs
    ego = np.asarray(ego, dtype=np.float64)
    yaw = float(ego[2])
    x0, y0, rnx, rny = raster_frame(geo, cs)
    raster = oracle.road_raster(geo.poly_off, geo.poly_xy, x0, y0, cs, rnx, rny)
    reach = 1.5 * radius
    ix0, iy0 = int(math.floor((ego[0] - reach - x0) / cs)), int(math.floor((ego[1] - reach - y0) / cs))
    n = window_edge(radius, cs)
    corn, cen, flags, _ = S.Scenario(0.1, [], list(obstacles)).obstacle_arrays(timestep)
    dirs, rmax, half = fan if fan is not None else (ray_dirs(n_rays, yaw, sensor_angle),
                                                    footprint_ranges(n_rays, yaw, sensor_angle, radius), half_fan_dirs(yaw))
    hi = HoleIndex(geo)
    rings = hi.enclosed(ego[:2], yaw, sensor_angle, radius)
    skip = hi.edge_skip(rings) if rings else None
    rng, hid, _ = oracle.raycast(geo.edges, corn, flags, ego[:2], dirs, radius, rmax=rmax, edge_skip=skip)
    full = sensor_angle >= 359.9
    hd = np.array([math.cos(yaw), math.sin(yaw)])
    ex = dict(hit_id=hid, edges=geo.edges, ocorn=corn, oflags=flags, rmax=rmax, edge_skip=skip, half_dirs=half,
              edge_line=geo.edge_line, shadow_length=shadow_length)
    cls, occ, n_exact = oracle.grid(raster, x0, y0, cs, ix0, iy0, n, n, ego[:2], hd, radius, full, dirs, rng, exact=ex,
                                    return_n_exact=True)
    vis = None
    if len(flags):
        vis = oracle.obstacle_visibility(geo.edges, corn, cen, flags, ego[:2], radius, full, dirs, edge_skip=skip, hit_id=hid)
    E, O = len(geo.edges), len(flags)
    return dict(E=E, chunks=n_chunks(E), O=O, n=n, nb=n_blocks(n * n), skipped=0 if skip is None else int(skip.sum()),
                n_occ=len(occ), n_exact=int(n_exact), hid=hid, vis=vis, cls=cls, occ=occ, corn=corn, flags=flags,
                frame=(x0, y0, ix0, iy0), vis_cells=int(((cls & 2) != 0).sum()))
