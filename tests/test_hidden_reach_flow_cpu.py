"""Lane flow of the hidden-traffic reach forecast (DESIGN.md §5.10 "Lane flow") without a GPU: the checker
(tests/ref_hidden_reach_flow.py) against cases worked out by hand, its invariants on random maps with random move tables
(Dijkstra against plain relaxation, flow never earlier than road, a table of 0xFF equal to road), the host builder of the move
table, the exported symbols and the refusals of the Python layer before any device work."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_reach_flow as RF
import ref_hidden_reach_road as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NE, N, NW, W, SW, S, SE = (1 << k for k in range(8))
EAST, NORTH, WEST, SOUTH = RF.sector(0), RF.sector(90), RF.sector(180), RF.sector(270)
FAR = [2, 8, 18, 4000]          # L[-1] = 822: holds every distance of the small maps below


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from frenetix_occlusion import _native
    return _native


def test_sectors():
    assert (EAST, NORTH, WEST, SOUTH) == (E | NE | SE, N | NE | NW, W | NW | SW, S | SW | SE)
    assert RF.sector(45) == E | NE | N and RF.sector(-45) == RF.sector(315) == E | SE | S
    assert RF.DIRS[2] == (0, 1) and RF.COST == [12, 17] * 4


# ------------------------------------------------------------------------------------------------ 1. by hand
def _strip(nx, ny, src):
    """window = whole raster, all road, all visible but the occluded cells `src`"""
    road = np.ones((ny, nx), dtype=np.uint8)
    cls = np.full((ny, nx), 3, dtype=np.uint8)
    for x, y in src:
        cls[y, x] = 5
    return cls, (0, 0, nx, ny), road


def test_one_eastbound_lane():
    cls, win, road = _strip(13, 3, [(6, 1)])
    moves = np.full((3, 13), EAST, dtype=np.uint8)
    d, _ = RF.flow_distance(cls, win, road, moves, FAR)
    d_road, _ = RR.road_distance(cls, win, road, FAR)
    for x in range(13):
        assert d[1, x] == (12 * (x - 6) if x >= 6 else RF.NONE)
        assert d_road[1, x] == 12 * abs(x - 6)                 # the undirected metric comes back down the lane
    assert d[0, 6] == RF.NONE and d[2, 6] == RF.NONE and d_road[0, 6] == 12       # no step across the lane
    assert d[0, 7] == 17 and d[2, 8] == 29                     # but forward and sideways
    A, A_e, _, _ = RF.arrival_map_flow(cls, win, road, moves, FAR)
    assert (A[:, :6] == 255).all() and (A_e[:, :6] != 255).all()


def test_two_opposite_lanes_do_not_feed_each_other():
    moves = np.zeros((4, 13), dtype=np.uint8)
    moves[:2], moves[2:] = EAST, WEST                          # two cells wide each, driving on the right
    for src, own, other in (((6, 1), slice(0, 2), slice(2, 4)), ((6, 2), slice(2, 4), slice(0, 2))):
        cls, win, road = _strip(13, 4, [src])
        d, _ = RF.flow_distance(cls, win, road, moves, FAR)
        assert (d[other] == RF.NONE).all()
        assert (d[own] != RF.NONE).sum() > 6
        assert (RR.road_distance(cls, win, road, FAR)[0] != RF.NONE).all()


def test_two_eastbound_lanes_lane_change_costs_a_diagonal():
    cls, win, road = _strip(9, 2, [(2, 0)])
    moves = np.full((2, 9), EAST, dtype=np.uint8)
    d, _ = RF.flow_distance(cls, win, road, moves, FAR)
    assert d[1, 3] == 17 and d[1, 4] == 29 and d[0, 4] == 24
    assert d[1, 2] == RF.NONE and d[1, 1] == RF.NONE and d[0, 1] == RF.NONE


def test_crossing_with_the_union_mask():
    """an eastbound arm (row c, from the west) meets a street of two lanes: column c - 1 southbound, column c northbound.  The two
    crossing cells carry the union of the arm's set and their lane's"""
    c, n = 5, 11
    road = np.zeros((n, n), dtype=np.uint8)
    moves = np.full((n, n), 0xFF, dtype=np.uint8)
    road[c, :c + 1] = 1
    road[:, c - 1:c + 1] = 1
    moves[c, :c - 1] = EAST
    moves[:, c - 1], moves[:, c] = SOUTH, NORTH
    moves[c, c - 1], moves[c, c] = SOUTH | EAST, NORTH | EAST
    cls = np.where(road != 0, 3, 2).astype(np.uint8)
    cls[c, 0] = 5
    win = (0, 0, n, n)
    d, _ = RF.flow_distance(cls, win, road, moves, FAR)
    assert d[c, c - 1] == 12 * (c - 1) and d[c, c] == 12 * c
    assert d[c + 1, c] == 12 * (c - 1) + 17                    # the left turn into the northbound lane, cutting the corner
    assert d[n - 1, c] == 12 * (c - 1) + 17 + 12 * (n - 2 - c)
    assert d[c - 1, c - 1] == 12 * (c - 2) + 17                # the right turn into the southbound lane, cutting the corner too
    assert d[0, c - 1] == 12 * (c - 2) + 17 + 12 * (c - 1)
    assert (d[c + 1:, c - 1] == RF.NONE).all()                 # not into the southbound lane's wrong side, north of the crossing
    assert (d[:c, c] == RF.NONE).all()                         # nor down the northbound lane
    d_road, _ = RR.road_distance(cls, win, road, FAR)
    assert (d_road[road != 0] != RF.NONE).all()


def test_a_free_cell_passes_traffic_both_ways():
    cls, win, road = _strip(11, 1, [(5, 0)])
    moves = np.full((1, 11), 0xFF, dtype=np.uint8)
    d, _ = RF.flow_distance(cls, win, road, moves, FAR)
    assert d[0].tolist() == [12 * abs(x - 5) for x in range(11)]
    moves[0, :3], moves[0, 8:] = WEST, WEST                    # a westbound lane on both sides of the free stretch
    d, _ = RF.flow_distance(cls, win, road, moves, FAR)
    assert d[0, :8].tolist() == [12 * abs(x - 5) for x in range(8)]       # out of the free cells into the lane, with it
    assert (d[0, 8:] == RF.NONE).all()                         # not against it: both ends decide
    moves[0, 5] = EAST                                         # the source itself bound to the east: nothing goes west
    d, _ = RF.flow_distance(cls, win, road, moves, FAR)
    assert (d[0, :5] == RF.NONE).all() and d[0, 6] == 12 and d[0, 7] == 24


def test_moves_outside_the_raster_are_free():
    moves = np.arange(12, dtype=np.uint8).reshape(3, 4)
    out = RF.moves_over(moves, (-1, 1, 4, 3))
    assert out.shape == (5, 6)
    assert (out[:, 0] == 0xFF).all() and (out[4] == 0xFF).all()          # x = -2 (and -1: column 1), y = 3
    assert (out[:, 1] == 0xFF).all() and out[0, 2:].tolist() == [0, 1, 2, 3] and out[3, 2:].tolist() == [0xFF] * 4


# ------------------------------------------------------------------------------------------------ 2. invariants
def _random_moves(rng, rny, rnx):
    kind = rng.random((rny, rnx))
    sect = np.array([RF.sector(45 * k) for k in range(8)], dtype=np.uint8)[rng.integers(0, 8, (rny, rnx))]
    anyb = rng.integers(0, 256, (rny, rnx)).astype(np.uint8)
    return np.where(kind < 0.5, sect, np.where(kind < 0.75, 0xFF, anyb)).astype(np.uint8)


def test_invariants_on_random_maps():
    rng = np.random.default_rng(20240131)
    later, cut, later_cells = 0, 0, 0
    for case in range(60):
        rnx, rny = int(rng.integers(16, 40)), int(rng.integers(16, 40))
        road = (rng.random((rny, rnx)) < rng.uniform(0.3, 0.9)).astype(np.uint8)
        nx, ny = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        win = (int(rng.integers(-nx + 1, rnx)), int(rng.integers(-ny + 1, rny)), nx, ny)      # hangs over the raster's edge
        cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx), p=[0.15, 0.1, 0.55, 0.05, 0.05, 0.1])
        hidden = (rng.random((ny, nx)) < 0.03).astype(np.uint8) if case % 2 else None
        J = int(rng.integers(1, 12))
        r2 = np.sort(rng.integers(0, int(rng.integers(1, 900)), J))
        moves = _random_moves(rng, rny, rnx)
        A, A_e, d, L = RF.arrival_map_flow(cls, win, road, moves, r2, hidden)
        A_road, _, d_road, _ = RR.arrival_map_road(cls, win, road, r2, hidden)
        S_, P = RR.passable(cls, win, road, hidden)
        out = RF.moves_over(moves, win)
        assert np.array_equal(RF.dijkstra(S_, P, out, int(L[-1])), RF.relax_to_fixed_point(S_, P, out, int(L[-1]))), case
        assert (d >= d_road).all() and np.array_equal(d == 0, d_road == 0)       # 65535 = none is the largest
        assert (A >= A_road).all() and (A_road >= A_e).all()
        assert ((d == RF.NONE) | (d <= L[-1])).all()
        free = np.full((rny, rnx), 0xFF, dtype=np.uint8)
        assert np.array_equal(RF.flow_distance(cls, win, road, free, r2, hidden)[0], d_road)
        assert np.array_equal(RF.arrival_map_flow(cls, win, road, free, r2, hidden)[0], A_road)
        later += int(((d > d_road) & (d != RF.NONE)).sum())
        cut += int(((d == RF.NONE) & (d_road != RF.NONE)).sum())
        later_cells += int((A > A_road).sum())
    assert later > 0 and cut > 0 and later_cells > 0               # the lanes do bite on these maps


# ------------------------------------------------------------------------------------------------ 3. the host table builder
def _lane(lid, yaw_deg, length=30.0, width=4.0, origin=(0.0, 0.0), n=16):
    """a straight lanelet from `origin` along `yaw_deg`"""
    from frenetix_occlusion import scenario as SC
    t = np.linspace(0.0, length, n)
    c, s = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    mid = np.stack((origin[0] + t * c, origin[1] + t * s), -1)
    nrm = 0.5 * width * np.array([-s, c])
    return SC.Lanelet(lid, mid + nrm, mid - nrm)


def _raster(lanes):
    from frenetix_occlusion import scenario as SC
    return SC.lane_move_raster(lanes, -40.0, -40.0, 0.5, 160, 160), SC.lane_yaw_raster(lanes, -40.0, -40.0, 0.5, 160, 160)


@pytest.mark.parametrize("yaw,bits", [(0, E | NE | SE), (90, N | NE | NW), (180, W | NW | SW), (40, E | NE | N)])
def test_lane_move_raster_of_a_straight_lane(yaw, bits):
    moves, lane_yaw = _raster([_lane(1, yaw)])
    assert moves.shape == (160, 160) and moves.dtype == np.uint8
    on = ~np.isnan(lane_yaw)
    assert on.sum() > 300                                           # 30 m x 4 m at 0.5 m
    assert (moves[on] == bits).all() and (moves[~on] == 0xFF).all()
    assert bits == sum(1 << k for k in range(8) if math.cos(math.radians(45 * k - yaw)) >= math.cos(math.radians(67.5)))


def test_lane_move_raster_takes_the_union_of_overlapping_lanelets():
    from frenetix_occlusion import scenario as SC
    a, b = _lane(1, 0, origin=(-15.0, 0.0)), _lane(2, 90, origin=(0.0, -15.0))      # they cross at the origin
    moves, lane_yaw = _raster([a, b])
    only_a = SC.lane_move_raster([a], -40.0, -40.0, 0.5, 160, 160)
    only_b = SC.lane_move_raster([b], -40.0, -40.0, 0.5, 160, 160)
    both = (only_a != 0xFF) & (only_b != 0xFF)
    assert both.sum() == 64                                         # the 4 m x 4 m crossing
    assert (moves[both] == (EAST | NORTH)).all() and (lane_yaw[both] == 0.0).all()          # (the heading raster keeps the first)
    assert np.array_equal(moves[~both], np.minimum(only_a, only_b)[~both])                  # elsewhere the one lanelet's, or 0xFF
    narrow = SC.lane_move_raster([a], -40.0, -40.0, 0.5, 160, 160, cone_deg=22.0)
    assert (narrow[only_a != 0xFF] == E).all()


# ------------------------------------------------------------------------------------------------ 4. symbols, Python
def test_symbols(native):
    lib = native.load()
    for name in ("fo_scene_set_lane_moves", "fo_scene_hidden_reach_flow", "fo_scene_hidden_clearance_flow"):
        assert name in native.EXPORTS and hasattr(lib, name)
    assert lib.fo_abi_version() == 12
    # no context: refused, not a crash
    assert lib.fo_scene_set_lane_moves(None, None) == native.FO_E_STATE
    assert lib.fo_scene_hidden_reach_flow(None, None, None) == native.FO_E_STATE
    assert lib.fo_scene_hidden_clearance_flow(None, None, None) == native.FO_E_STATE


def test_refusals_before_any_device_work(native):
    from frenetix_occlusion.sensor_model import HIDDEN_REACH_FLOWS, HiddenClearance, HiddenReach, SensorModel
    assert HIDDEN_REACH_FLOWS == ("any", "lanes")
    assert list(HiddenReach.__dataclass_fields__)[-1] == "flow" and list(HiddenClearance.__dataclass_fields__)[-1] == "flow"
    z = np.zeros((2, 31))
    veh = (4.508, 1.610, 1.4227)
    calls = ((SensorModel.hidden_reach, dict(v_max=13.9)), (SensorModel.hidden_clearance, dict(v_cap=13.9)))
    for fn, kw in calls:
        kw = dict(kw, vehicle=veh, dt=0.1)
        for sm in (SimpleNamespace(window=None), SimpleNamespace()):          # (not even the window is looked at)
            with pytest.raises(ValueError, match="flow 'left'"):
                fn(sm, z, z, z, metric="road", flow="left", **kw)
            with pytest.raises(ValueError, match="metric 'road'"):
                fn(sm, z, z, z, metric="euclid", flow="lanes", **kw)
            with pytest.raises(ValueError, match="metric 'manhattan'"):        # the metric is looked at first
                fn(sm, z, z, z, metric="manhattan", flow="left", **kw)
        with pytest.raises(RuntimeError, match="previous launch"):            # known values go on to the usual checks
            fn(SimpleNamespace(window=None), z, z, z, metric="road", flow="lanes", **kw)
        # a model without a move table: refused after the checks of the arguments, before the device is looked at
        bare = SimpleNamespace(window=object(), cell_size=0.5, lane_moves=None)
        with pytest.raises(ValueError, match="lengths"):
            fn(bare, z, z, z, metric="road", flow="lanes", lengths=np.zeros(3), **kw)
        with pytest.raises(RuntimeError, match="move table"):
            fn(bare, z, z, z, metric="road", flow="lanes", **kw)
