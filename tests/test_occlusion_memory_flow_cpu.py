"""The vehicle layer of the occlusion memory (DESIGN.md §5.9 "Vehicle layer") without a GPU: the checker
(tests/ref_occlusion_memory_flow.py) on a one-way lane whose answer is written down by hand, its relation to the road and the
Euclidean memory (subset; equal to the road memory under a table of 0xFF), Dijkstra against a whole-grid relaxation, the halo n,
the tie to the lane-flow forecast of §5.10, and the library / Python layer."""
import math
import os

import numpy as np
import pytest

import ref_hidden_reach as HR
import ref_hidden_reach_flow as F
import ref_occlusion_memory as OM
import ref_occlusion_memory_flow as V
import ref_occlusion_memory_road as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from frenetix_occlusion import _native
    return _native


# ------------------------------------------------------------------------------------------------ 1. by hand
def one_way_lane(sources):
    """60 x 3 raster = window.  Row 1 is a lane that flows +x (E, NE, SE out of every cell); rows 0 and 2 are not road.  Columns
    10 .. 49 were seen empty and are occluded now (a 40-cell stretch), columns 50 .. 59 are road out of range, columns 0 .. 9
    too ("up") or visible ("down").  The previous vehicle set holds the ten cells `sources` ("down": columns 50 .. 59, "up":
    0 .. 9).  r2 = 17: h = 4, L = 53.
    -> (cls, win, road, moves, prev)"""
    nx, ny = 60, 3
    road = np.zeros((ny, nx), dtype=np.uint8)
    road[1] = 1
    moves = np.full((ny, nx), F.ANY, dtype=np.uint8)
    moves[1] = F.sector(0.0)
    cls = road.copy()
    cls[1, 10:50] = 5
    prev = np.zeros((ny, nx), dtype=np.uint8)
    if sources == "down":
        prev[1, 50:60] = 1
        cls[1, 0:10] = 3
    else:
        prev[1, 0:10] = 1
    return cls, (0, 0, nx, ny), road, moves, prev


def test_one_way_lane_by_hand():
    """sources downstream of the stretch: a vehicle there drives away from it, V = 0 on all 40 cells, while the road memory
    refills the last isqrt(17) = 4 columns (12 |dx| <= 53 and dx^2 <= 17: |dx| <= 4).  Sources upstream: the lane delivers
    them, and V is the road memory's answer, the first 4 columns"""
    assert F.sector(0.0) == 0b10000011
    cls, win, road, moves, prev = one_way_lane("down")
    Hr, _ = R.step(cls, win, road, 17, prev, win)
    Vv = V.step(cls, win, road, moves, 17, prev, win)
    assert [int(x) for x in np.flatnonzero(Hr[1, 10:50])] == [36, 37, 38, 39]
    assert not Vv[1, 10:50].any()
    assert np.array_equal(Vv[1, 50:], np.ones(10, dtype=np.uint8)) and not Vv[1, :10].any()    # out of range: the road bit / seen
    cls, win, road, moves, prev = one_way_lane("up")
    Hr, _ = R.step(cls, win, road, 17, prev, win)
    Vv = V.step(cls, win, road, moves, 17, prev, win)
    assert [int(x) for x in np.flatnonzero(Vv[1, 10:50])] == [0, 1, 2, 3]
    assert np.array_equal(Vv, Hr)
    d, L = V.flow_distance(win, road, moves, 17, prev, win)
    assert L == 53 and [int(v) for v in d[1, 9:15]] == [0, 12, 24, 36, 48, V.NONE]


# ------------------------------------------------------------------------------------------------ 2. random cases
def _cases(n=60, seed=20240611):
    """random raster and move table, two windows that may be shifted, disjoint or partly off the raster, r2 up to 1024"""
    rng = np.random.default_rng(seed)
    for case in range(n):
        rnx, rny = int(rng.integers(24, 48)), int(rng.integers(24, 48))
        road = (rng.random((rny, rnx)) < rng.uniform(0.3, 0.9)).astype(np.uint8)
        moves = rng.integers(0, 256, (rny, rnx)).astype(np.uint8)
        moves[rng.random((rny, rnx)) < rng.uniform(0.0, 0.6)] = F.ANY

        def window():
            nx, ny = int(rng.integers(8, 20)), int(rng.integers(8, 20))
            return (int(rng.integers(-6, rnx - nx + 7)), int(rng.integers(-6, rny - ny + 7)), nx, ny)
        W, W2 = window(), window()
        prev = (rng.random((W[3], W[2])) < rng.uniform(0.02, 0.5)).astype(np.uint8)
        cls2 = rng.choice(np.array([0, 1, 3, 4, 5], dtype=np.uint8), (W2[3], W2[2]), p=[0.15, 0.15, 0.2, 0.1, 0.4])
        r2 = int(rng.choice([0, 1, 2, 5, 17, 60, 200, 853, 1024])) if case % 2 else int(rng.integers(0, 1025))
        yield case, road, moves, W, prev, W2, cls2, r2


def test_vehicles_inside_road_inside_euclid():
    n_less = 0
    for case, road, moves, W, prev, W2, cls2, r2 in _cases():
        He, _ = OM.step(cls2, W2, road, r2, prev, W)
        Hr, _ = R.step(cls2, W2, road, r2, prev, W)
        Vv = V.step(cls2, W2, road, moves, r2, prev, W)
        assert (Vv <= Hr).all() and (Hr <= He).all(), case
        occ = ((cls2 & 4) != 0) & ((cls2 & 2) == 0)
        assert np.array_equal(Vv[~occ], Hr[~occ]), case
        n_less += int((Vv != Hr).sum())
        # a smaller previous set gives a smaller set (monotonicity: what carries the subset over a drive)
        less = prev & (np.arange(prev.size).reshape(prev.shape) % 3 != 0).astype(np.uint8)
        assert (V.step(cls2, W2, road, moves, r2, less, W) <= Vv).all(), case
    assert n_less > 0


def test_a_table_of_any_gives_the_road_memory():
    for case, road, moves, W, prev, W2, cls2, r2 in _cases(30):
        Hr, _ = R.step(cls2, W2, road, r2, prev, W)
        assert np.array_equal(V.step(cls2, W2, road, np.full_like(moves, F.ANY), r2, prev, W), Hr), case


def test_reset_is_h_of_a_reset_step():
    """on class bytes as the visibility stage makes them (an occluded cell is a road cell of the raster)"""
    for case, road, moves, W, prev, W2, cls2, r2 in _cases(10):
        rd = OM.previous_p(road, None, None, W2, 0)
        cls = np.where(rd != 0, cls2 | 1, cls2 & 2).astype(np.uint8)
        H0, out = OM.step(cls, W2, road, 0)
        assert np.array_equal(out, cls) and (cls & 4).any(), case
        assert np.array_equal(V.step(cls, W2, road, moves, r2), H0), case


def test_dijkstra_against_relaxation_to_a_fixed_point():
    for case, road, moves, W, prev, W2, cls2, r2 in _cases():
        n, L = R.halo(r2), R.reach_units(r2)
        PV, passable = R.grids(road, prev, W, W2, n)
        out = F.moves_over(moves, W2, n)
        a, b = F.dijkstra(PV, passable, out, L), F.relax_to_fixed_point(PV, passable, out, L)
        assert np.array_equal(a, b), case
        assert ((a == V.NONE) | (a <= L)).all() and (a[PV] == 0).all() and (a[~passable] == V.NONE).all()


# ------------------------------------------------------------------------------------------------ 3. the halo
def test_a_deciding_directed_path_leaves_the_h_halo():
    """r2 = 1024: h = 32, n = 34.  A one-cell window at (40, 40); its cell is road, seen empty, occluded now.  The only way in is a
    straight corridor 34 cells long that flows +x from a hidden cell at (6, 40): 34 * 12 = 408 <= 416.  A second hidden cell at
    (40, 10), joined to nothing, passes the disc test.  The path's first two cells lie outside the window grown by h; with the
    corridor flowing -x nothing arrives at all"""
    road = np.zeros((81, 81), dtype=np.uint8)
    road[40, 7:41] = 1
    moves = np.full((81, 81), F.ANY, dtype=np.uint8)
    moves[40, 7:41] = F.sector(0.0)
    prev_win = (0, 0, 81, 81)
    prev = np.zeros((81, 81), dtype=np.uint8)
    prev[40, 6] = 1
    prev[10, 40] = 1
    win = (40, 40, 1, 1)
    cls = np.array([[5]], dtype=np.uint8)
    assert R.step(cls, win, road, 1024, prev, prev_win)[0][0, 0] == 1
    assert V.step(cls, win, road, moves, 1024, prev, prev_win)[0, 0] == 1
    assert V.step(cls, win, road, moves, 1024, prev, prev_win, grow=32)[0, 0] == 0
    d, L = V.flow_distance(win, road, moves, 1024, prev, prev_win)
    assert int(d[0, 0]) == 408 and L == 416
    moves[40, 7:41] = F.sector(180.0)
    assert V.step(cls, win, road, moves, 1024, prev, prev_win)[0, 0] == 0


# ------------------------------------------------------------------------------------------------ 4. the forecast
def test_what_the_lane_flow_forecast_reaches_in_j_steps_is_what_the_vehicle_layer_keeps_j_steps_later():
    rng = np.random.default_rng(20240612)
    n_cells, n_kept, n_fewer = 0, 0, 0
    for case in range(60):
        rnx, rny = int(rng.integers(24, 48)), int(rng.integers(24, 48))
        road = (rng.random((rny, rnx)) < rng.uniform(0.4, 0.9)).astype(np.uint8)
        moves = rng.integers(0, 256, (rny, rnx)).astype(np.uint8)
        moves[rng.random((rny, rnx)) < rng.uniform(0.0, 0.6)] = F.ANY
        nx, ny = int(rng.integers(8, 20)), int(rng.integers(8, 20))
        W = (int(rng.integers(-6, rnx - nx + 7)), int(rng.integers(-6, rny - ny + 7)), nx, ny)
        rd = OM.previous_p(road, None, None, W, 0)          # the raster's road bit inside the window, 0 off the raster
        cls = np.where(rd != 0, rng.choice(np.array([1, 3, 5], dtype=np.uint8), (ny, nx), p=[0.2, 0.6, 0.2]), 0).astype(np.uint8)
        cls2 = np.where(rd != 0, rng.choice(np.array([1, 3, 5], dtype=np.uint8), (ny, nx), p=[0.2, 0.2, 0.6]),
                        rng.choice(np.array([0, 4], dtype=np.uint8), (ny, nx))).astype(np.uint8)
        cs, dt = 0.5, 0.1
        table = HR.reach_table(float(rng.uniform(0.0, 14.0)), dt, math.sqrt(2.0) * cs if case % 3 else 0.0, cs, 11)
        j = int(rng.integers(1, 11))
        S_W = HR.sources(cls, W, road)
        V2 = V.step(cls2, W, road, moves, int(table[j]), prev_v=S_W.astype(np.uint8), prev_win=W)
        H2, _ = R.step(cls2, W, road, int(table[j]), prev_h=S_W.astype(np.uint8), prev_win=W)
        A_flow, _, _, _ = F.arrival_map_flow(cls, W, road, moves, table)
        sel = ((cls2 & 4) != 0) & ((cls2 & 2) == 0)
        assert np.array_equal(V2[sel] != 0, A_flow[sel] <= j), case
        n_cells += int(sel.sum())
        n_kept += int((V2[sel] != 0).sum())
        n_fewer += int((V2[sel] != H2[sel]).sum())
    assert n_cells > 2000 and 0 < n_kept < n_cells and n_fewer > 0


# ------------------------------------------------------------------------------------------------ 5. a drive
def test_memory_follows_a_drive_inside_the_road_memory():
    """the host rules: one plan, V inside H at every step of a drive over random class bytes, the reasons shared"""
    rng = np.random.default_rng(5)
    road = (rng.random((40, 60)) < 0.7).astype(np.uint8)
    moves = rng.integers(0, 256, (40, 60)).astype(np.uint8)
    mv, mh = V.Memory(13.9, 0.1, 0.5), R.Memory(13.9, 0.1, 0.5)
    n_less = 0
    for step, t in enumerate([0, 1, 2, 3, 3, 4, 14, 15, 100, 101]):
        win = (3 + 2 * step, 5, 24, 20)
        rd = OM.previous_p(road, None, None, win, 0)
        cls = np.where(rd != 0, rng.choice(np.array([1, 3, 5], dtype=np.uint8), (20, 24), p=[0.1, 0.4, 0.5]), 0).astype(np.uint8)
        Vv, reason = mv.advance(cls, win, road, moves, t)
        H, _, reason_h = mh.advance(cls, win, road, t)
        assert reason == reason_h == {0: "first", 4: "time", 8: "reach"}.get(step), step
        assert (Vv <= H).all(), step
        if reason is not None:
            assert np.array_equal(Vv, H), step
        n_less += int((Vv != H).sum())
    assert n_less > 0


# ------------------------------------------------------------------------------------------------ 6. library, Python layer
def test_symbol_and_abi(native):
    lib = native.load()
    name = "fo_scene_set_occlusion_memory_vehicles"
    assert name in native.EXPORTS and hasattr(lib, name)
    assert lib.fo_abi_version() == 12
    assert lib.fo_scene_set_occlusion_memory_vehicles(None, None) == native.FO_E_ARG       # no context: refused, not a crash


def test_vehicles_in_the_python_layer(native):
    import yaml
    from frenetix_occlusion.hidden_traffic import HiddenClearance, HiddenReach
    from frenetix_occlusion.interface import occlusion_memory_vehicles
    from frenetix_occlusion.occlusion_memory import OCCLUSION_MEMORY_VEHICLES
    from frenetix_occlusion.sensor_model import SensorModel
    assert OCCLUSION_MEMORY_VEHICLES == ("off", "lanes")
    assert occlusion_memory_vehicles(None) == "off" and occlusion_memory_vehicles({}) == "off"
    assert occlusion_memory_vehicles({"occlusion_memory_vehicles": "lanes"}) == "lanes"
    assert occlusion_memory_vehicles({"occlusion_memory_vehicles": "off"}) == "off"
    assert occlusion_memory_vehicles({"occlusion_memory_vehicles": False}) == "off"         # (YAML's reading of a bare `off`)
    for bad in ("road", "Lanes", "", 3, 0, True):
        with pytest.raises(ValueError):
            occlusion_memory_vehicles({"occlusion_memory_vehicles": bad})
    sm = SensorModel.__new__(SensorModel)          # (no device: the arguments are refused before anything else is looked at)
    with pytest.raises(ValueError, match="vehicles"):
        sm.enable_occlusion_memory(vehicles="x")
    with pytest.raises(ValueError, match="vehicles"):
        sm.enable_occlusion_memory(False, vehicles="x")
    sm.lane_moves = None                            # a model built from bare geometry: no move table
    with pytest.raises(ValueError, match="move table"):
        sm.enable_occlusion_memory(metric="road", vehicles="lanes")
    with open(os.path.join(ROOT, "frenetix-occlusion_amd", "frenetix_occlusion", "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert "occlusion_memory_vehicles" in cfg["accelerator"]
    assert occlusion_memory_vehicles(cfg["accelerator"]) == "off"
    assert HiddenReach.__dataclass_fields__["from_vehicle_memory"].default is False
    assert HiddenClearance.__dataclass_fields__["from_vehicle_memory"].default is False
