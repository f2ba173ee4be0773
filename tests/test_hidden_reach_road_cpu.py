"""Road metric of the hidden-traffic reach forecast (DESIGN.md §5.10 "Road metric") without a GPU: the checker
(tests/ref_hidden_reach_road.py) against cases worked out by hand, its invariants on random maps (Dijkstra against plain
relaxation, road never earlier than Euclid, open road equal to Euclid), the exported symbol and structure, and the refusal of
an unknown metric before any device work."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_reach as HR
import ref_hidden_reach_road as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from frenetix_occlusion import _native
    return _native


# ------------------------------------------------------------------------------------------------ 1. by hand
def _single_source(n=12, src=(5, 5)):
    """window = whole raster, all road, all visible but one occluded cell"""
    road = np.ones((n, n), dtype=np.uint8)
    cls = np.full((n, n), 3, dtype=np.uint8)
    cls[src[1], src[0]] = 5
    return cls, (0, 0, n, n), road


FAR = [2, 8, 18, 400]          # L = 18, 36, 55, 260: the last entry holds every distance of a 12 x 12 window


def test_free_road():
    cls, win, road = _single_source()
    d, L = RR.road_distance(cls, win, road, FAR)
    assert L.tolist() == [18, 36, 55, 260]
    at = lambda x, y: int(d[y, x])
    assert at(5, 5) == 0
    assert at(6, 6) == 17 and at(8, 5) == 36 and at(10, 7) == 70 and at(10, 0) == 85
    for gy in range(12):           # every cell: 12 per step along the longer side, 5 more per step along the shorter
        for gx in range(12):
            dx, dy = sorted((abs(gx - 5), abs(gy - 5)), reverse=True)
            assert at(gx, gy) == 12 * dx + 5 * dy
    A, A_e, _, _ = RR.arrival_map_road(cls, win, road, FAR)
    assert np.array_equal(A, A_e)                      # open road: the Euclidean map


def _wall(gap):
    cls, win, road = _single_source()
    cls[:, 7], road[:, 7] = 2, 0                       # a visible wall that is not road, between the source and column 8
    if gap:
        cls[0, 7], road[0, 7] = 3, 1
    return cls, win, road


def test_wall_with_a_gap():
    cls, win, road = _wall(True)
    d, _ = RR.road_distance(cls, win, road, FAR)
    at = lambda x, y: int(d[y, x])
    assert at(6, 5) == 12 and at(7, 0) == 70 and at(8, 5) == 135 and at(8, 1) == 87 and at(8, 11) == 207
    assert (d[1:, 7] == RR.NONE).all()
    A, A_e, _, L = RR.arrival_map_road(cls, win, road, FAR)
    assert A_e[5, 8] == 2 and A[5, 8] == 3             # 135 > L[2] = 55: round the wall, not through it


def test_closed_wall_is_the_euclidean_tests_wall_case():
    cls, win, road = _wall(False)
    A, A_e, d, _ = RR.arrival_map_road(cls, win, road, [2, 8, 18])
    assert d[5, 8] == RR.NONE and A[5, 8] == 255
    assert HR.arrival_map(cls, win, road, [2, 8, 18])[0][5, 8] == 2 and A_e[5, 8] == 2
    assert (A[:, 8:] == 255).all() and (A[:, 7] == 255).all()
    assert A[5, 6] == 0 and d[5, 6] == 12


def test_diagonal_step_between_two_blocked_cells():
    cls, win, road = _single_source()
    for x, y in ((6, 5), (5, 6)):                      # the two cells touch diagonally; (6, 6) lies behind them
        cls[y, x], road[y, x] = 2, 0
    d, _ = RR.road_distance(cls, win, road, FAR)
    assert d[5, 6] == RR.NONE and d[6, 5] == RR.NONE
    assert d[6, 6] == 17                               # the permissive rule: the two end cells alone decide


def test_zero_reach_and_no_source():
    cls, win, road = _single_source()
    d, L = RR.road_distance(cls, win, road, [0, 0])
    assert L.tolist() == [0, 0] and d[5, 5] == 0 and (np.delete(d.ravel(), 5 * 12 + 5) == RR.NONE).all()
    cls[5, 5] = 3
    A, _, d, _ = RR.arrival_map_road(cls, win, road, FAR)
    assert (d == RR.NONE).all() and (A == 255).all()


# ------------------------------------------------------------------------------------------------ 2. invariants
def test_invariants_on_random_maps():
    rng = np.random.default_rng(20240131)
    later, n_hidden = 0, 0
    for case in range(60):
        rnx, rny = int(rng.integers(16, 40)), int(rng.integers(16, 40))
        road = (rng.random((rny, rnx)) < rng.uniform(0.3, 0.9)).astype(np.uint8)
        nx, ny = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        win = (int(rng.integers(-nx + 1, rnx)), int(rng.integers(-ny + 1, rny)), nx, ny)      # hangs over the raster's edge
        cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx), p=[0.15, 0.1, 0.55, 0.05, 0.05, 0.1])
        hidden = (rng.random((ny, nx)) < 0.03).astype(np.uint8) if case % 2 else None
        n_hidden += hidden is not None
        J = int(rng.integers(1, 12))
        r2 = np.sort(rng.integers(0, int(rng.integers(1, 900)), J))
        A, A_e, d, L = RR.arrival_map_road(cls, win, road, r2, hidden)
        assert (A >= A_e).all()                                   # 255 = never is the latest
        later += int((A > A_e).sum())
        assert L.tolist() == [math.isqrt(169 * int(v)) for v in r2]
        assert np.array_equal(d == 0, HR.sources(cls, win, road, hidden))
        S, P = RR.passable(cls, win, road, hidden)
        assert np.array_equal(RR.dijkstra(S, P, int(L[-1])), RR.relax_to_fixed_point(S, P, int(L[-1]))), case
        assert ((d == RR.NONE) | (d <= L[-1])).all()
    assert later > 0 and n_hidden == 30                            # the road metric does bite on these maps


def test_open_road_equals_euclid():
    """an axis-aligned rectangle of road is the only passable set: the lattice path to the nearest source is passable, so
    d^2 <= 169 D2 <= 169 R2[j] and the road metric changes nothing"""
    rng = np.random.default_rng(7)
    for case in range(20):
        rnx, rny = int(rng.integers(20, 40)), int(rng.integers(20, 40))
        x0, y0 = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        x1, y1 = int(rng.integers(x0 + 6, rnx + 1)), int(rng.integers(y0 + 6, rny + 1))
        road = np.zeros((rny, rnx), dtype=np.uint8)
        road[y0:y1, x0:x1] = 1
        nx, ny = int(rng.integers(4, 30)), int(rng.integers(4, 30))
        win = (int(rng.integers(-3, rnx - 3)), int(rng.integers(-3, rny - 3)), nx, ny)
        QX, QY = np.meshgrid(np.arange(win[0], win[0] + nx), np.arange(win[1], win[1] + ny))
        inside = (QX >= x0) & (QX < x1) & (QY >= y0) & (QY < y1)
        cls = np.where(inside, rng.choice(np.array([1, 3, 3, 3, 5], dtype=np.uint8), (ny, nx)),
                       rng.choice(np.array([0, 2], dtype=np.uint8), (ny, nx))).astype(np.uint8)
        r2 = np.sort(rng.integers(0, 500, 9))
        A, A_e, _, _ = RR.arrival_map_road(cls, win, road, r2)
        assert np.array_equal(A, A_e), case


def test_the_weights_never_exceed_thirteen_times_the_euclidean_length():
    for dx in range(300):
        for dy in range(dx + 1):
            w = 12 * dx + 5 * dy
            assert 144 * (dx * dx + dy * dy) <= w * w <= 169 * (dx * dx + dy * dy)      # ratio to 13 Euclid in [12 / 13, 1]
    assert 169 * 255 ** 2 < 2 ** 31 and 13 * 255 + 17 < 65535


# ------------------------------------------------------------------------------------------------ 3. symbol, structure, Python
def test_symbol_and_structure(native, tmp_path):
    import ctypes as C
    import subprocess
    lib = native.load()
    assert "fo_scene_hidden_reach_road" in native.EXPORTS and hasattr(lib, "fo_scene_hidden_reach_road")
    assert lib.fo_abi_version() == 12
    fields = [n for n, *_ in native.HiddenReachRoad._fields_]
    assert fields == ["base", "d_dist_or_null"]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fo_hip.h"', 'int main(void) {',
             'printf("%zu\\n", sizeof(fo_hidden_reach_road_t));', 'printf("%zu\\n", sizeof(fo_hidden_reach_t));']
    lines += ['printf("%%zu\\n", offsetof(fo_hidden_reach_road_t, %s));' % f for f in fields] + ['return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(native.HiddenReachRoad) and out[1] == C.sizeof(native.HiddenReach)
    assert out[2:] == [getattr(native.HiddenReachRoad, f).offset for f in fields]
    # no context: refused, not a crash
    assert lib.fo_scene_hidden_reach_road(None, None, None) == native.FO_E_STATE


def test_unknown_metric_is_refused_before_any_device_work(native):
    from frenetix_occlusion.sensor_model import SensorModel, hidden_reach_road_units
    z = np.zeros((2, 31))
    veh = (4.508, 1.610, 1.4227)
    for sm in (SimpleNamespace(window=None), SimpleNamespace()):          # (not even the window is looked at)
        with pytest.raises(ValueError, match="metric 'manhattan'"):
            SensorModel.hidden_reach(sm, z, z, z, vehicle=veh, v_max=13.9, dt=0.1, metric="manhattan")
    with pytest.raises(RuntimeError, match="previous launch"):            # a known metric goes on to the usual checks
        SensorModel.hidden_reach(SimpleNamespace(window=None), z, z, z, vehicle=veh, v_max=13.9, dt=0.1, metric="road")
    r2 = np.array([0, 2, 8, 18, 7225, 254 ** 2 + 2 * 254], dtype=np.int32)
    got = hidden_reach_road_units(r2)
    assert got.dtype == np.int32 and np.array_equal(got, RR.reach_units(r2)) and got.tolist() == [0, 18, 36, 55, 1105, 3314]
