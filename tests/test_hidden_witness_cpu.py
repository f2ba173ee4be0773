"""Hidden-traffic witnesses on the CPU (DESIGN.md §5.10 "Witnesses"): the checker tests/ref_hidden_witness.py is itself held to
the heap-Dijkstra checkers of the road metric and the lane flow (every walk it makes is a cheapest allowed path from a source),
to hand cases with exact routes, and the host layer (``HiddenWitness.routes / speed / select``,
``FOAgentManager.add_route_agent``) is run on CPU tensors."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_reach as HR
import ref_hidden_reach_flow as RF
import ref_hidden_reach_road as RR
import ref_hidden_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20250607
FREE = 0xFF
CS, ORIGIN = 0.5, (-3.0, 7.5)
HL, HW, WB = 2.254, 0.805, 1.4227


def sector_table(rng, rny, rnx, block=6):
    """a heading per block of cells as its three-direction sector, a fifth of the blocks free"""
    by, bx = -(-rny // block), -(-rnx // block)
    sect = np.array([RF.sector(45 * k) for k in range(8)], dtype=np.uint8)[rng.integers(0, 8, (by, bx))]
    sect[rng.random((by, bx)) < 0.2] = FREE
    return np.repeat(np.repeat(sect, block, axis=0), block, axis=1)[:rny, :rnx].copy()


def random_cases(n=42):
    """rasters of 30 .. 45 cells a side, windows that hang over each edge of the raster in turn, class bytes, a few sources (a hidden mask in
    half of the cases), reaches of 0 .. 21 cells; tables: free, random sectors, two sector tables OR-ed"""
    rng = np.random.default_rng(SEED)
    for case in range(n):
        rnx, rny = int(rng.integers(30, 46)), int(rng.integers(30, 46))
        road = (rng.random((rny, rnx)) < (0.55, 0.06)[case % 2]).astype(np.uint8)
        nx, ny = int(rng.integers(14, 30)), int(rng.integers(14, 30))
        corner = case % 5
        ix0 = [-nx // 2, rnx - (nx + 1) // 2, int(rng.integers(0, rnx - nx)), int(rng.integers(0, rnx - nx)), int(rng.integers(-nx + 1, rnx))][corner]
        iy0 = [int(rng.integers(-1, 3)), int(rng.integers(-1, 3)), -ny // 2, rny - (ny + 1) // 2, int(rng.integers(-ny + 1, rny))][corner]
        win = (ix0, iy0, nx, ny)
        cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx), p=[0.1, 0.006, 0.7, 0.007, 0.007, 0.18])
        hidden = (rng.random((ny, nx)) < 0.006).astype(np.uint8) if case % 2 else None
        if case % 4 == 3:            # two sources in the window and none outside it: long walks
            road[:] = 0
            cls[(cls & 2) == 0] = 3
            hidden = np.zeros((ny, nx), dtype=np.uint8)
            hidden.ravel()[rng.integers(0, nx * ny, 2)] = 1
        h = int(rng.integers(0, 15)) if case % 4 == 0 else int(rng.integers(9, 22))
        J = [1, 6, 12][case % 3]
        top = int(rng.integers(h * h, (h + 1) * (h + 1)))
        r2 = np.sort(rng.integers(0, top + 1, J))
        r2[-1] = top
        kind = ("free", "random", "or")[case % 3]
        moves = {"free": lambda: np.full((rny, rnx), FREE, dtype=np.uint8), "random": lambda: sector_table(rng, rny, rnx),
                 "or": lambda: sector_table(rng, rny, rnx) | sector_table(rng, rny, rnx, 4)}[kind]()
        M, T = 14, J
        x = ORIGIN[0] + (ix0 + rng.uniform(-4, nx + 4, (M, T))) * CS
        y = ORIGIN[1] + (iy0 + rng.uniform(-4, ny + 4, (M, T))) * CS
        th = rng.uniform(-math.pi, math.pi, (M, T))
        th[rng.random((M, T)) < 0.3] = 0.5 * math.pi
        head = np.stack((np.cos(th), np.sin(th)), -1)
        x[rng.random((M, T)) < 0.04] = np.nan
        yield SimpleNamespace(case=case, road=road, win=win, cls=cls, hidden=hidden, r2=r2, moves=moves, kind=kind, x=x, y=y, head=head)


def _witnesses(c, flow):
    """the maps of the Dijkstra checker for one flow, the forecast's ``first`` on them and the witness checker's outputs"""
    if flow:
        A, _, d, L = RF.arrival_map_flow(c.cls, c.win, c.road, c.moves, c.r2, c.hidden)
    else:
        A, _, d, L = RR.arrival_map_road(c.cls, c.win, c.road, c.r2, c.hidden)
    _, first, _ = HR.trajectories(A, c.win, c.road, ORIGIN, CS, c.x, c.y, c.head, HL, HW, WB)
    cap = (W.min_path_cap(c.r2[-1]) + 3) // 4 * 4
    out = W.witnesses(A, d, c.win, c.road, first, ORIGIN, CS, c.x, c.y, c.head, HL, HW, WB, cap, c.moves if flow else None)
    return A, d, L, first, cap, out


# ------------------------------------------------------------------------------------------------ 1. the checker is valid
def test_every_walk_is_a_cheapest_allowed_path_from_a_source():
    walks = cells_walked = outside = 0
    for c in random_cases():
        S, P = RR.passable(c.cls, c.win, c.road, c.hidden)       # over the window grown by one cell
        ix0, iy0, nx, ny = c.win
        for flow in (False, True):
            A, d, L, first, cap, (cell, src, steps, wdist, dirs) = _witnesses(c, flow)
            out = RF.moves_over(c.moves, c.win) if flow else np.full(S.shape, FREE, dtype=np.uint8)
            maps = W.Maps(A, d, c.win, c.road)
            for m in range(len(first)):
                if first[m] < 0:
                    assert steps[m] == -1 and wdist[m] == -1 and (cell[m] == W.NO_CELL).all() and (src[m] == W.NO_CELL).all()
                    assert (dirs[m] == 255).all()
                    continue
                n = int(steps[m])
                assert 0 <= n <= int(L[-1]) // 12 <= cap, (c.case, flow, m, n)      # never -2: no empty K on a forecast's maps
                assert maps.arrival(*cell[m]) <= first[m] and wdist[m] == maps.dist(*cell[m]) <= L[first[m]]
                assert (dirs[m, n:] == 255).all() and (dirs[m, :n] < 8).all()
                ks = [int(k) for k in dirs[m, :n][::-1]]          # travel order
                q = (int(src[m, 0]), int(src[m, 1]))
                gq = (q[0] - ix0 + 1, q[1] - iy0 + 1)             # in the grown window
                if 0 <= gq[0] < nx + 2 and 0 <= gq[1] < ny + 2:
                    assert S[gq[1], gq[0]], (c.case, flow, m)     # src is a source
                else:     # farther from the window only the conflict cell itself can lie (the footprint hangs over): raster road
                    assert n == 0 and 0 <= q[0] < c.road.shape[1] and 0 <= q[1] < c.road.shape[0] and c.road[q[1], q[0]]
                outside += not (0 <= q[0] - ix0 < nx and 0 <= q[1] - iy0 < ny)
                total = 0
                for k in ks:
                    g = (q[0] + W.DIRS[k][0], q[1] + W.DIRS[k][1])
                    gg = (g[0] - ix0 + 1, g[1] - iy0 + 1)
                    assert 0 <= gg[0] < nx + 2 and 0 <= gg[1] < ny + 2 and P[gg[1], gg[0]]                     # g is passable
                    assert (int(out[gq[1], gq[0]]) >> k) & (int(out[gg[1], gg[0]]) >> k) & 1                   # both ends allow k
                    total += W.COST[k]
                    assert maps.dist(*g) == total                 # ... and every prefix is a cheapest path itself
                    q, gq = g, gg
                assert q == (int(cell[m, 0]), int(cell[m, 1])) and total == wdist[m]
                walks += 1
                cells_walked += n
    print(f"{walks} walks over {cells_walked} cells, {outside} sources outside their window")
    assert walks > 300 and cells_walked > 1000 and outside > 10


# ------------------------------------------------------------------------------------------------ 2. hand cases
def _field(n, win_at=(20, 20)):
    """an n x n window of visible road inside a raster without road: nothing outside the window is a source"""
    road = np.zeros((60, 60), dtype=np.uint8)
    return road, (win_at[0], win_at[1], n, n), np.full((n, n), 3, dtype=np.uint8)


def test_serpentine_exact_route():
    """one-cell-wide corridors up column 0, down column 2, up column 4; the walls in columns 1 and 3 have one gap each, at the
    top and at the bottom; the only source is the foot of column 0.  The route is unique: N N N, NE and SE through the first gap,
    S S, SE and NE through the second, N N N"""
    road, win, cls = _field(5)
    cls[:, 1] = cls[:, 3] = 2
    cls[4, 1] = cls[0, 3] = 3
    cls[0, 0] = 5
    r2 = [0, 400]
    A, _, d, L = RR.arrival_map_road(cls, win, road, r2)
    assert d[4, 4] == 6 * 12 + 2 * 12 + 4 * 17 == 164 <= L[-1]
    maps = W.Maps(A, d, win, road)
    g = (win[0] + 4, win[1] + 4)
    for c in [g]:
        steps, src, dirs = W.walk(maps, c, 16)
    travel = [2, 2, 2, 1, 7, 6, 6, 7, 1, 2, 2, 2]
    assert steps == 12 and src == (win[0], win[1]) and dirs == travel[::-1]
    at = g
    for k in dirs:                                              # a unique route: one predecessor in every cell
        assert W.predecessors(maps, at) == [k]
        at = (at[0] - W.DIRS[k][0], at[1] - W.DIRS[k][1])
    # the whole definition on it: a pose whose footprint is that one cell
    x = np.array([[0.0, ORIGIN[0] + (g[0] + 0.5) * CS]])
    y = np.array([[0.0, ORIGIN[1] + (g[1] + 0.5) * CS]])
    head = np.array([[[1.0, 0.0], [1.0, 0.0]]])
    cell, s, n, wd, dd = W.witnesses(A, d, win, road, [1], ORIGIN, CS, x, y, head, 0.1, 0.1, 0.0, 16)
    assert tuple(cell[0]) == g and tuple(s[0]) == (win[0], win[1]) and n[0] == 12 and wd[0] == 164
    assert list(dd[0]) == travel[::-1] + [255] * 4
    # a row that is too short, and one that just holds it
    assert W.walk(maps, g, 12)[0] == 12
    steps, at, dirs = W.walk(maps, g, 8)
    assert steps == -2 and dirs == travel[::-1][:8] and maps.dist(*at) == 164 - (3 * 12 + 17 + 17 + 2 * 12 + 17)


def test_open_field_keeps_straight():
    """the source at (-5, -2) of g*: three E steps and two NE steps in any order are cheapest; the walk (from g* back) takes the
    lowest direction first, E, keeps it while it lies on a cheapest path, then NE"""
    road, win, cls = _field(12)
    g, s = (win[0] + 8, win[1] + 6), (win[0] + 3, win[1] + 4)
    cls[s[1] - win[1], s[0] - win[0]] = 5
    A, _, d, L = RR.arrival_map_road(cls, win, road, [0, 64])
    maps = W.Maps(A, d, win, road)
    assert maps.dist(*g) == 3 * 12 + 2 * 17
    assert W.predecessors(maps, g) == [0, 1]
    steps, src, dirs = W.walk(maps, g, 8)
    assert (steps, src, dirs) == (5, s, [0, 0, 0, 1, 1])


def test_one_way_lane_walks_upstream():
    """a lane of one row that runs east, a source three cells downstream of g* and one six cells upstream: along the road the
    nearer one is the witness, along the lanes only the upstream one can arrive"""
    road, win, cls = _field(14)
    cls[:] = 2
    cls[5, 1:13] = 3
    cls[5, 2] = cls[5, 11] = 5
    moves = np.full(road.shape, RF.sector(0), dtype=np.uint8)
    g = (win[0] + 8, win[1] + 5)
    A, _, d, _ = RR.arrival_map_road(cls, win, road, [0, 100])
    assert W.walk(W.Maps(A, d, win, road), g, 12) == (3, (win[0] + 11, win[1] + 5), [4, 4, 4])
    A, _, d, _ = RF.arrival_map_flow(cls, win, road, moves, [0, 100])
    assert W.walk(W.Maps(A, d, win, road, moves), g, 12) == (6, (win[0] + 2, win[1] + 5), [0] * 6)
    assert d[5, 12] == 12 and d[5, 10] == 8 * 12                # nothing drives west out of the downstream source


# ------------------------------------------------------------------------------------------------ 3. the free table
def test_free_table_gives_the_road_witness():
    n = 0
    for c in random_cases(12):
        c.moves = np.full(c.road.shape, FREE, dtype=np.uint8)
        road, flow = _witnesses(c, False), _witnesses(c, True)
        assert np.array_equal(road[1], flow[1])
        for a, b in zip(road[5], flow[5]):
            assert a.dtype == b.dtype and np.array_equal(a, b), c.case
        n += int((road[5][2] > 0).sum())
    assert n > 30


# ------------------------------------------------------------------------------------------------ 4. the host layer
def _host_witness(c, flow=True, dt=0.1, v_max=8.0):
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.cell_window import CellWindow  # noqa: F401  (the package imports without a GPU)
    from frenetix_occlusion.hidden_traffic import HiddenReach, HiddenWitness
    A, d, L, first, cap, (cell, src, steps, wdist, dirs) = _witnesses(c, flow)
    t = torch.as_tensor
    reach = HiddenReach(t(A), torch.zeros(c.x.shape, dtype=torch.int32), t(first), torch.zeros(len(first), dtype=torch.int32),
                        np.asarray(c.r2, dtype=np.int32), c.win, metric="road", flow="lanes" if flow else "any")
    return HiddenWitness(reach, t(cell), t(src), t(steps), t(wdist), t(dirs), ORIGIN, CS, dt, v_max, cap), first


def test_routes_and_speed_on_cpu_tensors():
    seen = 0
    for c in random_cases(12):
        # the forecast's own reach table for (v_max, dt, margin): the speed bound speaks of it
        dt, v_max, margin, T = 0.1, 8.0, math.sqrt(2.0) * CS, c.x.shape[1]
        c.r2 = HR.reach_table(v_max, dt, margin, CS, T)
        w, first = _host_witness(c, flow=c.case % 2 == 0, dt=dt, v_max=v_max)
        steps, src, cell, dirs = (np.asarray(getattr(w, n)) for n in ("steps", "source", "cell", "dirs"))
        idx = list(range(len(first)))
        for m, route in zip(idx, w.routes(idx)):
            if steps[m] < 0:
                assert route is None and w.speed(m) == 0.0
                continue
            n = int(steps[m])
            assert route.dtype == np.float64 and route.shape == (n + 1, 2)
            centre = lambda g: (ORIGIN[0] + (g[0] + 0.5) * CS, ORIGIN[1] + (g[1] + 0.5) * CS)
            assert tuple(route[0]) == centre(src[m]) and np.allclose(route[-1], centre(cell[m]), atol=1e-12, rtol=0)
            hops = np.array([W.DIRS[k] for k in dirs[m, :n][::-1]], dtype=np.float64).reshape(n, 2) * CS      # travel order
            assert np.allclose(np.diff(route, axis=0), hops, atol=1e-12, rtol=0)
            length = float(np.hypot(hops[:, 0], hops[:, 1]).sum())
            k = int(first[m])
            if k == 0:
                assert w.speed(m) == 0.0
            else:
                assert w.speed(m) == pytest.approx(length / (k * dt), rel=1e-12)
                assert w.speed(m) <= 13.0 / 12.0 * (v_max + margin / (k * dt)) * (1 + 1e-12)
                seen += n > 0
    assert seen > 10


def test_select_groups_by_source_block_and_orders_by_arrival():
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import HiddenReach, HiddenWitness
    #          m:   0         1         2        3         4         5          6
    src = [(8, 8), (9, 10), (40, 3), (11, 11), (-1, -1), (41, 2), (W.NO_CELL, W.NO_CELL)]
    first = [5, 3, 3, 3, 9, 7, -1]
    dist = [60, 41, 12, 29, 0, 5, -1]
    steps = [5, 3, 1, 2, 0, 1, -1]
    t = lambda a, dt=torch.int32: torch.as_tensor(np.array(a), dtype=dt)
    reach = HiddenReach(None, None, t(first), None, np.zeros(10, dtype=np.int32), None)
    w = HiddenWitness(reach, t(src), t(src), t(steps), t(dist), torch.full((7, 8), 255, dtype=torch.uint8), ORIGIN, CS, 0.1, 8.0, 8)
    # blocks of 4 cells: (2, 2) holds m = 0, 1, 3 -> the smallest (k*, dist, m) is m = 3; (10, 0) holds 2, 5 -> 2; (-1, -1) holds 4
    assert w.select() == [2, 3, 4]
    assert w.select(max_agents=2) == [2, 3] and w.select(max_agents=0) == []
    # single cells: everyone on its own, ordered by (k*, dist, m)
    assert w.select(merge_cells=1) == [2, 3, 1, 0, 5, 4]
    # one block for all: the earliest, nearest witness
    assert w.select(merge_cells=1 << 20) == [2, 4]              # (floor division: the cell (-1, -1) lies in block (-1, -1))


def _agent_manager(dt):
    import yaml
    pytest.importorskip("torch")
    from frenetix_occlusion import interface
    from frenetix_occlusion.agent import FOAgentManager
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    return FOAgentManager(SimpleNamespace(obstacles=[]), np.array([[0.0, 0.0], [10.0, 0.0]]), cfg["agent_manager"], 0, dt=dt, device="cpu")


def test_route_agents_pass_the_conflict_cell_at_their_sample():
    from frenetix_occlusion.agent import FOAgentManager  # noqa: F401
    added = 0
    for c in (c for c in random_cases(30) if c.case < 4 or c.case % 4 == 3):      # (the cases with long walks, and a few others)
        dt, v_max, T = 0.1, 8.0, c.x.shape[1]
        c.r2 = HR.reach_table(v_max, dt, math.sqrt(2.0) * CS, CS, T)
        w, first = _host_witness(c, flow=c.case % 2 == 1, dt=dt, v_max=v_max)
        am = _agent_manager(dt)
        picked = [m for m in range(len(first)) if int(w.steps[m]) >= 0]       # (every witness: select has its own test)
        assert set(w.select(max_agents=99, merge_cells=1)) <= set(picked)
        for m, route in zip(picked, w.routes(picked)):
            a = am.add_route_agent(route, w.speed(m), agent_type="Car", horizon=(T - 0.5) * dt)
            assert am._manual[-1] is a and am._pred_cache is None and len(a.predictions) == 1
            p = a.predictions[0]
            assert p["pos_list"].shape == (T, 2) and len(p["v_list"]) == len(p["orientation_list"]) == T and p["cov_list"].shape == (T, 2, 2)
            k = int(first[m])
            assert np.abs(p["pos_list"][0] - route[0]).max() <= 1e-9
            if k > 0 or len(route) == 1:
                assert np.abs(p["pos_list"][k] - route[-1]).max() <= 1e-9, (c.case, m, k)      # at the conflict cell's centre at k*
            if len(route) > 1:
                seg = route[1] - route[0]
                assert a.initial_orientation == pytest.approx(math.atan2(seg[1], seg[0]))
            added += k > 0 and len(route) > 2
        assert len(am._manual) == len(picked)
    assert added > 5
    # a one-point route stands still
    am = _agent_manager(0.1)
    a = am.add_route_agent(np.array([[3.0, 4.0]]), 0.0, horizon=2.95)
    assert np.array_equal(a.predictions[0]["pos_list"], np.tile([[3.0, 4.0]], (30, 1))) and (a.predictions[0]["v_list"] == 0.0).all()
    with pytest.raises(NotImplementedError):
        am.add_route_agent(np.array([[3.0, 4.0]]), 0.0, agent_type="Tram")


# ------------------------------------------------------------------------------------------------ 5. the launch plan
_PLAN_DRIVER = r"""
#include <cstdio>
#include "fo_hip.h"
#include "fo_scene_plan.hpp"
int main() {
  long long M, r2;
  printf("%d %d %d\n", HW_LANES, HW_PER_BLOCK, FO_HIDDEN_WITNESS_MAX_STEPS);
  while (scanf("%lld %lld", &M, &r2) == 2) printf("%d %d\n", witness_blocks((int)M), witness_min_cap((int)r2));
  return 0;
}
"""


def test_launch_plan_and_limits(tmp_path):
    """the host functions of csrc/fo_scene_plan.hpp behind the launch (built alone with the host compiler): 32 trajectories per
    workgroup, the shortest row is the checker's, and FO_HIDDEN_WITNESS_MAX_STEPS serves every reach the forecast accepts"""
    import shutil
    import subprocess
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "driver.cpp").write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "driver")
    csrc = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"), "-o", exe])
    asked = [(M, r2) for M in (0, 1, 31, 32, 33, 64, 70, 10000, 2 ** 31 - 1) for r2 in (0, 1, 2, 2379, 7056, 254 ** 2, 255 ** 2 - 1)]
    out = subprocess.run([exe], input="\n".join(f"{M} {r2}" for M, r2 in asked) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [8, 32, 276]
    for (M, r2), line in zip(asked, out[1:]):
        assert [int(v) for v in line.split()] == [-(-M // 32), W.min_path_cap(r2)], (M, r2)
    assert W.min_path_cap(255 ** 2 - 1) == 276 and W.min_path_cap(2379) == 52        # the halo cap; the exact-row case of the GPU test
    from frenetix_occlusion import _native as N
    from frenetix_occlusion.hidden_traffic import witness_path_cap
    assert N.HIDDEN_WITNESS_MAX_STEPS == 276 and witness_path_cap([0, 255 ** 2 - 1]) == 276 and witness_path_cap([2379]) == 52
    assert witness_path_cap([7056]) == 92 and witness_path_cap([0]) == 0
