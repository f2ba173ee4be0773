"""Lane flow of the hidden-traffic reach forecast on the device (fo_scene_set_lane_moves, fo_scene_hidden_reach_flow,
fo_scene_hidden_clearance_flow; DESIGN.md §5.10 "Lane flow") against the heap-Dijkstra statement of its definition
(tests/ref_hidden_reach_flow.py), with move tables of the test's own.  Every output is an exact integer: all comparisons are ``==``."""
import glob
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_clearance as HC
import ref_hidden_reach as HR
import ref_hidden_reach_flow as RF
import ref_hidden_reach_road as RR
import test_hidden_reach_gpu as T
import test_hidden_reach_road_gpu as RG
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DT, VEH, HL, HW, WB = T.DT, T.VEH, T.HL, T.HW, T.WB
_np = T._np
TILE, BAND = RG.TILE, RG.BAND
SEED = 20250301
FREE = 0xFF


# ------------------------------------------------------------------------------------------------ raw entries
def _set_moves(sm, moves):
    """the test's own table in the place of the model's (None: no table)"""
    if moves is None:
        return sm.ctx._lib.fo_scene_set_lane_moves(sm.ctx._h, None)
    moves = np.ascontiguousarray(moves, dtype=np.uint8)
    assert moves.shape == tuple(sm.raster_dims)[::-1]
    return sm.ctx._lib.fo_scene_set_lane_moves(sm.ctx._h, moves.ctypes.data)


def _raw_reach(torch, sm, entry, cls, win, r2, hidden=None, x=None, y=None, head=None, lens=None, dist=True, **over):
    """fo_scene_hidden_reach_flow / _road (``entry``) with class bytes / windows / tables of the test's own; returns
    (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_cls, d_hid = up(cls, np.uint8), up(hidden, np.uint8)
    M = 0 if x is None else x.shape[0]
    Tn = 1 if x is None else x.shape[1]
    tx, ty, th, tl = up(x, np.float64), up(y, np.float64), up(head, np.float64), up(lens, np.int32)
    arrival = torch.full((win[3], win[2]), 77, dtype=torch.uint8, device=dev)
    d_dist = torch.full((win[3], win[2]), 7777, dtype=torch.int16, device=dev)      # (the bytes of a uint16 map)
    cells = torch.full((M, Tn), -7, dtype=torch.int32, device=dev)
    first = torch.full((M,), -7, dtype=torch.int32, device=dev)
    slack = torch.full((M,), -7, dtype=torch.int32, device=dev)
    r2 = np.ascontiguousarray(r2, dtype=np.int32)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=HL, hw=HW, wb=WB, J=len(r2),
              h_r2=r2.ctypes.data_as(C.POINTER(C.c_int32)), d_cls=p(d_cls), d_hidden_or_null=p(d_hid), win_ix0=win[0],
              win_iy0=win[1], win_nx=win[2], win_ny=win[3], d_arrival=arrival.data_ptr(), d_cells=p(cells), d_first=p(first),
              d_slack=p(slack))
    kw.update(over)
    args = N.HiddenReachRoad(base=N.HiddenReach(**kw), d_dist_or_null=d_dist.data_ptr() if dist else None)
    rc = getattr(sm.ctx._lib, entry)(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(arrival=_np(arrival), dist=_np(d_dist).view(np.uint16), cells=_np(cells), first=_np(first),
                                    slack=_np(slack))


def _raw_clearance(torch, sm, cls, win, r2_cap, hidden=None, x=None, y=None, head=None, lens=None, metric=1):
    """fo_scene_hidden_clearance_flow; returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_cls, d_hid = up(cls, np.uint8), up(hidden, np.uint8)
    M = 0 if x is None else x.shape[0]
    Tn = 1 if x is None else x.shape[1]
    tx, ty, th, tl = up(x, np.float64), up(y, np.float64), up(head, np.float64), up(lens, np.int32)
    key = torch.full((win[3], win[2]), -7, dtype=torch.int32, device=dev)
    qmin = torch.full((M, Tn), -7, dtype=torch.int32, device=dev)
    d_dist = torch.full((win[3], win[2]), 7777, dtype=torch.int16, device=dev)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    args = N.HiddenClearance(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=HL, hw=HW, wb=WB,
                             r2_cap=int(r2_cap), metric=metric, d_cls=p(d_cls), d_hidden_or_null=p(d_hid), win_ix0=win[0],
                             win_iy0=win[1], win_nx=win[2], win_ny=win[3], d_key=key.data_ptr(), d_qmin=p(qmin),
                             d_dist_or_null=d_dist.data_ptr())
    rc = sm.ctx._lib.fo_scene_hidden_clearance_flow(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(key=_np(key), qmin=_np(qmin), dist=_np(d_dist).view(np.uint16))


# ------------------------------------------------------------------------------------------------ the random cases
def block_table(rng, rny, rnx):
    """a heading (a multiple of 45 degrees) constant per 8 x 8 block, turned into its three-direction sector; a quarter of the
    blocks free, and a further 5 % of single cells"""
    by, bx = (rny + 7) // 8, (rnx + 7) // 8
    sect = np.array([RF.sector(45 * k) for k in range(8)], dtype=np.uint8)[rng.integers(0, 8, (by, bx))]
    sect[rng.random((by, bx)) < 0.25] = FREE
    moves = np.repeat(np.repeat(sect, 8, axis=0), 8, axis=1)[:rny, :rnx].copy()
    moves[rng.random((rny, rnx)) < 0.05] = FREE
    return moves


def random_cases(sm, rnx, rny, cap, n=40):
    """the cases of the road metric's device test (window shapes, a window over every edge of the raster in turn, reaches from 0
    to the cap with windows cut to 24 x 24 above 60, a hidden mask in half of them, poses, ragged lengths), each with a table of
    its own.  ``sm``: anything with ``cell_size`` and ``raster_origin``"""
    rng = np.random.default_rng(SEED)
    halos = [0, 1, 3, 13, 34, 64, 65, cap]
    shapes = [(1, 1), (1, 37), (41, 1), (TILE, TILE), (TILE + 1, TILE + 1), (TILE, TILE + 1), (97, 70), (70, 45)]
    for case in range(n):
        h = halos[case % len(halos)]
        nx, ny = shapes[(case // len(halos) + case) % len(shapes)]
        if h > 60:
            nx, ny = min(nx, 24), min(ny, 24)
        corner = case % 5            # the four edges of the raster in turn, then anywhere
        ix0 = [-nx // 2, rnx - (nx + 1) // 2, int(rng.integers(0, max(rnx - nx, 1))), int(rng.integers(0, max(rnx - nx, 1))),
               int(rng.integers(-nx + 1, rnx))][corner]
        iy0 = [int(rng.integers(-1, 3)), int(rng.integers(-1, 3)), -ny // 2, rny - (ny + 1) // 2, int(rng.integers(-ny + 1, rny))][corner]
        win = (ix0, iy0, nx, ny)
        cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx), p=[0.12, 0.04, 0.6, 0.03, 0.03, 0.18])
        hidden = (rng.random((ny, nx)) < 0.02).astype(np.uint8) if case % 2 else None
        if hidden is not None and h > 60:                 # two sources alone: distances of several bands in a small window
            hidden[:] = 0
            hidden.ravel()[rng.integers(0, nx * ny, 2)] = 1
        J = [1, 31, 254, 7][case % 4]
        top = int(rng.integers(h * h, (h + 1) * (h + 1)))
        r2 = np.sort(rng.integers(0, top + 1, J))
        r2[-1] = top
        Tn = min([1, 31, J][case % 3], J)
        M = [37, 70, 1, 129][case % 4]
        x, y, head = T._random_poses(rng, sm, win, M, Tn)
        lens = rng.integers(-1, Tn + 2, M).astype(np.int32) if case % 2 else None
        yield SimpleNamespace(case=case, h=h, win=win, cls=cls, hidden=hidden, r2=r2, x=x, y=y, head=head, lens=lens,
                              moves=block_table(rng, rny, rnx))


def _parked():
    lanes, obstacles, _ = T._parked_car_scene()
    sm, _ = T._sensor(lanes, obstacles)
    return sm, sm.road_raster()


def test_random_class_maps_windows_tables_and_poses(torch_cuda):
    """40 seeded cases on the parked-car map, every output against the checker; the lanes bite (cells arrive later and cells are
    cut off), one band and eighteen both occur"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    edges, seen_bands = set(), set()
    reached = later = cut = 0
    for c in random_cases(sm, rnx, rny, N.HIDDEN_REACH_MAX_HALO):
        assert _set_moves(sm, c.moves) == N.FO_OK
        ix0, iy0, nx, ny = c.win
        edges |= {e for e, over in zip("lrbt", (ix0 < 0, ix0 + nx > rnx, iy0 < 0, iy0 + ny > rny)) if over}
        rc, msg, out = _raw_reach(torch, sm, "fo_scene_hidden_reach_flow", c.cls, c.win, c.r2, c.hidden, c.x, c.y, c.head, c.lens,
                                  dist=c.case % 7 != 6)
        assert rc == 0, msg
        A, A_e, d, L = RF.arrival_map_flow(c.cls, c.win, road, c.moves, c.r2, c.hidden)
        if c.case % 7 != 6:
            assert np.array_equal(out.dist, d), (c.case, c.h, c.win, int((out.dist != d).sum()))
        else:
            assert (out.dist == 7777).all()               # no buffer handed in: the distances stay in the context
        assert np.array_equal(out.arrival, A), (c.case, c.h, c.win)
        cells, first, slack = HR.trajectories(A, c.win, road, sm.raster_origin, sm.cell_size, c.x, c.y, c.head, HL, HW, WB, c.lens)
        assert np.array_equal(out.cells, cells), c.case
        assert np.array_equal(out.first, first) and np.array_equal(out.slack, slack), c.case
        d_road, _ = RR.road_distance(c.cls, c.win, road, c.r2, c.hidden)
        on = (d_road > 0) & (d_road < RR.NONE)
        reached += int(on.sum())
        later += int((on & (d > d_road) & (d < RF.NONE)).sum())
        cut += int((on & (d == RF.NONE)).sum())
        seen_bands.add(max(-(-int(L[-1]) // BAND), 1))
    print(f"{reached} cells within the road's reach: {later} later along the lanes, {cut} cut off; bands {sorted(seen_bands)}")
    assert edges == set("lrbt") and {1, 18} <= seen_bands
    assert later > 0.05 * reached and cut > 0.01 * reached       # not vacuous: the tables change the answer


def test_free_table_equals_the_road_entry(torch_cuda):
    """a table of 0xFF: the flow entry's outputs are the road entry's, byte for byte, on ten of the random cases"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    assert _set_moves(sm, np.full((rny, rnx), FREE, dtype=np.uint8)) == N.FO_OK
    finite = 0
    for c in random_cases(sm, rnx, rny, N.HIDDEN_REACH_MAX_HALO, n=10):
        got = {}
        for entry in ("fo_scene_hidden_reach_flow", "fo_scene_hidden_reach_road"):
            rc, msg, got[entry] = _raw_reach(torch, sm, entry, c.cls, c.win, c.r2, c.hidden, c.x, c.y, c.head, c.lens)
            assert rc == 0, msg
        a, b = got.values()
        for k in ("dist", "arrival", "cells", "first", "slack"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (c.case, k)
        finite += int(((a.dist > 0) & (a.dist < RR.NONE)).sum())
    assert finite > 100


# ------------------------------------------------------------------------------------------------ the serpentine
def _two_streets():
    """two parallel streets 60 m apart: the raster between them is on the map and not road, so that a window there has no source
    outside it and still reads the move table (off the raster every byte is 0xFF, whatever the table says)"""
    from frenetix_occlusion import scenario as S

    def straight(lid, y_lo, y_hi, n=41):
        xs = np.linspace(-10, 70, n)
        return S.Lanelet(lid, np.stack((xs, np.full(n, y_hi)), -1), np.stack((xs, np.full(n, y_lo)), -1))
    sm, _ = T._sensor([straight(1, -3.5, 0.0), straight(2, 60.0, 63.5)], [])
    return sm, sm.road_raster()


def test_directed_serpentine(torch_cuda):
    """the road test's serpentine (walls in every second column, their gaps alternately at the top and at the bottom, one source
    in a corner) in a 40 x 40 window over cells of the raster that are not road: nothing outside the window is a source, as off
    the raster, and the table is read.  Every corridor is one-way in its direction of travel (the two end rows, where the path
    turns, are free): the distances are the road metric's.  With one corridor reversed everything behind it is 65535.  The
    path crosses the border between the tiles in every column and more than four bands."""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _two_streets()
    rny, rnx = road.shape
    n = 40
    win = (30, 40, n, n)
    assert rnx >= win[0] + n + 1 and rny >= win[1] + n + 1
    assert not road[win[1] - 1:win[1] + n + 1, win[0] - 1:win[0] + n + 1].any()
    cls = np.full((n, n), 3, dtype=np.uint8)
    for c in range(1, n, 2):
        cls[:, c] = 2
        cls[n - 1 if c % 4 == 1 else 0, c] = 3
    cls[0, 0] = 5
    lane = np.full((n, n), FREE, dtype=np.uint8)
    for c in range(0, n, 2):
        lane[1:n - 1, c] = RF.sector(90 if c % 4 == 0 else 270)
    r2 = [0, 100, 2500, 10000, 40000, 254 ** 2]
    A_r, A_e, d_road, L = RR.arrival_map_road(cls, win, road, r2)
    assert L[-1] == 13 * 254 and L[-1] >= 4 * BAND
    assert d_road[n - 1, 1] == (n - 2) * 12 + 17              # up the first column, diagonally into the gap
    for reverse in (None, 4):
        moves = np.full((rny, rnx), RF.sector(0), dtype=np.uint8)      # (outside the window: anything, it is not passable)
        here = lane.copy()
        if reverse is not None:
            here[1:n - 1, reverse] = RF.sector(270)
        moves[win[1]:win[1] + n, win[0]:win[0] + n] = here
        assert _set_moves(sm, moves) == N.FO_OK
        A, _, d, _ = RF.arrival_map_flow(cls, win, road, moves, r2)
        if reverse is None:
            assert np.array_equal(d, d_road) and np.array_equal(A, A_r)
            assert (d[(cls & 1) != 0] < RF.NONE).sum() > 4 * BAND // 12
        else:
            assert np.array_equal(d[:, :reverse], d_road[:, :reverse]) and d[0, reverse] == d_road[0, reverse]
            assert (d[1:, reverse] == RF.NONE).all() and (d[:, reverse + 1:] == RF.NONE).all()
            assert (d_road[:, reverse + 1:] < RF.NONE).sum() > 100
        rc, msg, out = _raw_reach(torch, sm, "fo_scene_hidden_reach_flow", cls, win, r2)
        assert rc == 0, msg
        assert np.array_equal(out.dist, d), (reverse, int((out.dist != d).sum()))
        assert np.array_equal(out.arrival, A)


# ------------------------------------------------------------------------------------------------ clearance
def _key_map_flow(cls, win, road, moves, r2_cap, hidden):
    """key = max(169 D2, d_flow^2) on road cells within the cap, NONE elsewhere (ref_hidden_clearance.key_map with d_flow)"""
    key = HC.key_map(cls, win, road, r2_cap, "euclid", hidden)[0]
    lcap = math.isqrt(169 * int(r2_cap))
    S, P = RR.passable(cls, win, road, hidden)
    d = RF.dijkstra(S, P, RF.moves_over(moves, win), lcap)[1:-1, 1:-1]
    near = (key != HC.NONE) & (d != RF.NONE)
    return np.where(near, np.maximum(key, d * d), HC.NONE).astype(np.int64), d


def test_clearance_key_and_qmin_match_the_checker(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    rng = np.random.default_rng(SEED + 1)
    later = cut = 0
    for n, (nx, ny, h) in enumerate([(33, 33, 3), (33, 33, 17), (70, 45, 17), (70, 45, 40), (8, 8, N.HIDDEN_REACH_MAX_HALO)]):
        win = ([int(rng.integers(5, rnx - nx - 5)), -nx // 3, rnx - nx // 2][n % 3], [int(rng.integers(-2, 4)), rny - ny // 2, -3][n % 3],
               nx, ny)
        cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx), p=[0.1, 0.04, 0.62, 0.03, 0.03, 0.18])
        hidden = (rng.random((ny, nx)) < 0.02).astype(np.uint8) if n % 2 else None
        if h > 60:
            hidden = np.zeros((ny, nx), dtype=np.uint8)
            hidden.ravel()[rng.integers(0, nx * ny, 2)] = 1
        r2_cap = int(rng.integers(h * h, (h + 1) * (h + 1)))
        Tn, M = [1, 5, 33][n % 3], [70, 1][n % 2]
        x, y, head = T._random_poses(rng, sm, win, M, Tn)
        lens = rng.integers(-1, Tn + 2, M).astype(np.int32) if n % 2 else None
        moves = block_table(rng, rny, rnx)
        assert _set_moves(sm, moves) == N.FO_OK
        rc, msg, out = _raw_clearance(torch, sm, cls, win, r2_cap, hidden, x, y, head, lens)
        assert rc == 0, msg
        key, d = _key_map_flow(cls, win, road, moves, r2_cap, hidden)
        assert np.array_equal(out.dist, d.astype(np.uint16)), (n, int((out.dist != d).sum()))
        assert np.array_equal(out.key, key), (n, int((out.key != key).sum()))
        qmin = HC.clearance(key, win, road, sm.raster_origin, sm.cell_size, x, y, head, HL, HW, WB, lens)
        assert np.array_equal(out.qmin, qmin), (n, int((out.qmin != qmin).sum()))
        kr = HC.key_map(cls, win, road, r2_cap, "road", hidden)[0]
        assert (key >= kr).all()
        later += int(((key > kr) & (key != HC.NONE)).sum())
        cut += int(((key == HC.NONE) & (kr != HC.NONE)).sum())
    assert later > 0 and cut > 0


def test_reach_from_the_flow_clearance_equals_hidden_reach(torch_cuda):
    """one visibility stage on scenario 1, the model's own table: what ``.reach(v)`` derives from the flow clearance is
    ``hidden_reach(v, metric="road", flow="lanes")``'s cells > 0, first and slack; no trajectory's critical speed falls"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    sc = T._scenario("scenario1")
    sm, obs = T._sensor(sc)
    ego, yaw = T._drive(torch, sm, obs, sc, 1)
    traj = SY.make_trajectories(128, 31, DT, seed=SEED, ego_pos=ego, ego_yaw=yaw)
    speeds = (2.0, 7.0, 13.9)
    args = (traj["x"], traj["y"], traj["theta"])
    hc = sm.hidden_clearance(*args, vehicle=VEH, v_cap=speeds[-1], dt=DT, metric="road", flow="lanes")
    assert hc.metric == "road" and hc.flow == "lanes" and hc.dist is not None
    cls, win, road, hid = T._state(torch, sm)
    key, d = _key_map_flow(cls, win, road, sm.lane_moves, hc.r2_cap, hid)
    assert np.array_equal(_np(hc.key), key) and np.array_equal(_np(hc.dist), d.astype(np.uint16))
    hits = 0
    for v in speeds:
        hr = sm.hidden_reach(*args, vehicle=VEH, v_max=v, dt=DT, metric="road", flow="lanes")
        assert hr.flow == "lanes"
        hit, first, slack = hc.reach(v)
        assert np.array_equal(_np(hit), _np(hr.cells) > 0), v
        assert np.array_equal(_np(first), _np(hr.first)) and np.array_equal(_np(slack), _np(hr.slack)), v
        hits += int((_np(hr.first) >= 0).sum())
    assert hits > 0
    any_ = sm.hidden_clearance(*args, vehicle=VEH, v_cap=speeds[-1], dt=DT, metric="road")
    assert any_.flow == "any"
    v_lanes, v_any = _np(hc.critical_speed()), _np(any_.critical_speed())
    assert (v_lanes >= v_any).all()
    print(f"critical speed: {int((v_lanes > v_any).sum())} of {len(v_any)} trajectories rise with the lanes")


# ------------------------------------------------------------------------------------------------ scenarios, through the interface
def _interface(tmp_path, sc):
    import yaml
    from frenetix_occlusion import interface, synthetic as SY
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["accelerator"]["spawn"]["mode"] = "cells"
    cfg["sensor_model"]["sensor_radius"], cfg["sensor_model"]["sensor_angle"] = 50.0, 360.0
    p = tmp_path / "occ.yaml"
    p.write_text(yaml.safe_dump(cfg))
    ego = np.asarray(sc.ego_initial, dtype=np.float64)
    path = ego[None, :2] + np.linspace(0.0, 80.0, 81)[:, None] * np.array([[math.cos(ego[2]), math.sin(ego[2])]])
    veh = SimpleNamespace(**dict(zip(("length", "width", "wb_rear_axle", "mass", "a_max"), SY.VEHICLE_BMW320I)))
    return interface.FOInterface(sc, path, veh, DT, config_path=str(p))


def _own_lane_ahead(sc, sm, win, ego, yaw):
    """bool [ny, nx]: window cells whose centre lies in the ego's own lane -- a lanelet that holds the ego's position, or one that
    follows such a lanelet (successors, transitively) -- ahead of the ego"""
    from frenetix_occlusion.scenario import points_in_polygon
    ix0, iy0, nx, ny = win
    cs, (x0, y0) = sm.cell_size, sm.raster_origin
    gx, gy = np.meshgrid(x0 + (ix0 + np.arange(nx) + 0.5) * cs, y0 + (iy0 + np.arange(ny) + 0.5) * cs)
    q = np.stack((gx.ravel(), gy.ravel()), -1)
    by_id = {ll.lanelet_id: ll for ll in sc.lanelets}
    todo = [ll.lanelet_id for ll in sc.lanelets if points_in_polygon(np.asarray(ego, dtype=np.float64)[None, :2], ll.polygon)[0]]
    lane, own = set(), np.zeros(nx * ny, dtype=bool)
    while todo:
        lid = todo.pop()
        if lid in lane or lid not in by_id:
            continue
        lane.add(lid)
        own |= points_in_polygon(q, by_id[lid].polygon)
        todo += list(by_id[lid].successors)
    ahead = (q[:, 0] - ego[0]) * math.cos(yaw) + (q[:, 1] - ego[1]) * math.sin(yaw) > 0.0
    return (own & ahead).reshape(ny, nx)


@pytest.mark.parametrize("name", ["scenario1", "city_grid"])
def test_scenarios_through_the_interface(torch_cuda, tmp_path, name):
    """a few steps of a drive, then ``hidden_reach(metric="road", flow="lanes")`` against the checker with the model's own table;
    the ego's own lane no longer arrives from the stretch ahead of it"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    sc = T._scenario(name)
    fo = _interface(tmp_path, sc)
    ego0 = np.asarray(sc.ego_initial, dtype=np.float64)
    yaw = float(ego0[2])
    for step in range(3):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        fo.evaluate_scenario({}, ego, yaw, (0.7634 * step, 0.0), float(ego0[3]), step, None)
    sm = fo.sensor_model
    assert sm.lane_moves is not None and sm.lane_moves.dtype == np.uint8 and sm.lane_moves.shape == tuple(sm.raster_dims)[::-1]
    on_lane = ~np.isnan(sm.lane_yaw)
    assert (sm.lane_moves[~on_lane] == FREE).all() and (sm.lane_moves[on_lane] != 0).all()
    assert (sm.lane_moves[on_lane] != FREE).sum() > 0.9 * on_lane.sum()      # (0xFF on a lane: where lanelets of every direction cross)
    traj = SY.make_trajectories(70, 31, DT, seed=SEED, ego_pos=ego, ego_yaw=yaw)
    with pytest.raises(ValueError, match="flow"):
        fo.hidden_reach(traj, metric="road", flow="left")
    out = fo.hidden_reach(traj, v_max=13.9, metric="road", flow="lanes")
    assert out.metric == "road" and out.flow == "lanes"
    cls, win, road, hid = T._state(torch, sm)
    A, A_e, d, L = RF.arrival_map_flow(cls, win, road, sm.lane_moves, out.r2, hid)
    assert np.array_equal(out.reach, L)
    got_d = _np(out.road_dist)
    assert got_d.dtype == np.uint16 and np.array_equal(got_d, d), f"{int((got_d != d).sum())} distances differ"
    assert np.array_equal(_np(out.arrival), A)
    x, y = np.asarray(traj["x"]), np.asarray(traj["y"])
    cells, first, slack = HR.trajectories(A, win, road, sm.raster_origin, sm.cell_size, x, y, _np(out.heading), HL, HW, WB)
    assert np.array_equal(_np(out.cells), cells)
    assert np.array_equal(_np(out.first), first) and np.array_equal(_np(out.slack), slack)
    rd = fo.hidden_reach(traj, v_max=13.9, metric="road")
    assert rd.flow == "any"
    A_road = _np(rd.arrival)
    assert np.array_equal(A_road, RR.arrival_map_road(cls, win, road, out.r2, hid)[0])
    assert (A >= A_road).all() and (A_road >= A_e).all()
    lane = _own_lane_ahead(sc, sm, win, ego, yaw) & ((cls & 1) != 0)
    assert lane.sum() > 20
    later = lane & (A > A_road)
    print(f"{name}: {int(later.sum())} of {int(lane.sum())} road cells of the ego's lane ahead arrive later with the lanes, "
          f"{int((later & (A == 255)).sum())} of them never")
    assert later.any()
    hc = fo.hidden_clearance(traj, v_cap=13.9, metric="road", flow="lanes")
    assert hc.flow == "lanes" and np.array_equal(_np(hc.dist), d)


# ------------------------------------------------------------------------------------------------ refusals and state
def test_refusals_and_the_state_of_the_table(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, road = _parked()
    rny, rnx = road.shape
    lib = sm.ctx._lib
    win = (3, 1, 12, 9)
    cls = np.full((9, 12), 5, dtype=np.uint8)
    x = np.zeros((2, 4))
    head = np.zeros((2, 4, 2))
    head[..., 0] = 1.0
    r2 = [2, 2, 8, 30]

    def reach():
        return _raw_reach(torch, sm, "fo_scene_hidden_reach_flow", cls, win, r2, None, x, x, head)

    def untouched_reach(out):
        return ((out.arrival == 77).all() and (out.cells == -7).all() and (out.first == -7).all() and (out.slack == -7).all()
                and (out.dist == 7777).all())

    # the model uploaded its own table: served
    rc, msg, out = reach()
    assert rc == N.FO_OK and (out.arrival == 0).all() and (out.dist == 0).all(), msg
    rc, msg, oc = _raw_clearance(torch, sm, cls, win, 30, None, x, x, head)
    assert rc == N.FO_OK and (oc.key == 0).all(), msg
    # the argument refusals of the road entry, under this entry's name
    rc, msg, out = _raw_reach(torch, sm, "fo_scene_hidden_reach_flow", cls, win, [2, 9, 8, 30], None, x, x, head)
    assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_reach_flow:") and "decreases" in msg and untouched_reach(out)
    # the flow clearance is a road metric
    for metric in (0, 2):
        rc, msg, oc = _raw_clearance(torch, sm, cls, win, 30, None, x, x, head, metric=metric)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_clearance_flow:") and f"metric = {metric}" in msg
        assert (oc.key == -7).all() and (oc.qmin == -7).all() and (oc.dist == 7777).all()
    # no table: FO_E_STATE, no output byte touched
    for drop in range(2):
        assert _set_moves(sm, None) == N.FO_OK
        rc, msg, out = reach()
        assert rc == N.FO_E_STATE and msg.startswith("fo_scene_hidden_reach_flow:") and "move table" in msg and untouched_reach(out)
        rc, msg, oc = _raw_clearance(torch, sm, cls, win, 30, None, x, x, head)
        assert rc == N.FO_E_STATE and msg.startswith("fo_scene_hidden_clearance_flow:") and "move table" in msg
        assert (oc.key == -7).all() and (oc.qmin == -7).all() and (oc.dist == 7777).all()
        # the road entry does not care
        rc, msg, out = _raw_reach(torch, sm, "fo_scene_hidden_reach_road", cls, win, r2, None, x, x, head)
        assert rc == N.FO_OK, msg
        if drop == 0:                                       # set again, served again; then dropped once more
            assert _set_moves(sm, np.full((rny, rnx), FREE, dtype=np.uint8)) == N.FO_OK
            assert reach()[0] == N.FO_OK
    # a map with two readers: the table cannot be replaced under the other reader's kernels
    other = N.Context(0)
    assert lib.fo_scene_share_map(other._h, sm.ctx._h) == N.FO_OK
    free = np.full((rny, rnx), FREE, dtype=np.uint8)
    for h in (sm.ctx._h, other._h):
        assert lib.fo_scene_set_lane_moves(h, free.ctypes.data) == N.FO_E_STATE
        assert lib.fo_scene_set_lane_moves(h, None) == N.FO_E_STATE
    assert "shared" in lib.fo_last_error(sm.ctx._h).decode()
    other.close()
    assert _set_moves(sm, free) == N.FO_OK and reach()[0] == N.FO_OK
    # no parameters, and a context without a map
    assert lib.fo_scene_hidden_reach_flow(sm.ctx._h, None, None) == N.FO_E_ARG
    assert lib.fo_scene_hidden_clearance_flow(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert lib.fo_scene_hidden_reach_flow(ctx._h, C.byref(N.HiddenReachRoad()), None) == N.FO_E_STATE
    assert lib.fo_scene_hidden_clearance_flow(ctx._h, C.byref(N.HiddenClearance()), None) == N.FO_E_STATE
    assert lib.fo_scene_set_lane_moves(ctx._h, free.ctypes.data) == N.FO_E_STATE
    assert N.load().fo_abi_version() == 12


def test_a_shared_map_brings_its_table(torch_cuda):
    """a second model that shares the first one's map takes over the host table and reads the device table"""
    torch = torch_cuda
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import SensorModel
    sc = T._scenario("scenario1")
    sm, obs = T._sensor(sc)
    sm2 = SensorModel(sc.lanelets, None, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, share_map_with=sm)
    assert sm2.lane_moves is sm.lane_moves
    ego, yaw = T._drive(torch, sm2, obs, sc, 1)
    traj = SY.make_trajectories(16, 31, DT, seed=1, ego_pos=ego, ego_yaw=yaw)
    out = sm2.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=VEH, v_max=13.9, dt=DT, metric="road", flow="lanes")
    cls, win, road, hid = T._state(torch, sm2)
    assert np.array_equal(_np(out.road_dist), RF.flow_distance(cls, win, road, sm.lane_moves, out.r2, hid)[0])


# ------------------------------------------------------------------------------------------------ the kernels of a call
_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import numpy as np, torch
import test_hidden_reach_gpu as T
from frenetix_occlusion import synthetic as SY
sc = T._scenario("scenario1")
sm, obs = T._sensor(sc, memory={{}})
ego, yaw = T._drive(torch, sm, obs, sc, 3)
traj = SY.make_trajectories(64, 31, 0.1, seed=1, ego_pos=ego, ego_yaw=yaw)
out = sm.hidden_reach(traj["x"], traj["y"], traj["theta"], vehicle=T.VEH, v_max=13.9, dt=0.1, metric="road", flow=sys.argv[1])
torch.cuda.synchronize()
print("child ok", int(out.reach[-1]))
'''


def _trace(tmp_path, flow):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_flow.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"),
                                         tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + flow)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), flow],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    reach = int(r.stdout.split("child ok")[1].split()[0])
    return "\n".join(open(f).read() for f in files).splitlines(), reach


def test_kernel_trace_of_the_two_flows(torch_cuda, tmp_path):
    """a drive with one road call launches none of the flow kernels; with one lanes call the flow bands the reach asks for in the
    place of the road bands, the road entry's merge, and the three kernels of the Euclidean call once each"""
    lines, reach = _trace(tmp_path, "any")
    count = lambda k: sum(k in line for line in lines)
    assert count("fo_hr_flow_") == 0
    assert count("fo_hr_road_band_kernel") == -(-reach // BAND) and count("fo_hr_road_arrival_kernel") == 1
    lines, reach = _trace(tmp_path, "lanes")
    assert count("fo_hr_road_band_kernel") == 0
    assert count("fo_hr_flow_band_kernel") == max(-(-reach // BAND), 1) == 6
    assert count("fo_hr_road_arrival_kernel") == 1
    assert count("fo_hr_rows_kernel") == 1 and count("fo_hr_cols_kernel") == 1 and count("fo_hr_traj_kernel") == 1
