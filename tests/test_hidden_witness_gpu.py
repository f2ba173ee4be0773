"""Hidden-traffic witnesses on the device (fo_scene_hidden_witness, DESIGN.md §5.10 "Witnesses") against the plain statement of
the definition (tests/ref_hidden_witness.py).  The maps the kernel walks are those the device's own road / flow forecast wrote (held
to their Dijkstra checkers by tests/test_hidden_reach_road_gpu.py and tests/test_hidden_reach_flow_gpu.py) or hand-made ones.
Every output is an exact integer: all comparisons are ``==``."""
import glob
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_witness as W
import test_hidden_reach_flow_gpu as FG
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DT, VEH, HL, HW, WB = T.DT, T.VEH, T.HL, T.HW, T.WB
_np = T._np
SEED = 20250611
FREE = 0xFF
OUTPUTS = ("cell", "src", "steps", "wdist", "dirs")


def cap_for(r2_last):
    return (W.min_path_cap(r2_last) + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw_witness(torch, sm, flow, win, r2, A, d, first, x, y, head, cap, hl=HL, hw=HW, wb=WB, drop=(), **over):
    """fo_scene_hidden_witness on maps and trajectories of the test's own; the output buffers are pre-filled with a pattern.
    ``drop``: names of pointers to hand over as NULL; ``over``: fields of the base structure or of the call to replace.
    Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    import ctypes as C
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    M, Tn = x.shape
    tx, ty, th = up(x, np.float64), up(y, np.float64), up(head, np.float64)
    dA, dd, df = up(A, np.uint8), up(np.asarray(d, dtype=np.uint16).view(np.int16), np.int16), up(first, np.int32)
    out = SimpleNamespace(cell=torch.full((M, 2), -7, dtype=torch.int32, device=dev), src=torch.full((M, 2), -7, dtype=torch.int32, device=dev),
                          steps=torch.full((M,), -7, dtype=torch.int32, device=dev), wdist=torch.full((M,), -7, dtype=torch.int32, device=dev),
                          dirs=torch.full((M, max(cap, 0)), 77, dtype=torch.uint8, device=dev))
    r2 = np.ascontiguousarray(r2, dtype=np.int32)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    base = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), hl=hl, hw=hw, wb=wb, J=len(r2),
                h_r2=r2.ctypes.data_as(C.POINTER(C.c_int32)), win_ix0=win[0], win_iy0=win[1], win_nx=win[2], win_ny=win[3],
                d_arrival=p(dA), d_first=p(df))
    call = dict(d_dist=p(dd), flow=int(flow), path_cap=int(cap), d_cell=p(out.cell), d_src=p(out.src), d_steps=p(out.steps),
                d_wdist=p(out.wdist), d_dirs=p(out.dirs))
    for k, v in over.items():
        (base if k in base or k in ("M", "T", "J") else call)[k] = v
    for k in drop:
        (base if k in base else call)[k] = None
    args = N.HiddenWitness(base=N.HiddenReach(**base), **call)
    rc = sm.ctx._lib.fo_scene_hidden_witness(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    return rc, msg, SimpleNamespace(**{k: _np(getattr(out, k)) for k in OUTPUTS})


def _untouched(out):
    return all((getattr(out, k) == (77 if k == "dirs" else -7)).all() for k in OUTPUTS)


def _same(out, ref, what):
    for k, r in zip(OUTPUTS, ref):
        got = getattr(out, k)
        assert got.dtype == r.dtype and got.shape == r.shape, (what, k)
        assert np.array_equal(got, r), (what, k, np.argwhere(got != r)[:4].tolist())


def _checker(sm, road, flow, moves, win, A, d, first, x, y, head, cap, hl=HL, hw=HW, wb=WB):
    return W.witnesses(A, d, win, road, first, sm.raster_origin, sm.cell_size, x, y, head, hl, hw, wb, cap, moves if flow else None)


def _parked():
    return FG._parked()


# ------------------------------------------------------------------------------------------------ 1. random cases
def random_cases(sm, rnx, rny):
    """every M of the 8-lane group's and the 32-trajectory workgroup's edges, both flows; windows of 40 x 30 .. 70 x 45 over every edge of
    the raster in turn, few sources (long walks) or many, a hidden mask in half of them, T in {1, 5, 31}, ragged lengths, poses that
    are NaN, a table per case"""
    rng = np.random.default_rng(SEED)
    for case, M in enumerate([1, 7, 8, 9, 31, 32, 33, 70] * 2):
        flow = case >= 8
        nx, ny = int(rng.integers(40, 71)), int(rng.integers(30, 46))
        corner = case % 5
        ix0 = [-nx // 2, rnx - (nx + 1) // 2, int(rng.integers(0, max(rnx - nx, 1))), int(rng.integers(0, max(rnx - nx, 1))),
               int(rng.integers(-nx + 1, rnx))][corner]
        iy0 = [int(rng.integers(-1, 3)), int(rng.integers(-1, 3)), -ny // 2, rny - (ny + 1) // 2, int(rng.integers(-ny + 1, rny))][corner]
        win = (ix0, iy0, nx, ny)
        sparse = case % 2 == 1
        cls = rng.choice(np.array([0, 1, 3, 5, 4, 2], dtype=np.uint8), (ny, nx),
                         p=[0.1, 0.004, 0.72, 0.003, 0.003, 0.17] if sparse else [0.12, 0.04, 0.6, 0.03, 0.03, 0.18])
        hidden = (rng.random((ny, nx)) < 0.004).astype(np.uint8) if case % 4 >= 2 else None
        Tn = [1, 5, 31][case % 3]
        h = int(rng.integers(18, 40)) if sparse else int(rng.integers(3, 14))
        top = int(rng.integers(h * h, (h + 1) * (h + 1)))
        r2 = np.sort(rng.integers(0, top + 1, Tn))
        r2[-1] = top
        x, y, head = T._random_poses(rng, sm, win, M, Tn)
        x[rng.random((M, Tn)) < 0.03] = np.nan
        lens = rng.integers(-1, Tn + 2, M).astype(np.int32) if case % 2 else None
        yield SimpleNamespace(case=case, M=M, flow=flow, win=win, cls=cls, hidden=hidden, r2=r2, x=x, y=y, head=head, lens=lens,
                              moves=FG.block_table(rng, rny, rnx))


def test_random_maps_windows_tables_and_poses(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    seen = dict(none=0, zero=0, now=0, walks=0, cells=0, longest=0, outside=0)
    for c in random_cases(sm, rnx, rny):
        assert FG._set_moves(sm, c.moves) == N.FO_OK
        entry = "fo_scene_hidden_reach_flow" if c.flow else "fo_scene_hidden_reach_road"
        rc, msg, maps = FG._raw_reach(torch, sm, entry, c.cls, c.win, c.r2, c.hidden, c.x, c.y, c.head, c.lens)
        assert rc == 0, msg
        cap = cap_for(c.r2[-1])
        rc, msg, out = _raw_witness(torch, sm, c.flow, c.win, c.r2, maps.arrival, maps.dist, maps.first, c.x, c.y, c.head, cap)
        assert rc == 0, msg
        ref = _checker(sm, road, c.flow, c.moves, c.win, maps.arrival, maps.dist, maps.first, c.x, c.y, c.head, cap)
        _same(out, ref, c.case)
        assert (out.steps >= -1).all()                          # never -2 on a forecast's own maps
        ix0, iy0, nx, ny = c.win
        walked = out.steps > 0
        seen["none"] += int((maps.first < 0).sum())
        seen["now"] += int((maps.first == 0).sum())
        seen["zero"] += int((out.steps == 0).sum())
        seen["walks"] += int(walked.sum())
        seen["cells"] += int(out.steps[walked].sum())
        seen["longest"] = max(seen["longest"], int(out.steps.max(initial=0)))
        s = out.src[out.steps >= 0]
        seen["outside"] += int(((s[:, 0] < ix0) | (s[:, 0] >= ix0 + nx) | (s[:, 1] < iy0) | (s[:, 1] >= iy0 + ny)).sum())
    print(seen)
    # not vacuous: trajectories without a finding, findings at sample 0, conflict cells that are sources, walks, long ones, and
    # walks that leave the window
    assert seen["none"] > 0 and seen["now"] > 10 and seen["zero"] > 10 and seen["walks"] > 30 and seen["longest"] >= 8 and seen["outside"] > 0


# ------------------------------------------------------------------------------------------------ 2. edges of the extension
def _pose_at(sm, gx, gy, Tn=2):
    """a trajectory whose rectangle's centre lies on the centre of raster cell (gx, gy) at its last sample, heading east, and far
    away before"""
    cs, (x0, y0) = sm.cell_size, sm.raster_origin
    x = np.full((1, Tn), 1e6)
    y = np.full((1, Tn), 1e6)
    x[0, -1], y[0, -1] = x0 + (gx + 0.5) * cs - WB, y0 + (gy + 0.5) * cs
    head = np.zeros((1, Tn, 2))
    head[..., 0] = 1.0
    return x, y, head


def test_edges_of_the_extension(torch_cuda):
    """(a) a conflict cell outside the window: raster road there is a source itself, no step; (b) the nearest source lies one cell
    outside the window: the walk leaves the window with its last step; (c) a source inside the window but off the raster"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    free = np.full((rny, rnx), FREE, dtype=np.uint8)
    assert FG._set_moves(sm, free) == N.FO_OK
    rows = np.flatnonzero(road.any(axis=1))
    cols = np.flatnonzero(road[rows[len(rows) // 2]])
    mid = int(rows[len(rows) // 2])
    assert len(rows) >= 8 and len(cols) >= 100 and cols[0] < 8 and cols[30] + 60 < rnx and road[mid, cols[0]:cols[30] + 60].all()
    r2 = [0, 30 * 30]
    cap = cap_for(r2[-1])
    # a window across the whole road, 40 columns wide: all of it seen and empty, so that every source lies outside it
    ix0 = int(cols[30])
    win = (ix0, int(rows[0]) - 3, 40, len(rows) + 6)
    cls = np.full((win[3], 40), 2, dtype=np.uint8)
    for wy in range(win[3]):
        if 0 <= win[1] + wy < rny:
            cls[wy] = np.where(road[win[1] + wy, ix0:ix0 + 40] != 0, 3, 2)
    for what, gx in (("a", ix0 + 40 + 12), ("b", ix0 + 40 - 7)):
        x, y, head = _pose_at(sm, gx, mid)
        rc, msg, maps = FG._raw_reach(torch, sm, "fo_scene_hidden_reach_road", cls, win, r2, None, x, y, head)
        assert rc == 0 and maps.first[0] == 1, (what, msg, maps.first)
        for flow in (0, 1):
            rc, msg, out = _raw_witness(torch, sm, flow, win, r2, maps.arrival, maps.dist, maps.first, x, y, head, cap)
            assert rc == 0, msg
            _same(out, _checker(sm, road, flow, free, win, maps.arrival, maps.dist, maps.first, x, y, head, cap), what)
            if what == "a":     # the footprint lies outside the window: its lowest, then leftmost cell, a source itself
                assert out.steps[0] == 0 and out.wdist[0] == 0 and out.cell[0, 0] >= ix0 + 40 and (out.cell[0] == out.src[0]).all()
            else:               # the rectangle's front is 2 cells from the window's edge: the source is the cell beyond the edge
                assert out.steps[0] >= 2 and out.src[0, 0] == ix0 + 40 and out.cell[0, 0] < ix0 + 40
                assert out.wdist[0] == 12 * (out.src[0, 0] - out.cell[0, 0]) and (out.dirs[0, :out.steps[0]] == 4).all()
    # (c) a window that hangs over the raster's left edge across the whole road; one source in it, off the raster
    win = (-6, int(rows[0]) - 3, 40, len(rows) + 6)
    cls = np.full((win[3], win[2]), 2, dtype=np.uint8)
    cls[mid - win[1] - 2:mid - win[1] + 3, :] = 3                # five rows of seen road, also off the raster
    cls[mid - win[1], 1] = 5                                     # raster cell (-5, mid)
    x, y, head = _pose_at(sm, 8, mid)
    rc, msg, maps = FG._raw_reach(torch, sm, "fo_scene_hidden_reach_road", cls, win, r2, None, x, y, head)
    assert rc == 0 and maps.first[0] == 1, (msg, maps.first)
    rc, msg, out = _raw_witness(torch, sm, 1, win, r2, maps.arrival, maps.dist, maps.first, x, y, head, cap)
    assert rc == 0, msg
    _same(out, _checker(sm, road, 1, free, win, maps.arrival, maps.dist, maps.first, x, y, head, cap), "c")
    assert tuple(out.src[0]) == (-5, mid) and out.steps[0] > 5 and out.cell[0, 0] > 0


# ------------------------------------------------------------------------------------------------ 3 + 5. hand-made maps
def _corridors(n=40):
    """a window of n x n cells over raster that is not road (tests/test_hidden_reach_flow_gpu._two_streets): up column 0 from the
    only source at its foot, NE and SE through the gap at the top of the wall in column 1, down column 2.  The distance map is
    written out by hand"""
    sm, road = FG._two_streets()
    win = (30, 40, n, n)
    assert not road[win[1] - 1:win[1] + n + 1, win[0] - 1:win[0] + n + 1].any()
    d = np.full((n, n), 65535, dtype=np.uint16)
    d[:n - 1, 0] = 12 * np.arange(n - 1)
    d[n - 1, 0] = 12 * (n - 1)
    d[n - 1, 1] = 12 * (n - 2) + 17
    d[:n - 1, 2] = 12 * (n - 2) + 34 + 12 * np.arange(n - 1)[::-1]
    d[n - 1, 2] = d[n - 1, 1] + 12
    return sm, road, win, d


def _corridor_poses(sm, win, cells):
    """a trajectory of two samples per cell, its second sample a rectangle of a fifth of a cell on the cell's centre"""
    cs, (x0, y0) = sm.cell_size, sm.raster_origin
    M = len(cells)
    x, y = np.full((M, 2), 1e6), np.full((M, 2), 1e6)
    for m, (cx, cy) in enumerate(cells):
        x[m, 1], y[m, 1] = x0 + (win[0] + cx + 0.5) * cs, y0 + (win[1] + cy + 0.5) * cs
    head = np.zeros((M, 2, 2))
    head[..., 0] = 1.0
    return x, y, head


def test_walk_of_exactly_path_cap_steps_and_padding(torch_cuda):
    """R2 = 2379: L = 634 = 12 * 50 + 2 * 17 and L // 12 = 52, a multiple of 4 -- the walk from (2, 26) takes 12 + 2 + 38 = 52
    steps, exactly the smallest path_cap; four more bytes of row are padding"""
    torch = torch_cuda
    sm, road, win, d = _corridors()
    r2 = [0, 2379]
    assert W.min_path_cap(r2[-1]) == 52 and d[26, 2] == 634
    A = np.where(d <= 634, 1, 255).astype(np.uint8)
    A[0, 0] = 0
    x, y, head = _corridor_poses(sm, win, [(2, 26), (0, 0), (2, 27), (0, 39)])
    first = np.array([1, 1, 1, 1], dtype=np.int32)
    travel = [2] * 38 + [1, 7] + [6] * 12
    for cap in (52, 56):
        for flow in (0, 1):          # (the model's own table: every cell of this window lies in no lanelet, 0xFF)
            rc, msg, out = _raw_witness(torch, sm, flow, win, r2, A, d, first, x, y, head, cap, hl=0.05, hw=0.05, wb=0.0)
            assert rc == 0, msg
            _same(out, _checker(sm, road, flow, sm.lane_moves, win, A, d, first, x, y, head, cap, 0.05, 0.05, 0.0), (cap, flow))
            assert out.steps.tolist() == [52, 0, 51, 39] and out.wdist.tolist() == [634, 0, 622, 468]
            assert (out.src == np.array([win[0], win[1]])).all()
            assert out.dirs[0].tolist() == travel[::-1] + [255] * (cap - 52)
            assert out.dirs[1].tolist() == [255] * cap and out.dirs[2].tolist() == travel[::-1][1:] + [255] * (cap - 51)
            assert out.dirs[3].tolist() == [2] * 39 + [255] * (cap - 39)


def test_maps_that_are_no_forecasts_stop_the_walk(torch_cuda):
    """A bounded loop by construction: the walk takes at most path_cap rounds whatever ``d`` holds, and every cell it reads was
    tested against the window and the raster first -- nothing here can fault, hang or read outside the maps.  (a) a ``d`` map
    edited on the host so that one corridor cell has no predecessor: the walks through it stop there with steps = -2, the rows
    of the others stay as they were; (b) a corridor whose distances run on beyond L: the row fills up, steps = -2 at the cell
    the walk stands on after path_cap steps"""
    torch = torch_cuda
    sm, road, win, d = _corridors()
    r2 = [0, 2379]
    A = np.where(d != 65535, 1, 255).astype(np.uint8)
    cells = [(2, 26), (0, 10), (0, 21), (0, 20), (2, 38)]
    x, y, head = _corridor_poses(sm, win, cells)
    first = np.array([1, 1, 1, 1, -1], dtype=np.int32)
    kw = dict(hl=0.05, hw=0.05, wb=0.0)
    rc, msg, before = _raw_witness(torch, sm, 0, win, r2, A, d, first, x, y, head, 52, **kw)
    assert rc == 0 and before.steps.tolist() == [52, 10, 21, 20, -1], msg
    e = d.copy()
    e[20, 0] += 1                                                # (0, 21) loses its only predecessor, and (0, 20) its own
    rc, msg, out = _raw_witness(torch, sm, 0, win, r2, A, e, first, x, y, head, 52, **kw)
    assert rc == 0, msg
    _same(out, _checker(sm, road, 0, None, win, A, e, first, x, y, head, 52, 0.05, 0.05, 0.0), "edited")
    assert out.steps.tolist() == [-2, 10, -2, -2, -1]
    assert out.src.tolist() == [[win[0], win[1] + 21], [win[0], win[1]], [win[0], win[1] + 21], [win[0], win[1] + 20], [W.NO_CELL] * 2]
    assert out.dirs[0].tolist() == before.dirs[0, :31].tolist() + [255] * 21 and (out.dirs[2:] == 255).all()
    for k in OUTPUTS:
        assert np.array_equal(getattr(out, k)[[1, 4]], getattr(before, k)[[1, 4]]), k
    assert out.wdist.tolist() == [634, 120, 252, 241, -1] and np.array_equal(out.cell, before.cell)
    # (b) R2 = 1600: L = 520, path_cap = 44 >= 43; the corridor's distances go on to 634
    r2 = [0, 1600]
    assert cap_for(r2[-1]) == 44
    rc, msg, out = _raw_witness(torch, sm, 0, win, r2, A, d, first, x, y, head, 44, **kw)
    assert rc == 0, msg
    _same(out, _checker(sm, road, 0, None, win, A, d, first, x, y, head, 44, 0.05, 0.05, 0.0), "beyond L")
    assert out.steps.tolist() == [-2, 10, 21, 20, -1] and (out.dirs[0] == before.dirs[0, :44]).all()
    assert out.src[0].tolist() == [win[0], win[1] + 8]           # 52 - 44 steps short of the source


# ------------------------------------------------------------------------------------------------ 4. the free table
def test_free_table_flow_equals_road(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = _parked()
    rny, rnx = road.shape
    assert FG._set_moves(sm, np.full((rny, rnx), FREE, dtype=np.uint8)) == N.FO_OK
    walks = 0
    for c in random_cases(sm, rnx, rny):
        if c.case not in (1, 3, 4, 7):
            continue
        rc, msg, maps = FG._raw_reach(torch, sm, "fo_scene_hidden_reach_road", c.cls, c.win, c.r2, c.hidden, c.x, c.y, c.head, c.lens)
        assert rc == 0, msg
        cap = cap_for(c.r2[-1])
        got = [_raw_witness(torch, sm, flow, c.win, c.r2, maps.arrival, maps.dist, maps.first, c.x, c.y, c.head, cap) for flow in (0, 1)]
        assert got[0][0] == got[1][0] == 0
        for k in OUTPUTS:
            assert np.array_equal(getattr(got[0][2], k), getattr(got[1][2], k)), (c.case, k)
        walks += int((got[0][2].steps > 0).sum())
    assert walks > 20


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    import ctypes as C
    sm, road = _parked()
    lib = sm.ctx._lib
    win = (3, 1, 12, 9)
    A, d = np.zeros((9, 12), dtype=np.uint8), np.zeros((9, 12), dtype=np.uint16)
    x = np.zeros((2, 4))
    head = np.zeros((2, 4, 2))
    head[..., 0] = 1.0
    first = np.zeros(2, dtype=np.int32)
    r2 = [2, 2, 8, 2379]

    def call(flow=0, cap=52, table=r2, **kw):
        return _raw_witness(torch, sm, flow, win, table, A, d, first, x, x, head, cap, **kw)

    rc, msg, out = call()
    assert rc == N.FO_OK and (out.steps >= 0).all(), msg
    nan = float("nan")
    ext = N.HIDDEN_REACH_MAX_HALF_EXTENT * sm.cell_size
    refused = [
        (dict(flow=2), "flow = 2"), (dict(flow=-1), "flow = -1"),
        (dict(cap=48), "path_cap = 48"), (dict(cap=54), "path_cap = 54"), (dict(cap=-4), "path_cap = -4"),
        (dict(table=[2, 9, 8, 30]), "decreases"), (dict(table=[-1, 2, 8, 30]), "negative"),
        (dict(table=[0, (N.HIDDEN_REACH_MAX_HALO + 1) ** 2], cap=N.HIDDEN_WITNESS_MAX_STEPS), "FO_HIDDEN_REACH_MAX_HALO"),
        (dict(J=0), "J = 0"), (dict(J=255), "J = 255"), (dict(drop=("h_r2",)), "h_r2"),
        (dict(M=-1), "M = -1"), (dict(T=0), "T = 0"), (dict(T=5), "T = 5"),
        (dict(drop=("d_arrival",)), "d_arrival"), (dict(drop=("d_dist",)), "d_dist"),
        (dict(drop=("d_x",)), "d_x"), (dict(drop=("d_y",)), "d_x"), (dict(drop=("d_heading",)), "d_heading"),
        (dict(drop=("d_first",)), "d_first"),
        (dict(drop=("d_cell",)), "d_cell"), (dict(drop=("d_src",)), "d_src"), (dict(drop=("d_steps",)), "d_steps"),
        (dict(drop=("d_wdist",)), "d_wdist"), (dict(drop=("d_dirs",)), "d_dirs"),
        (dict(win_nx=0), "window"), (dict(win_ny=40000), "window"),
        (dict(hl=-0.1), "half extents"), (dict(hw=nan), "half extents"), (dict(wb=ext * 1.01), "half extents"),
    ]
    for kw, text in refused:
        rc, msg, out = call(**kw)
        assert rc == N.FO_E_ARG and msg.startswith("fo_scene_hidden_witness:") and text in msg, (kw, rc, msg)
        assert _untouched(out), kw
    # M = 0: fine, and nothing is written
    e = np.zeros((0, 4))
    rc, msg, out = _raw_witness(torch, sm, 0, win, r2, A, d, first[:0], e, e, np.zeros((0, 4, 2)), 52)
    assert rc == N.FO_OK, msg
    # the lanes without a table: FO_E_STATE; the road walk does not care
    assert FG._set_moves(sm, None) == N.FO_OK
    rc, msg, out = call(flow=1)
    assert rc == N.FO_E_STATE and msg.startswith("fo_scene_hidden_witness:") and "move table" in msg and _untouched(out)
    assert call(flow=0)[0] == N.FO_OK
    # no parameters, and a context without a map
    assert lib.fo_scene_hidden_witness(sm.ctx._h, None, None) == N.FO_E_ARG
    ctx = N.Context(0)
    assert lib.fo_scene_hidden_witness(ctx._h, C.byref(N.HiddenWitness()), None) == N.FO_E_STATE
    assert N.load().fo_abi_version() == 12 and N.HIDDEN_WITNESS_MAX_STEPS == 276


# ------------------------------------------------------------------------------------------------ 7. through the interface
def _interface(tmp_path, sc, memory=True):
    import yaml
    from frenetix_occlusion import interface, synthetic as SY
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    acc = cfg["accelerator"]
    acc["spawn"]["mode"] = "cells"
    if memory:
        acc["occlusion_memory"]["enabled"], acc["occlusion_memory_metric"], acc["occlusion_memory_vehicles"] = True, "road", "lanes"
    cfg["sensor_model"]["sensor_radius"], cfg["sensor_model"]["sensor_angle"] = 50.0, 360.0
    p = tmp_path / "occ.yaml"
    p.write_text(yaml.safe_dump(cfg))
    ego = np.asarray(sc.ego_initial, dtype=np.float64)
    path = ego[None, :2] + np.linspace(0.0, 80.0, 81)[:, None] * np.array([[math.cos(ego[2]), math.sin(ego[2])]])
    veh = SimpleNamespace(**dict(zip(("length", "width", "wb_rear_axle", "mass", "a_max"), SY.VEHICLE_BMW320I)))
    return interface.FOInterface(sc, path, veh, DT, config_path=str(p))


def _drive(fo, sc, steps, first=0):
    ego0 = np.asarray(sc.ego_initial, dtype=np.float64)
    yaw = float(ego0[2])
    for step in range(first, first + steps):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        fo.evaluate_scenario({}, ego, yaw, (0.7634 * step, 0.0), float(ego0[3]), step, None)
    return ego, yaw


def test_witness_agents_through_the_interface(torch_cuda, tmp_path):
    """scenario 1, the occlusion memory on with its vehicle layer: the witnesses of a 64-candidate fan become phantom agents, each
    is under its representative candidate's footprint at the sample the forecast named (DCE <= 1e-3, the rounding step of the
    sweep's DCE), the device batch's own slots cost what they cost without the call, and the next step has dropped the agents"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.sensor_model import HiddenWitness
    sc = T._scenario("scenario1")
    fo = _interface(tmp_path, sc)
    ego, yaw = _drive(fo, sc, 3)
    sm, am = fo.sensor_model, fo.agent_manager
    assert sm.occlusion_memory_vehicles == "lanes"
    traj = SY.make_trajectories(64, 31, DT, seed=SEED, ego_pos=ego, ego_yaw=yaw)
    plain = fo.trajectory_safety_assessment_batch(traj, mode="full")
    nb = am.n_slots()
    assert plain is not None and nb > 0 and not am._manual
    pf0, pi0 = _np(plain.result.pair_f), _np(plain.result.pair_i)
    cost0 = _np(plain.cost)
    with pytest.raises(TypeError):
        fo.hidden_witness(traj, metric="euclid")                 # the Euclidean metric has no route and is not offered
    w = fo.hidden_witness(traj, v_max=13.9, flow="lanes")
    assert isinstance(w, HiddenWitness) and w.reach.metric == "road" and w.reach.flow == "lanes" and w.reach.from_vehicle_memory
    assert w.path_cap == cap_for(w.reach.r2[-1]) and w.path_cap % 4 == 0 and tuple(w.dirs.shape) == (64, w.path_cap)
    # the device's rows are the checker's on the device's own maps
    cls, win, road, _ = T._state(torch, sm)
    x, y = np.asarray(traj["x"]), np.asarray(traj["y"])
    ref = W.witnesses(_np(w.reach.arrival), _np(w.reach.road_dist), win, road, _np(w.reach.first), sm.raster_origin, sm.cell_size, x, y,
                      _np(w.reach.heading), HL, HW, WB, w.path_cap, sm.lane_moves)
    _same(SimpleNamespace(cell=_np(w.cell), src=_np(w.source), steps=_np(w.steps), wdist=_np(w.dist), dirs=_np(w.dirs)), ref, "interface")
    picked = w.select(max_agents=8, merge_cells=4)
    assert picked, "no candidate of the fan meets hidden traffic"
    agents = fo.add_witness_agents(w, max_agents=8, merge_cells=4)
    assert len(agents) == len(picked) and am._manual == agents and am.n_slots() == nb + len(agents)
    full = fo.trajectory_safety_assessment_batch(traj, mode="full")
    pf, pi = _np(full.result.pair_f), _np(full.result.pair_i)
    assert pf.shape[1] == nb + len(agents)
    for i, m in enumerate(picked):
        dce = float(pf[N.PF["dce"], nb + i, m])
        print(f"agent {i}: candidate {m}, k* = {int(w.reach.first[m])}, {int(w.steps[m])} steps, {w.speed(m):.2f} m/s, DCE {dce:.3g}")
        assert dce <= 1e-3, (i, m, dce)
    assert np.array_equal(pf[:, :nb], pf0, equal_nan=True) and np.array_equal(pi[:, :nb], pi0)
    assert (_np(full.cost)[:, N.COST["min_dce"]] <= cost0[:, N.COST["min_dce"]]).all()
    _drive(fo, sc, 1, first=3)
    assert not am._manual and am.n_slots() == am._batch.pos.shape[0]


# ------------------------------------------------------------------------------------------------ 8. the kernels of a drive
_TRACE_CHILD = '''
import hashlib, pathlib, sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import numpy as np, torch
import test_hidden_reach_gpu as T
import test_hidden_witness_gpu as WG
from frenetix_occlusion import synthetic as SY
sc = T._scenario("scenario1")
fo = WG._interface(pathlib.Path(sys.argv[2]), sc)
h = hashlib.sha256()
for step in range(3):
    ego, yaw = WG._drive(fo, sc, 1, first=step)
    traj = SY.make_trajectories(64, 31, 0.1, seed=1, ego_pos=ego, ego_yaw=yaw)
    if sys.argv[1] == "witness":
        out = fo.hidden_witness(traj, v_max=13.9, flow="lanes").reach
    else:
        out = fo.hidden_reach(traj, v_max=13.9, metric="road", flow="lanes")
    ba = fo.trajectory_safety_assessment_batch(traj)
    torch.cuda.synchronize()
    parts = [fo.sensor_model.cell_class, fo.sensor_model.occlusion_memory_hidden, fo.sensor_model.occlusion_memory_hidden_vehicles,
             ba.cost if ba is not None else np.zeros(1), out.first, out.arrival, np.array([sp.position for sp in fo.spawn_points], dtype=np.float64)]
    for p in parts:
        h.update(np.ascontiguousarray(p.cpu().numpy() if torch.is_tensor(p) else p).tobytes())
print("child ok", h.hexdigest())
'''


def _trace(tmp_path, what):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_witness.py"
    child.write_text(_TRACE_CHILD.format(root=T.ROOT, pkg=os.path.join(T.ROOT, "frenetix-occlusion_amd"), tests=os.path.join(T.ROOT, "tests")))
    d = tmp_path / ("trace_" + what)
    cfg = tmp_path / ("cfg_" + what)
    cfg.mkdir()
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), what, str(cfg)],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    return "\n".join(open(f).read() for f in files).splitlines(), r.stdout.split("child ok")[1].split()[0]


def test_kernel_trace_one_launch_per_call_and_nothing_else_changes(torch_cuda, tmp_path):
    """three steps of a drive with one forecast each: with ``hidden_reach(metric="road")`` no witness kernel is launched, with
    ``hidden_witness`` exactly one per call; class bytes, H_k, V_k, spawn points, costs and the forecast are the same bits"""
    lines, digest_reach = _trace(tmp_path, "reach")
    count = lambda k: sum(k in line for line in lines)
    assert count("fo_hr_witness") == 0 and count("fo_hr_traj_kernel") == 3
    lines, digest_witness = _trace(tmp_path, "witness")
    assert count("fo_hr_witness_kernel") == 3 and count("fo_hr_traj_kernel") == 3
    assert digest_witness == digest_reach
