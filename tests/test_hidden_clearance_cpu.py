"""Hidden-traffic clearance (DESIGN.md §5.10 "Clearance and critical speed") without a GPU and without the library: the
checker (tests/ref_hidden_clearance.py) tied to the two reach checkers on random maps, cases worked out by hand, the critical
speed's bracket, and the Python layer's own arithmetic (``HiddenClearance.reach`` / ``.critical_speed`` on CPU tensors) and
argument checks.  Every comparison is an exact integer equality unless it says otherwise."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_clearance as HC
import ref_hidden_reach as HR
import ref_hidden_reach_road as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "frenetix-occlusion_amd")
DT = 0.1
HL, HW, WB = 2.254, 0.805, 1.4227
V_TABLES = (2.0, 7.0, 13.9)            # a pedestrian, a cyclist, the cap
V_CAP = V_TABLES[-1]


def _product():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    torch = pytest.importorskip("torch")
    from frenetix_occlusion import sensor_model
    return torch, sensor_model


def _random_case(rng, case, sparse=False):
    """a raster with road and blocks of non-road, a window of 12-40 cells a side that lies inside the raster, touches its edge or
    runs off it, class bytes consistent with the raster inside it, a hidden mask in every second case, ragged poses"""
    cs = [1.0, 0.5, 2.0][case % 3]
    rnx, rny = int(rng.integers(30, 60)), int(rng.integers(30, 60))
    road = np.ones((rny, rnx), dtype=np.uint8)
    for _ in range(int(rng.integers(2, 7))):                              # building blocks
        bx, by = int(rng.integers(0, rnx - 4)), int(rng.integers(0, rny - 4))
        road[by:by + int(rng.integers(3, 14)), bx:bx + int(rng.integers(3, 14))] = 0
    nx, ny = int(rng.integers(12, 41)), int(rng.integers(12, 41))
    place = case % 4                                                      # inside, touching an edge, off the raster, anywhere
    if sparse:                      # the window is the raster: nothing outside it is a source
        ix0, iy0, nx, ny = 0, 0, rnx, rny
    elif place == 0:
        ix0, iy0 = int(rng.integers(1, max(rnx - nx, 2))), int(rng.integers(1, max(rny - ny, 2)))
    elif place == 1:
        ix0, iy0 = (0 if case % 8 < 4 else rnx - nx), int(rng.integers(0, max(rny - ny, 1)))
    elif place == 2:
        ix0, iy0 = int(rng.integers(-nx // 2, 0)), rny - ny // 2
    else:
        ix0, iy0 = int(rng.integers(-nx + 1, rnx)), int(rng.integers(-ny + 1, rny))
    win = (ix0, iy0, nx, ny)
    QX, QY = np.meshgrid(np.arange(ix0, ix0 + nx), np.arange(iy0, iy0 + ny))
    on = (QX >= 0) & (QX < rnx) & (QY >= 0) & (QY < rny)
    is_road = np.zeros((ny, nx), dtype=bool)
    is_road[on] = road[QY[on], QX[on]] != 0
    vis = rng.random((ny, nx)) < (0.97 if sparse else 0.8)
    occ = ~vis & (rng.random((ny, nx)) < 0.5)
    cls = (is_road * 1 + vis * 2 + occ * 4).astype(np.uint8)
    hidden = None
    if case % 2 or sparse:          # (sparse: six to twelve sources, so that few poses stand on one)
        hidden = (rng.random((ny, nx)) < 0.02).astype(np.uint8)
        if sparse:
            hidden[:] = 0
            hidden.ravel()[rng.integers(0, nx * ny, int(rng.integers(6, 13)))] = 1
    T = [1, 5, 31][case % 3]
    M = 6
    origin = (-3.0, 2.5)
    x = origin[0] + (ix0 + rng.uniform(-4, nx + 4, (M, 1)) + np.cumsum(rng.uniform(-1.5, 1.5, (M, T)), axis=1)) * cs
    y = origin[1] + (iy0 + rng.uniform(-4, ny + 4, (M, 1)) + np.cumsum(rng.uniform(-1.5, 1.5, (M, T)), axis=1)) * cs
    th = rng.uniform(-math.pi, math.pi, (M, T))
    head = np.stack((np.cos(th), np.sin(th)), -1)
    lens = rng.integers(0, T + 2, M).astype(np.int32) if case % 2 else None
    return SimpleNamespace(cs=cs, road=road, win=win, cls=cls, hidden=hidden, T=T, origin=origin, x=x, y=y, head=head, lens=lens)


def _reference_reach(c, metric, r2):
    if metric == "road":
        A = RR.arrival_map_road(c.cls, c.win, c.road, r2, c.hidden)[0]
    else:
        A = HR.arrival_map(c.cls, c.win, c.road, r2, c.hidden)[0]
    return HR.trajectories(A, c.win, c.road, c.origin, c.cs, c.x, c.y, c.head, HL, HW, WB, c.lens)


# ------------------------------------------------------------------------------------------------ 1. the tie
def test_tie_to_the_reach_forecast_on_random_cases():
    """60 random cases, both metrics, three tables under one cap: what qmin says of cells > 0, first and slack is what the reach
    checkers compute from their arrival maps; the product's HiddenClearance.reach (torch, CPU tensors) says the same"""
    torch, SM = _product()
    rng = np.random.default_rng(20240611)
    seen = dict(hit=0, miss=0, off=0, edge=0, hidden=0, ragged=0, differs=0, T=set())
    for case in range(60):
        c = _random_case(rng, case)
        margin = math.sqrt(2.0) * c.cs
        ix0, iy0, nx, ny = c.win
        rny, rnx = c.road.shape
        seen["off"] += ix0 < 0 or iy0 < 0 or ix0 + nx > rnx or iy0 + ny > rny
        seen["edge"] += ix0 == 0 or ix0 + nx == rnx
        seen["hidden"] += c.hidden is not None
        seen["ragged"] += c.lens is not None
        seen["T"].add(c.T)
        tables = [HR.reach_table(v, DT, margin, c.cs, c.T) for v in V_TABLES]
        r2_cap = int(tables[-1][-1])
        keys = {}
        for metric in ("euclid", "road"):
            key, D2, d = HC.key_map(c.cls, c.win, c.road, r2_cap, metric, c.hidden)
            keys[metric] = key
            qmin = HC.clearance(key, c.win, c.road, c.origin, c.cs, c.x, c.y, c.head, HL, HW, WB, c.lens)
            if c.lens is not None:
                for m in range(len(c.lens)):
                    assert (qmin[m, max(int(c.lens[m]), 0):] == HC.NONE).all()
            out = SM.HiddenClearance(torch.as_tensor(key.astype(np.int32)), torch.as_tensor(qmin.astype(np.int32)), None, None,
                                     None, r2_cap, metric, DT, margin, c.cs)
            for v, r2 in zip(V_TABLES, tables):
                cells, first, slack = _reference_reach(c, metric, r2)
                hit, f, s = HC.reach_from_qmin(qmin, r2)
                assert np.array_equal(hit, cells > 0), (case, metric, v)
                assert np.array_equal(f, first) and np.array_equal(s, slack), (case, metric, v)
                ph, pf, ps = out.reach(v)
                assert ph.dtype == torch.bool and pf.dtype == torch.int32 and ps.dtype == torch.int32
                assert np.array_equal(ph.numpy(), hit) and np.array_equal(pf.numpy(), first) and np.array_equal(ps.numpy(), slack)
                seen["hit"] += int((first >= 0).sum())
                seen["miss"] += int((first < 0).sum())
        assert (keys["road"] >= keys["euclid"]).all()
        seen["differs"] += int((keys["road"] > keys["euclid"]).sum())
    assert seen["hit"] > 100 and seen["miss"] > 100 and seen["off"] >= 15 and seen["edge"] >= 10
    assert seen["hidden"] == 30 and seen["ragged"] == 30 and seen["T"] == {1, 5, 31} and seen["differs"] > 0


# ------------------------------------------------------------------------------------------------ 2. by hand
def _corridor():
    """a 20 x 9 raster = window: a corridor of road in the rows 3 .. 5, everything visible but one occluded road cell at (4, 4)"""
    road = np.zeros((9, 20), dtype=np.uint8)
    road[3:6] = 1
    cls = np.where(road != 0, 3, 2).astype(np.uint8)
    cls[4, 4] = 5
    return cls, (0, 0, 20, 9), road


def test_known_key_of_one_source_in_a_corridor():
    cls, win, road = _corridor()
    key, D2, _ = HC.key_map(cls, win, road, 100)                # h = 10: D2 = 100 is the cell (14, 4)
    for gy in range(9):
        for gx in range(20):
            d2 = (gx - 4) ** 2 + (gy - 4) ** 2
            want = 169 * d2 if road[gy, gx] and d2 <= 100 else HC.NONE
            assert key[gy, gx] == want, (gx, gy)
    assert key[4, 4] == 0 and key[4, 14] == 169 * 100           # D2 = r2_cap is kept (<=) ...
    assert key[3, 14] == HC.NONE and key[4, 15] == HC.NONE      # ... 101 and 121 are not
    assert (key[:3] == HC.NONE).all() and (key[6:] == HC.NONE).all()      # not road: NONE, however near
    assert D2[2, 4] == 4
    # open corridor: the lattice path to the source is passable, d^2 <= 169 D2 everywhere, the road key is the same
    key_r, _, d = HC.key_map(cls, win, road, 100, "road")
    assert np.array_equal(key_r, key) and d[4, 14] == 120 and d[3, 13] == 12 * 9 + 5


def test_known_key_behind_a_wall_with_a_gap():
    """the 12 x 12 open field of the road checker's wall test: source (5, 5), a wall in column 7 with a gap at row 0"""
    n = 12
    road = np.ones((n, n), dtype=np.uint8)
    cls = np.full((n, n), 3, dtype=np.uint8)
    cls[5, 5] = 5
    cls[:, 7], road[:, 7] = 2, 0
    cls[0, 7], road[0, 7] = 3, 1
    win = (0, 0, n, n)
    cap = 400
    key, _, d = HC.key_map(cls, win, road, cap, "road")
    ke, _, _ = HC.key_map(cls, win, road, cap, "euclid")
    assert math.isqrt(169 * cap) == 260
    assert d[5, 8] == 135 and ke[5, 8] == 169 * 9 and key[5, 8] == 135 ** 2            # round the wall: d^2 > 169 D2
    assert d[1, 8] == 87 and ke[1, 8] == 169 * 25 and key[1, 8] == 87 ** 2
    assert d[5, 6] == 12 and key[5, 6] == 169 == ke[5, 6]                              # before the wall: 144 < 169, the maximum flips
    assert d[0, 7] == 70 and ke[0, 7] == 169 * 29 == key[0, 7]                           # in the gap: 70^2 = 4900 < 4901, Euclid by one
    assert d[11, 8] == 207 and key[11, 8] == 207 ** 2
    assert (key[1:, 7] == HC.NONE).all()                                               # the wall itself is not road
    assert ((key >= ke) | (key == HC.NONE)).all()
    # a cap that keeps D2 but not d: Lcap = isqrt(169 * 45) = 87 keeps (8, 1) with d = 87 and drops (8, 5) with d = 135
    key, _, d = HC.key_map(cls, win, road, 45, "road")
    assert math.isqrt(169 * 45) == 87 and key[1, 8] == 87 ** 2 and key[5, 8] == HC.NONE and d[5, 8] == RR.NONE
    assert HC.key_map(cls, win, road, 45, "euclid")[0][5, 8] == 169 * 9
    # closed wall: behind it nothing is reachable
    cls[0, 7], road[0, 7] = 2, 0
    key, _, _ = HC.key_map(cls, win, road, cap, "road")
    assert (key[:, 8:] == HC.NONE).all()


def test_known_clearance_of_poses():
    cls, win, road = _corridor()
    key, _, _ = HC.key_map(cls, win, road, 100)
    cs, origin = 1.0, (0.0, 0.0)
    # a 2 x 1 cell rectangle (hl = 1, hw = 0.5, no wheelbase) centred on the cell centre (gx + 0.5, 4.5): covers columns gx - 1 .. gx + 1
    x = np.array([[8.5, 5.5, 30.5], [8.5, 8.5, 8.5]])
    y = np.array([[4.5, 4.5, 4.5], [1.5, 7.5, 100.5]])           # the second row of poses: no road cell under the footprint
    head = np.zeros((2, 3, 2))
    head[..., 0] = 1.0
    q = HC.clearance(key, win, road, origin, cs, x, y, head, 1.0, 0.5, 0.0)
    assert q[0].tolist() == [169 * 9, 0, HC.NONE]                # nearest column 7 -> D2 = 9; over the source; off the raster
    assert (q[1] == HC.NONE).all()
    assert HC.clearance(key, win, road, origin, cs, x, y, head, 1.0, 0.5, 0.0, lens=[1, 0])[0].tolist() == [169 * 9, HC.NONE, HC.NONE]
    # outside the window a raster road cell counts as key 0: a window that ends at column 9 leaves (10, 4) outside
    win2 = (0, 0, 10, 9)
    key2, _, _ = HC.key_map(cls[:, :10], win2, road, 100)
    x2, y2 = np.array([[11.5]]), np.array([[4.5]])
    assert HC.clearance(key2, win2, road, origin, cs, x2, y2, head[:1, :1], 1.0, 0.5, 0.0)[0, 0] == 0
    hit, first, slack = HC.reach_from_qmin(q[:1], [0, 4, 9])
    assert hit.tolist() == [[False, True, False]] and first.tolist() == [1] and slack.tolist() == [-1]


# ------------------------------------------------------------------------------------------------ 3. the critical speed
def test_critical_speed_brackets_the_forecast():
    """euclid: the forecast at v_crit (1 + 1e-9) hits, at v_crit (1 - 1e-9) it does not (a float64 formula whose rounding is
    around 1e-15); road: no hit just below v_crit, and v_crit_road >= v_crit_euclid.
    v_crit = 0 has no lower side.  margin = 0.3 cells makes floor(margin^2 / cs^2) = 0, so v_crit = 0 arises only where a footprint
    covers a source cell itself (D2 = 0); no choice of margin and dt removes that, since random poses may stand on a source.  The
    sources are therefore sparse (6 to 12 cells, the window is the whole raster), every pose with 0 < v_crit is bracketed --
    more than 100 of them are asked for -- and the few poses that do stand on a source are not dropped but checked for what
    v_crit = 0 claims: the forecast hits at v_max = 0."""
    torch, SM = _product()
    rng = np.random.default_rng(77)
    n_bracket, n_zero, n_inf, n_above, n_road_later = 0, 0, 0, 0, 0
    for case in range(60):
        c = _random_case(rng, case, sparse=True)
        margin = 0.3 * c.cs
        r2_cap = int(HR.reach_table(V_CAP, DT, margin, c.cs, c.T)[-1])
        vc = {}
        for metric in ("euclid", "road"):
            key, _, _ = HC.key_map(c.cls, c.win, c.road, r2_cap, metric, c.hidden)
            qmin = HC.clearance(key, c.win, c.road, c.origin, c.cs, c.x, c.y, c.head, HL, HW, WB, c.lens)
            v = HC.critical_speed(qmin, c.cs, DT, margin)
            out = SM.HiddenClearance(None, torch.as_tensor(qmin.astype(np.int32)), None, None, None, r2_cap, metric, DT, margin, c.cs)
            pv = out.critical_speed()
            # the same float64 formula; torch may divide by multiplying with a reciprocal: a few ulp, against the bracket's 1e-9
            assert pv.dtype == torch.float64 and np.array_equal(np.isinf(pv.numpy()), np.isinf(v))
            assert np.allclose(pv.numpy(), v, rtol=1e-14, atol=0.0)
            vc[metric] = v
            for m in range(len(v)):
                q = qmin[m:m + 1]
                hits = lambda vm: HC.reach_from_qmin(q, HR.reach_table(vm, DT, margin, c.cs, c.T))[1][0] >= 0
                if np.isinf(v[m]):
                    assert (q == HC.NONE).all() or c.T == 1 or not hits(V_CAP)
                    n_inf += 1
                elif v[m] == 0.0:
                    assert hits(0.0)
                    n_zero += 1
                else:
                    assert not hits(v[m] * (1 - 1e-9)), (case, metric, m, v[m])
                    if v[m] * (1 + 1e-9) > V_CAP:          # beyond the cap's table: nothing to ask of qmin
                        assert not hits(V_CAP)
                        n_above += 1
                    elif metric == "euclid":
                        assert hits(v[m] * (1 + 1e-9)), (case, m, v[m])
                        n_bracket += 1
        assert (vc["road"] >= vc["euclid"]).all()
        n_road_later += int((vc["road"] > vc["euclid"]).sum())
        # one trajectory per case against the reach checker itself, not through qmin
        fin = np.flatnonzero(np.isfinite(vc["euclid"]) & (vc["euclid"] > 0) & (vc["euclid"] * (1 + 1e-9) <= V_CAP))
        if len(fin):
            m = int(fin[0])
            for sign, want in ((1, True), (-1, False)):
                r2 = HR.reach_table(vc["euclid"][m] * (1 + sign * 1e-9), DT, margin, c.cs, c.T)
                A = HR.arrival_map(c.cls, c.win, c.road, r2, c.hidden)[0]
                first = HR.trajectories(A, c.win, c.road, c.origin, c.cs, c.x[m:m + 1], c.y[m:m + 1], c.head[m:m + 1], HL, HW, WB,
                                        None if c.lens is None else c.lens[m:m + 1])[1]
                assert (first[0] >= 0) == want, (case, m, sign)
    print(f"bracketed {n_bracket}, v_crit = 0: {n_zero}, inf: {n_inf}, above the cap: {n_above}, later along the road: {n_road_later}")
    assert n_bracket > 100 and n_inf > 0 and n_road_later > 0 and n_zero < n_bracket


def test_critical_speed_by_hand():
    # cs = 0.5 m, margin = 0.5 m, dt = 0.1 s; floor(margin^2 / cs^2) = 1
    q = np.array([[169 * 4, 169 * 100, 169 * 16],     # k = 0: D2 = 4 > 1 -> inf; k = 1: (5 - 0.5) / 0.1 = 45; k = 2: (2 - 0.5) / 0.2 = 7.5
                  [169 * 1, HC.NONE, HC.NONE],        # k = 0 within the margin: 0
                  [HC.NONE, 169 * 1, HC.NONE],        # k = 1: r = 0.5 <= margin: 0
                  [HC.NONE, HC.NONE, HC.NONE]])
    v = HC.critical_speed(q, 0.5, 0.1, 0.5)
    assert v[0] == 7.5 and v[1] == 0.0 and v[2] == 0.0 and np.isinf(v[3])


# ------------------------------------------------------------------------------------------------ 4. Python argument checks
def test_python_argument_checks():
    torch, SM = _product()
    z = np.zeros((2, 31))
    veh = (4.508, 1.610, 1.4227)
    call = lambda sm, *a, **kw: SM.SensorModel.hidden_clearance(sm, *a, vehicle=veh, dt=0.1, **kw)
    for sm in (SimpleNamespace(window=None), SimpleNamespace()):          # (not even the window is looked at)
        with pytest.raises(ValueError, match="metric 'manhattan'"):
            call(sm, z, z, z, v_cap=13.9, metric="manhattan")
    with pytest.raises(RuntimeError, match="previous launch"):
        call(SimpleNamespace(window=None), z, z, z, v_cap=13.9, metric="road")
    sm = SimpleNamespace(window=object(), cell_size=0.5)                  # (every check below comes before any device work)
    with pytest.raises(ValueError, match="at most 254"):                  # 13.9 m/s over 10 s: a halo of 279 cells
        call(sm, np.zeros((2, 101)), np.zeros((2, 101)), np.zeros((2, 101)), v_cap=13.9)
    with pytest.raises(ValueError, match=r"x, y and theta must be \[M, T\]"):
        call(sm, z, z[:1], z, v_cap=13.9)
    with pytest.raises(ValueError, match=r"x, y and theta must be \[M, T\]"):
        call(sm, z, z, z[:, :30], v_cap=13.9)
    with pytest.raises(ValueError, match=r"heading must be \[M, T, 2\]"):
        call(sm, z, z, None, v_cap=13.9, heading=np.zeros((2, 31)))
    with pytest.raises(ValueError, match="lengths"):
        call(sm, z, z, z, v_cap=13.9, lengths=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="v_cap >= 0"):
        call(sm, z, z, z, v_cap=-1.0)
    with pytest.raises(ValueError, match="half extents"):
        SM.SensorModel.hidden_clearance(sm, z, z, z, vehicle=(100.0, 1.6, 1.4), v_cap=13.9, dt=0.1)
    # .reach beyond the cap
    margin = math.sqrt(2.0) * 0.5
    r2_cap = int(HR.reach_table(7.0, 0.1, margin, 0.5, 31)[-1])
    out = SM.HiddenClearance(None, torch.full((2, 31), HC.NONE, dtype=torch.int32), None, None, None, r2_cap, "euclid", 0.1, margin, 0.5)
    hit, first, slack = out.reach(7.0)                                    # the cap itself is served
    assert not hit.any() and first.tolist() == [-1, -1] and slack.tolist() == [HC.SLACK_NONE] * 2
    with pytest.raises(ValueError, match="beyond r2_cap"):
        out.reach(7.5)
    assert np.isinf(out.critical_speed().numpy()).all()
