"""Hidden-traffic reach forecast without a GPU: the NumPy checker (tests/ref_hidden_reach.py) against cases
worked out by hand and against the occlusion memory's own model (tests/ref_occlusion_memory.py) -- what the forecast says can
be reached in j steps is what the memory keeps occluded j steps later --, the checker's two footprint scans against each
other, the reach table, the exported symbol and structure, and the refusals of the Python layer that need no device."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_reach as HR
import ref_occlusion_memory as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from frenetix_occlusion import _native
    return _native


# ------------------------------------------------------------------------------------------------ 1. by hand
def _single_source(n=12, src=(5, 5)):
    """window = whole raster (nothing outside it is a source), all road, all visible but one occluded cell"""
    road = np.ones((n, n), dtype=np.uint8)
    cls = np.full((n, n), 3, dtype=np.uint8)
    cls[src[1], src[0]] = 5
    return cls, (0, 0, n, n), road


def test_single_source_rings():
    cls, win, road = _single_source()
    A, D2 = HR.arrival_map(cls, win, road, [2, 8, 18])
    assert D2[5, 5] == 0 and A[5, 5] == 0           # the hidden cell itself
    assert D2[6, 6] == 2 and A[6, 6] == 0           # 1 + 1 <= R2[0]
    assert D2[5, 7] == 4 and A[5, 7] == 1           # 4 > 2, <= 8
    assert D2[7, 7] == 8 and A[7, 7] == 1
    assert D2[5, 8] == 9 and A[5, 8] == 2
    assert D2[8, 8] == 18 and A[8, 8] == 2          # on the last ring's edge: <=
    assert D2[5, 9] == 16 and A[5, 9] == 2
    assert A[8, 9] == 255                            # 16 + 9 = 25 > 18 (outside the searched disc: D2 = -1)
    assert A[1, 1] == 255
    # every cell: the ring index of its own squared distance
    for gy in range(12):
        for gx in range(12):
            d2 = (gx - 5) ** 2 + (gy - 5) ** 2
            want = 0 if d2 <= 2 else 1 if d2 <= 8 else 2 if d2 <= 18 else 255
            assert A[gy, gx] == want, (gx, gy)


def test_reach_crosses_a_wall_and_skips_cells_that_are_not_road():
    cls, win, road = _single_source()
    cls[:, 7] = 2                 # a visible wall that is not road, between the source (5, 5) and column 8
    road[:, 7] = 0
    A, _ = HR.arrival_map(cls, win, road, [2, 8, 18])
    assert (A[:, 7] == 255).all()                    # not road: never
    assert A[5, 8] == 2 and A[5, 9] == 2             # behind the wall: Euclidean reach, by definition
    assert A[5, 6] == 0


def test_no_source_and_zero_reach():
    cls, win, road = _single_source()
    A, _ = HR.arrival_map(cls, win, road, [0, 0, 0])
    assert A[5, 5] == 0 and (np.delete(A.ravel(), 5 * 12 + 5) == 255).all()
    cls[5, 5] = 3
    A, D2 = HR.arrival_map(cls, win, road, [2, 8, 18])
    assert (A == 255).all() and (D2 == -1).all()


def test_outside_the_window():
    road = np.zeros((10, 14), dtype=np.uint8)
    road[:, 2:12] = 1
    win = (4, 3, 5, 4)
    cls = np.full((4, 5), 3, dtype=np.uint8)          # everything in the window is seen
    A, D2 = HR.arrival_map(cls, win, road, [1, 4])
    assert A[0, 0] == 0 and D2[0, 0] == 1             # next to unobserved road left of and below the window
    assert A[1, 2] == 1 and D2[1, 2] == 4             # two cells from the window's lower edge (row 2 is road)
    gx = np.array([3, 9, 12, 1, -1, 5, 5, 5])
    gy = np.array([3, 4, 4, 4, 4, -1, 10, 2])
    got = HR.arrival_at(A, win, road, gx, gy)
    assert got.tolist() == [0, 0, 255, 255, 255, 255, 255, 0]   # road / road / not road / not road / off the raster x3 / road
    assert HR.arrival_at(A, win, road, np.array([4]), np.array([3]))[0] == A[0, 0]
    # a hidden mask replaces the class rule inside the window only
    hid = np.zeros((4, 5), dtype=np.uint8)
    hid[3, 4] = 1
    S = HR.sources(cls, win, road, hid, h=1)
    assert S[1:5, 1:6].sum() == 1 and S[4, 5] and S[0, 0] and S[0, 3]


def test_footprint_ties_and_counts():
    """an axis-aligned rectangle whose edges run through cell centres: <= keeps them"""
    road = np.ones((20, 20), dtype=np.uint8)
    win = (0, 0, 20, 20)
    A = np.full((20, 20), 3, dtype=np.uint8)
    cs, origin = 0.5, (0.0, 0.0)
    x, y = np.full((1, 5), 5.25), np.full((1, 5), 4.75)        # a cell centre: cell (10, 9)
    head = np.zeros((1, 5, 2))
    head[..., 0] = 1.0
    cells, first, slack = HR.trajectories(A, win, road, origin, cs, x, y, head, 1.0, 0.5, 0.0)
    assert cells.tolist() == [[0, 0, 0, 15, 15]]       # |u| <= 1.0: 5 centres along, |w| <= 0.5: 3 across
    assert first.tolist() == [3] and slack.tolist() == [-1]
    cells2, _, _ = HR.trajectories(A, win, road, origin, cs, x, y, head, 0.999, 0.499, 0.0)
    assert cells2.tolist() == [[0, 0, 0, 3, 3]]
    head90 = np.zeros((1, 5, 2))
    head90[..., 1] = 1.0
    cells3, _, _ = HR.trajectories(A, win, road, origin, cs, x, y, head90, 1.0, 0.5, 0.5)   # centre moves up by wb
    assert cells3.tolist() == [[0, 0, 0, 15, 15]]
    c4, f4, s4 = HR.trajectories(A, win, road, origin, cs, x, y, head, 1.0, 0.5, 0.0, lens=np.array([3]))
    assert c4.tolist() == [[0] * 5] and f4.tolist() == [-1] and s4.tolist() == [1]          # A - k at k = 2
    c5, f5, s5 = HR.trajectories(A, win, road, origin, cs, x + 100.0, y, head, 1.0, 0.5, 0.0)
    assert c5.sum() == 0 and f5.tolist() == [-1] and s5.tolist() == [HR.SLACK_NONE]         # off the raster


def test_the_two_footprint_scans_agree():
    rng = np.random.default_rng(5)
    for case in range(12):
        rnx, rny = int(rng.integers(20, 40)), int(rng.integers(20, 40))
        road = (rng.random((rny, rnx)) < 0.7).astype(np.uint8)
        nx, ny = int(rng.integers(6, 16)), int(rng.integers(6, 16))
        win = (int(rng.integers(-4, rnx - 4)), int(rng.integers(-4, rny - 4)), nx, ny)
        A = rng.choice(np.array([0, 1, 2, 5, 255], dtype=np.uint8), (ny, nx))
        cs, origin = 0.5, (-3.0, 2.0)
        M, T = 6, 7
        x = origin[0] + (win[0] + rng.uniform(0, nx, (M, T))) * cs
        y = origin[1] + (win[1] + rng.uniform(0, ny, (M, T))) * cs
        th = rng.uniform(-math.pi, math.pi, (M, T))
        th[0] = [0.0, math.pi / 2, math.pi, -math.pi / 2, math.pi / 4, 0.0, 0.0]
        head = np.stack((np.cos(th), np.sin(th)), -1)
        lens = rng.integers(0, T + 1, M) if case % 2 else None
        a = HR.trajectories(A, win, road, origin, cs, x, y, head, 2.254, 0.805, 1.4227, lens)
        b = HR.trajectories_whole_window(A, win, road, origin, cs, x, y, head, 2.254, 0.805, 1.4227, lens)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
        assert np.array_equal(a[2] <= 0, a[1] >= 0)


# ------------------------------------------------------------------------------------------------ 2. the memory's model
def test_reach_in_j_steps_is_what_the_memory_keeps_occluded_j_steps_later():
    rng = np.random.default_rng(20240131)
    n_cells, n_kept = 0, 0
    for case in range(60):
        rnx, rny = int(rng.integers(24, 48)), int(rng.integers(24, 48))
        road = (rng.random((rny, rnx)) < rng.uniform(0.2, 0.8)).astype(np.uint8)
        def window():
            nx, ny = int(rng.integers(8, 20)), int(rng.integers(8, 20))
            return (int(rng.integers(-6, rnx - nx + 7)), int(rng.integers(-6, rny - ny + 7)), nx, ny)
        W, W2 = window(), window()
        cls = rng.choice(np.array([0, 1, 3, 5], dtype=np.uint8), (W[3], W[2]), p=[0.2, 0.2, 0.45, 0.15])
        cls2 = rng.choice(np.array([0, 1, 3, 5], dtype=np.uint8), (W2[3], W2[2]), p=[0.2, 0.2, 0.2, 0.4])
        cs, dt = 0.5, 0.1
        r2 = HR.reach_table(float(rng.uniform(0.0, 14.0)), dt, math.sqrt(2.0) * cs if case % 3 else 0.0, cs, 11)
        j = int(rng.integers(1, 11))
        S_W = HR.sources(cls, W, road)                       # S restricted to W
        H2, _ = OM.step(cls2, W2, road, int(r2[j]), prev_h=S_W.astype(np.uint8), prev_win=W)
        h = math.isqrt(int(r2[j]))
        D2 = HR.squared_distance(HR.sources(cls, W, road, over=W2, h=h), W2, h, int(r2[j]))
        sel = ((cls2 & 4) != 0) & ((cls2 & 2) == 0)          # every occluded-class, non-visible cell of W'
        want = (D2 >= 0) & (D2 <= int(r2[j]))
        assert np.array_equal(H2[sel] != 0, want[sel]), case
        n_cells += int(sel.sum())
        n_kept += int(want[sel].sum())
    assert n_cells > 3000 and 0 < n_kept < n_cells           # both answers occur


# ------------------------------------------------------------------------------------------------ 3. the Python layer
def test_reach_table_is_the_memorys(native):
    from frenetix_occlusion.sensor_model import hidden_reach_r2
    for v_max, dt, margin, cs, J in ((13.9, 0.1, math.sqrt(2.0) * 0.5, 0.5, 31), (0.0, 0.1, 0.0, 0.5, 5), (8.3, 0.2, 0.3, 0.25, 40),
                                     (50.0, 0.1, 1.0, 0.5, 25)):
        got = hidden_reach_r2(v_max, dt, margin, cs, J)
        assert got.dtype == np.int32 and len(got) == J
        for j in range(J):
            assert int(got[j]) == OM.reach_r2(v_max, j * dt, margin, cs)
        assert np.array_equal(got, HR.reach_table(v_max, dt, margin, cs, J))
        assert (np.diff(got) >= 0).all()


def test_symbol_constants_and_structure(native, tmp_path):
    import ctypes as C
    import subprocess
    lib = native.load()
    assert "fo_scene_hidden_reach" in native.EXPORTS and hasattr(lib, "fo_scene_hidden_reach")
    assert lib.fo_abi_version() == 12
    txt = open(os.path.join(ROOT, "include", "fo_hip.h")).read()
    assert f"#define FO_HIDDEN_REACH_MAX_HALO {native.HIDDEN_REACH_MAX_HALO}" in txt and native.HIDDEN_REACH_MAX_HALO >= 192
    fields = [n for n, *_ in native.HiddenReach._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fo_hip.h"', 'int main(void) {',
             'printf("%zu\\n", sizeof(fo_hidden_reach_t));']
    lines += ['printf("%%zu\\n", offsetof(fo_hidden_reach_t, %s));' % f for f in fields] + ['return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(native.HiddenReach)
    assert out[1:] == [getattr(native.HiddenReach, f).offset for f in fields]
    # no context: refused, not a crash
    assert lib.fo_scene_hidden_reach(None, None, None) == native.FO_E_STATE


def test_python_layer_refuses_without_touching_a_device(native):
    from frenetix_occlusion.interface import FOInterface
    from frenetix_occlusion.sensor_model import CellWindow, SensorModel
    z = np.zeros((2, 31))
    veh = (4.508, 1.610, 1.4227)
    with pytest.raises(RuntimeError, match="previous launch"):
        SensorModel.hidden_reach(SimpleNamespace(window=None), z, z, z, vehicle=veh, v_max=13.9, dt=0.1)
    sm = SimpleNamespace(window=CellWindow(0.0, 0.0, 0.5, 0, 0, 10, 10), cell_size=0.5)
    call = lambda *a, **k: SensorModel.hidden_reach(sm, *a, **{"vehicle": veh, "v_max": 13.9, "dt": 0.1, **k})
    with pytest.raises(ValueError, match="v_max"):
        call(z, z, z, v_max=-1.0)
    with pytest.raises(ValueError, match="v_max"):
        call(z, z, z, margin=-0.1)
    with pytest.raises(ValueError, match="v_max"):
        call(z, z, z, dt=0.0)
    with pytest.raises(ValueError, match="half extents"):
        call(z, z, z, inflate=-3.0)
    with pytest.raises(ValueError, match="half extents"):
        call(z, z, z, inflate=float("inf"))
    with pytest.raises(ValueError, match="half extents"):
        call(z, z, z, vehicle=(4.5, 64.1, 1.4))
    with pytest.raises(ValueError, match=r"\[M, T\]"):
        call(z, z[:, :30], z)
    with pytest.raises(ValueError, match="samples per trajectory"):
        call(np.zeros((1, 255)), np.zeros((1, 255)), np.zeros((1, 255)))
    with pytest.raises(ValueError, match="samples per trajectory"):
        call(np.zeros((1, 0)), np.zeros((1, 0)), np.zeros((1, 0)))
    with pytest.raises(ValueError, match="at most 254"):          # 13.9 m/s x 25.3 s = 703 cells
        call(np.zeros((1, 254)), np.zeros((1, 254)), np.zeros((1, 254)))
    with pytest.raises(ValueError, match="lengths"):
        call(z, z, z, lengths=np.zeros(3, dtype=np.int32))
    fo = SimpleNamespace(timestep=None, sensor_model=SimpleNamespace(window=None))
    with pytest.raises(RuntimeError, match="evaluate_scenario"):
        FOInterface.hidden_reach(fo, {"x": z, "y": z, "theta": z})
