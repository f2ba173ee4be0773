"""The road metric of the occlusion memory on the device (fo_scene_set_occlusion_memory_road, DESIGN.md §5.9 "Road metric")
against the checker of its definition (tests/ref_occlusion_memory_road.py): drives through the one-call step and the stage
calls, two parallel roads whose answer is written down by hand, the smallest windows / reaches / previous windows at which
the kernel takes another path, the compaction's counts, `euclid` untouched, the kernels a run launches, and the refusals."""
import ctypes as C
import glob
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_occlusion_memory as OM
import ref_occlusion_memory_road as R
import test_occlusion_memory_gpu as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = T.DT


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


# ------------------------------------------------------------------------------------------------ drives
@pytest.mark.parametrize("name", ["scenario1", "city_grid"])
def test_drive_matches_the_checker_on_both_paths(torch_cuda, name):
    """12 steps, rule families on; the timestep advances by 1 and once by 10 (r2 = 853 at 13.9 m/s: a halo of 31 cells, the
    large shape of the kernel).  At every step H, the class bytes, the occluded index list and its count are the checker's on
    the classes of a run without memory, through the one-call step and through the stage calls; so are the reset reasons"""
    torch = torch_cuda
    sc, ego0, yaw, path = T._scenario(name)
    inter = getattr(sc, "intersections", None)
    off = T._stack(torch, sc.lanelets, sc.obstacles, path, inter, ego0[:2], yaw)
    fused = T._stack(torch, sc.lanelets, sc.obstacles, path, inter, ego0[:2], yaw, memory={"metric": "road"})
    staged = T._stack(torch, sc.lanelets, sc.obstacles, path, inter, ego0[:2], yaw, memory={"metric": "road"})
    assert fused.sm.occlusion_memory_metric == "road" and off.sm.occlusion_memory_metric == "euclid"
    road = off.sm.road_raster()
    model = R.Memory(13.9, DT, off.sm.cell_size)
    euclid = OM.Memory(13.9, DT, off.sm.cell_size)
    ts = [0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 19, 20]
    r2s, n_less = [], 0
    for step, t in enumerate(ts):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        a = T._run(torch, off, ego, yaw, float(ego0[3]), step, t)
        f = T._run(torch, fused, ego, yaw, float(ego0[3]), step, t)
        s = T._run(torch, staged, ego, yaw, float(ego0[3]), step, t, staged=True)
        w = f["win"]
        win = (w.ix0, w.iy0, w.nx, w.ny)
        r2s.append(model.plan(t)[0])
        H, out, reason = model.advance(a["cls"], win, road, t)
        He, _, _ = euclid.advance(a["cls"], win, road, t)
        assert f["reason"] == s["reason"] == reason == ("first" if step == 0 else None), step
        assert np.array_equal(f["H"], H) and np.array_equal(s["H"], H), step
        assert np.array_equal(f["cls"], out), step
        want = np.flatnonzero(out.reshape(-1) & 4)
        assert len(f["occ"]) == len(want) and np.array_equal(f["occ"], want), step
        T._same(f, s)
        if reason is not None:
            T._same(f, a)
        assert (H <= He).all(), step                # (the Euclidean memory of the same drive: a superset at every step)
        n_less += int((H != He).sum())
    assert r2s[1] == 17 and r2s[6] == 853
    print(f"{name}: cells hidden under euclid and not under road, summed over the drive: {n_less}")


# ------------------------------------------------------------------------------------------------ small synthetic maps
def _lane(lid, x_lo, x_hi, y_lo, y_hi, n=41):
    from frenetix_occlusion import scenario as S
    xs = np.linspace(x_lo, x_hi, n)
    return S.Lanelet(lid, np.stack((xs, np.full(n, y_hi)), -1), np.stack((xs, np.full(n, y_lo)), -1))


def _sensor(torch, lanes, car_xy, path_y):
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    path = np.stack((np.linspace(-5, 65, 141), np.full(141, path_y)), -1)
    car = S.Obstacle(77, "static", "parkedVehicle", 4.5, 1.8, 0, np.array([car_xy[0], car_xy[1], 0.0, 0.0]), np.zeros((0, 4)))
    sm = SensorModel(lanes, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720)
    obs = FOObstacles([car])
    obs.update(0)
    sm.upload_obstacles(obs)
    return sm


def _launch(torch, sm, ego, arm=None, win=None):
    """one visibility stage; arm = (entry point name, r2, prev_h [pny, pnx], prev_win) arms the context by hand (the sensor
    model's own memory is off); win = (ix0, iy0, nx, ny) replaces the sensor model's window"""
    from frenetix_occlusion import _native as N
    from frenetix_occlusion.sensor_model import CellWindow
    if win is not None:
        (x0, y0), cs = sm.raster_origin, sm.cell_size
        sm._window_for = lambda ego_pos: CellWindow(x0, y0, cs, *win)
    w = sm._window_for(ego)
    cur = None
    if arm is not None:
        fn, r2, prev_h, pw = arm
        cur = torch.full((w.nx * w.ny,), 7, dtype=torch.uint8, device="cuda")
        prev = torch.as_tensor(np.ascontiguousarray(prev_h, dtype=np.uint8)).cuda().reshape(-1)
        m = N.OcclusionMemory(r2=r2, reset=0, prev_ix0=pw[0], prev_iy0=pw[1], prev_nx=pw[2], prev_ny=pw[3],
                              d_prev=prev.data_ptr(), prev_bytes=prev.numel(), d_cur=cur.data_ptr(), cur_bytes=cur.numel())
        assert getattr(sm.ctx._lib, fn)(sm.ctx._h, C.byref(m)) == N.FO_OK
    sm.launch(np.asarray(ego, dtype=np.float64), 0.0)
    torch.cuda.synchronize()
    n = int(sm.n_occluded.item())
    return dict(cls=sm.cell_class.cpu().numpy().copy(), occ=sm.occluded_idx_buffer[:n].cpu().numpy().copy(), n=n,
                H=None if cur is None else cur.view(w.ny, w.nx).cpu().numpy(), win=(w.ix0, w.iy0, w.nx, w.ny))


def _check(got, cls0, road, r2, prev_h, pw, ref=R):
    H, out = ref.step(cls0, got["win"], road, r2, prev_h, pw)
    assert np.array_equal(got["H"], H)
    assert np.array_equal(got["cls"], out)
    want = np.flatnonzero(out.reshape(-1) & 4)
    assert got["n"] == len(want) and np.array_equal(got["occ"], want)
    return H


ROAD, EUCLID = "fo_scene_set_occlusion_memory_road", "fo_scene_set_occlusion_memory"


@pytest.mark.parametrize("gap", [False, True])
def test_two_parallel_roads_by_hand(torch_cuda, gap):
    """near lane y in [-3.5, 0], a strip of 1 m (two cell rows) that is not road, far lane y in [1, 4.5], both 50 m long inside
    the window; the ego on the near lane behind a parked car whose shadow falls over both.  The classes are the visibility
    stage's; the previous hidden set is made by hand: the far lane, nothing else.  r2 = 17 (h = 4, L = 53).
    `euclid` keeps every occluded cell off the far lane whose disc holds a far-lane cell: at most 4 rows from it.  `road`:
    nothing joins the lanes, so all of those are cleared; with a connector one cell wide at x = 20 the cells a path through it
    reaches within 53 stay: the connector's two cells (12, 24), below it 36 and 48, beside those 41 41 53 53 and 53 53"""
    torch = torch_cuda
    lanes = [_lane(1, -10.0, 40.0, -3.5, 0.0), _lane(2, -10.0, 40.0, 1.0, 4.5)]
    if gap:
        lanes.append(_lane(3, 20.0, 20.5, 0.0, 1.0, n=2))
    sm = _sensor(torch, lanes, (10.0, -0.95), -1.75)
    ego = (0.0, -1.75)
    base = _launch(torch, sm, ego)
    ix0, iy0, nx, ny = win = base["win"]
    road = sm.road_raster()
    rd = OM.previous_p(road, None, None, win, 0) != 0
    rows = np.flatnonzero(rd.any(axis=1))
    cols = np.flatnonzero(rd.any(axis=0))
    # the map the hand answer is written for: 7 near rows, 2 strip rows, 7 far rows, every lane row road from cols[0] to cols[-1]
    assert len(rows) == (16 if gap else 14) and rows[-1] - rows[0] == 15
    near, strip, far = rows[0] + np.arange(7), rows[0] + 7 + np.arange(2), rows[0] + 9 + np.arange(7)
    assert rd[near][:, cols[0]:cols[-1] + 1].all() and rd[far][:, cols[0]:cols[-1] + 1].all()
    gx = None
    if gap:
        assert (rd[strip].sum(axis=1) == 1).all() and rd[strip[0]].argmax() == rd[strip[1]].argmax()
        gx = int(rd[strip[0]].argmax())
    else:
        assert not rd[strip].any()
    prev_h = np.zeros((ny, nx), dtype=np.uint8)
    prev_h[far] = rd[far]
    cls0 = base["cls"]
    occ = ((cls0 & 4) != 0) & ((cls0 & 2) == 0)
    e = _launch(torch, sm, ego, (EUCLID, 17, prev_h, win))
    r = _launch(torch, sm, ego, (ROAD, 17, prev_h, win))
    _check(e, cls0, road, 17, prev_h, win, ref=OM)
    _check(r, cls0, road, 17, prev_h, win)
    # by hand: rows and columns away from the far lane's rectangle
    Y, X = np.mgrid[0:ny, 0:nx]
    dy = np.maximum(np.maximum(far[0] - Y, Y - far[-1]), 0)
    dx = np.maximum(np.maximum(cols[0] - X, X - cols[-1]), 0)
    in_far = (dy == 0) & (dx == 0)
    keep_e = occ & (dx * dx + dy * dy <= 17)
    keep_r = occ & in_far
    if gap:
        below = near[-1]                                    # the near lane's row next to the strip
        path_cells = [(gx, strip[0]), (gx, strip[1]), (gx, below), (gx, below - 1), (gx - 1, below), (gx + 1, below),
                      (gx - 2, below), (gx + 2, below), (gx - 1, below - 1), (gx + 1, below - 1)]
        for x, y in path_cells:
            assert occ[y, x], "the car's shadow does not cover the connector"
            keep_r[y, x] = True
    assert np.array_equal(e["H"][occ] != 0, keep_e[occ])
    assert np.array_equal(r["H"][occ] != 0, keep_r[occ])
    cleared = keep_e & ~keep_r
    assert cleared.sum() > 0 and cleared[near[-2:]].sum() > 0, "no occluded near-lane cell within the disc of the far lane"
    assert np.array_equal((e["cls"] & 4) != 0, keep_e) and np.array_equal((r["cls"] & 4) != 0, keep_r)
    assert not ((r["cls"] & 4) != 0)[cleared].any() and ((e["cls"] & 4) != 0)[cleared].all()


@pytest.fixture(scope="module")
def parked(torch_cuda):
    lanes, _, _ = T._parked_car_scene()
    sm = _sensor(torch_cuda, lanes, (17.0, -2.4), -1.0)
    return sm, sm.road_raster()


def _cell(sm, x, y):
    (x0, y0), cs = sm.raster_origin, sm.cell_size
    return int(math.floor((x - x0) / cs)), int(math.floor((y - y0) / cs))


def _prev(rng, pw, density, road):
    """a previous hidden set made by hand: random cells, a band of rows seen empty, and in the left half of its window no cell
    on or next to road (what is hidden there is cut off from the road: the disc reaches across, the road metric does not)"""
    h = (rng.random((pw[3], pw[2])) < density).astype(np.uint8)
    h[pw[3] // 3:pw[3] // 3 + 6] = 0
    rd = np.pad(OM.previous_p(road, None, None, pw, 0) != 0, 1)
    near = np.zeros((pw[3], pw[2]), dtype=bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near |= rd[dy:dy + pw[3], dx:dx + pw[2]]
    near[:, pw[2] // 2:] = False
    h[near] = 0
    return h


@pytest.mark.parametrize("shape", [(45, 37), (33, 65)])
def test_smallest_shapes_match_the_checker(torch_cuda, parked, shape):
    """windows that are no multiple of the 32 x 32 tile, over the shadow of a parked car (and partly off the raster, which ends
    a few metres beside the lanes); every reach at which the kernel changes its path -- 0 (no round), 1, 2, 17 (the usual one),
    853 and 1024 (the large shape; the cap) --; the previous window shifted by (-7, +5), disjoint, and partly off the raster"""
    torch = torch_cuda
    sm, road = parked
    rny, rnx = road.shape
    nx, ny = shape
    cx, cy = _cell(sm, -2.0 if nx == 45 else 24.0, -10.0 if nx == 45 else -20.0)
    win = (cx, cy, nx, ny)
    ego = (0.0, -1.0)
    base = _launch(torch, sm, ego, win=win)
    cls0 = base["cls"]
    occ = (cls0 & 4) != 0
    assert base["win"] == win and occ.sum() > 0
    assert cy < 0 or cy + ny > rny, "the window was meant to reach off the raster"
    if nx == 45:      # a tile without an occluded cell next to one with occluded cells
        assert not occ[:32, :32].any() and occ[:32, 32:].any()
    rng = np.random.default_rng(7 + nx)
    n_diff = 0
    for r2 in (0, 1, 2, 17, 853, 1024):
        for pw in ((cx - 7, cy + 5, nx, ny), (cx + 200, cy + 150, 20, 12), (-9, rny - 11, 58, 40), win):
            prev_h = _prev(rng, pw, 0.02 if r2 > 100 else 0.2, road)
            r = _launch(torch, sm, ego, (ROAD, r2, prev_h, pw))
            H = _check(r, cls0, road, r2, prev_h, pw)
            He, _ = OM.step(cls0, win, road, r2, prev_h, pw)
            assert (H <= He).all()
            n_diff += int((H != He).sum())
    assert n_diff > 0, "the two metrics never differed"


def test_counts_where_cleared_cells_straddle_compaction_blocks(torch_cuda):
    """a wave of the road kernel is two 32-cell row segments of a tile, not 64 consecutive cells.  The two parallel lanes
    under the car's shadow, in a window 36 cells wide and 64 high placed so that the near lane's last row is window row 28
    (cells 1008 .. 1043: the block boundary 1024 in tile row 0) and the far lane holds row 35 (1260 .. 1295: 1280, tile row 1).
    Nothing was hidden before (every occluded cell is cleared), then random previous sets: count and index list are exact"""
    torch = torch_cuda
    lanes = [_lane(1, -10.0, 40.0, -3.5, 0.0), _lane(2, -10.0, 40.0, 1.0, 4.5)]
    sm = _sensor(torch, lanes, (10.0, -0.95), -1.75)
    road = sm.road_raster()
    ego = (0.0, -1.75)
    cx, cy = _cell(sm, 24.0, -3.25)
    win = (cx, cy - 22, 36, 64)
    base = _launch(torch, sm, ego, win=win)
    cls0 = base["cls"]
    assert base["win"] == win
    rng = np.random.default_rng(3)
    idx = np.arange(64 * 36).reshape(64, 36)
    for r2, prev_h in ((0, np.zeros((64, 36), dtype=np.uint8)), (17, _prev(rng, win, 0.05, road)), (853, _prev(rng, win, 0.002, road))):
        r = _launch(torch, sm, ego, (ROAD, r2, prev_h, win))
        H = _check(r, cls0, road, r2, prev_h, win)
        if r2 == 0:
            cleared = ((cls0 & 4) != 0) & (H == 0)
            assert r["n"] == 0 and cleared.sum() > 100
            for band in range(2):    # every tile row: some wave (rows y, y + 1 of a tile) clears cells of more than one block
                waves = 0
                for tx in range(2):
                    for y in range(32 * band, 32 * band + 32, 2):
                        sel = cleared[y:y + 2, 32 * tx:32 * tx + 32]
                        waves += len(set((idx[y:y + 2, 32 * tx:32 * tx + 32][sel] >> 8).tolist())) > 1
                assert waves > 0, band


# ------------------------------------------------------------------------------------------------ euclid is untouched
def test_euclid_is_the_old_call(torch_cuda):
    """metric="euclid" against a sensor model armed the way it was before the metric existed, and against the disc's checker"""
    torch = torch_cuda
    sc, ego0, yaw, path = T._scenario("city_grid")
    a = T._stack(torch, sc.lanelets, sc.obstacles, path, None, ego0[:2], yaw, memory={})
    b = T._stack(torch, sc.lanelets, sc.obstacles, path, None, ego0[:2], yaw, memory={"metric": "euclid"})
    off = T._stack(torch, sc.lanelets, sc.obstacles, path, None, ego0[:2], yaw)
    model = OM.Memory(13.9, DT, a.sm.cell_size)
    road = a.sm.road_raster()
    for step in range(6):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        ra = T._run(torch, a, ego, yaw, float(ego0[3]), step, step)
        rb = T._run(torch, b, ego, yaw, float(ego0[3]), step, step)
        ro = T._run(torch, off, ego, yaw, float(ego0[3]), step, step)
        T._same(ra, rb)
        w = ra["win"]
        H, out, reason = model.advance(ro["cls"], (w.ix0, w.iy0, w.nx, w.ny), road, step)
        assert np.array_equal(ra["H"], rb["H"]) and np.array_equal(rb["H"], H) and np.array_equal(rb["cls"], out)
        assert ra["reason"] == rb["reason"] == reason


_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import numpy as np, torch
import test_occlusion_memory_gpu as T
import test_occlusion_memory_road_gpu as G
lanes, _, _ = T._parked_car_scene()
sm = G._sensor(torch, lanes, (17.0, -2.4), -1.0)
sm.enable_occlusion_memory(dt=0.1, metric=sys.argv[1])
reasons = []
for i, t in enumerate((0, 1, 2, 2, 3)):
    sm.launch(np.array([0.8 * i, -1.0]), 0.0, timestep=t)
    torch.cuda.synchronize()
    reasons.append(str(sm.occlusion_memory_reset_reason))
print("child ok", ",".join(reasons))
'''


def _trace(tmp_path, metric):
    import shutil
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    child = tmp_path / "child_memory.py"
    child.write_text(_TRACE_CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "frenetix-occlusion_amd"),
                                         tests=os.path.join(ROOT, "tests")))
    d = tmp_path / ("trace_" + metric)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child), metric],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    reasons = r.stdout.split("child ok")[1].split()[0].split(",")
    return "\n".join(open(f).read() for f in files).splitlines(), reasons


def test_kernel_trace_of_the_two_metrics(torch_cuda, tmp_path):
    """five steps, the fourth with a timestep that does not advance: a run that never arms `road` launches the disc kernel five
    times and the road kernel never; a run that arms `road` launches the road kernel on the three steps that are no reset and
    the disc kernel on the two that are"""
    lines, reasons = _trace(tmp_path, "euclid")
    count = lambda k: sum(k in line for line in lines)
    assert reasons == ["first", "None", "None", "time", "None"]
    assert count("fo_occlusion_memory_road_kernel") == 0 and count("fo_occlusion_memory_kernel") == 5
    lines, reasons = _trace(tmp_path, "road")
    assert reasons == ["first", "None", "None", "time", "None"]
    assert count("fo_occlusion_memory_road_kernel") == 3 and count("fo_occlusion_memory_kernel") == 2


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_the_later_call_wins(torch_cuda, parked):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, road = parked
    lib, h = sm.ctx._lib, sm.ctx._h
    buf = torch.zeros(8, dtype=torch.uint8, device="cuda")
    call = lambda m: lib.fo_scene_set_occlusion_memory_road(h, m)
    cap = N.OCCLUSION_MEMORY_MAX_HALO
    assert call(N.OcclusionMemory(r2=cap * cap + 1, reset=1, d_cur=buf.data_ptr(), cur_bytes=8)) == N.FO_E_ARG
    assert call(N.OcclusionMemory(r2=-1, reset=1, d_cur=buf.data_ptr(), cur_bytes=8)) == N.FO_E_ARG
    assert call(N.OcclusionMemory(r2=4, reset=1, d_cur=None, cur_bytes=8)) == N.FO_E_ARG
    assert call(N.OcclusionMemory(r2=4, reset=0, prev_nx=4, prev_ny=4, d_prev=buf.data_ptr(), prev_bytes=8,
                                  d_cur=buf.data_ptr() + 4, cur_bytes=4)) == N.FO_E_ARG          # previous buffer too small
    assert call(N.OcclusionMemory(r2=4, reset=0, prev_nx=2, prev_ny=2, d_prev=buf.data_ptr(), prev_bytes=4,
                                  d_cur=buf.data_ptr(), cur_bytes=4)) == N.FO_E_ARG              # one buffer for both steps
    assert call(N.OcclusionMemory(r2=cap * cap, reset=1, d_cur=buf.data_ptr(), cur_bytes=8)) == N.FO_OK
    ego = np.array([0.0, -1.0])
    with pytest.raises(N.NativeError) as e:          # armed with an 8-byte buffer: the next visibility stage refuses the window
        sm.launch(ego, 0.0)
    assert e.value.code == N.FO_E_ARG
    cx, cy = _cell(sm, 21.0, -14.0)
    win = (cx, cy, 40, 64)
    base = _launch(torch, sm, ego, win=win)          # ... and the arming went with it
    cls0 = base["cls"]
    prev_h = _prev(np.random.default_rng(5), win, 0.05, road)
    He, _ = OM.step(cls0, win, road, 17, prev_h, win)
    Hr, _ = R.step(cls0, win, road, 17, prev_h, win)
    assert (He != Hr).any()
    m = N.OcclusionMemory(r2=cap * cap, reset=1, d_cur=buf.data_ptr(), cur_bytes=8)
    # the later of the two arming calls decides
    assert call(m) == N.FO_OK
    assert np.array_equal(_launch(torch, sm, ego, (EUCLID, 17, prev_h, win))["H"], He)
    assert lib.fo_scene_set_occlusion_memory(h, m) == N.FO_OK
    assert np.array_equal(_launch(torch, sm, ego, (ROAD, 17, prev_h, win))["H"], Hr)
    # NULL disarms, through either entry
    assert call(m) == N.FO_OK and call(None) == N.FO_OK
    assert np.array_equal(_launch(torch, sm, ego)["cls"], cls0)
    assert call(m) == N.FO_OK and lib.fo_scene_set_occlusion_memory(h, None) == N.FO_OK
    assert np.array_equal(_launch(torch, sm, ego)["cls"], cls0)
    # a reset through the road entry is the disc call's reset: the classes of an unarmed stage, H = what they say
    cur = torch.full((40 * 64,), 7, dtype=torch.uint8, device="cuda")
    assert call(N.OcclusionMemory(r2=17, reset=1, d_cur=cur.data_ptr(), cur_bytes=cur.numel())) == N.FO_OK
    got = _launch(torch, sm, ego)
    H0, out0 = OM.step(cls0, win, road, 0)
    assert np.array_equal(got["cls"], cls0) and np.array_equal(out0, cls0)
    assert np.array_equal(cur.view(64, 40).cpu().numpy(), H0)
