"""The extended future-visibility sweep (fo_scene_future_visibility_ex) on a real MI355X: against the old entry with its
defaults, the C oracle pose by pose with moving occluder slices, the NumPy checker of tests/ref_future_visibility.py for
sector fans and first-seen counts, a known answer (an obstacle that drives off), the FOInterface path and its refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ref_future_visibility as RF

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


def _load(name):
    from frenetix_occlusion import scenario as S
    if name == "city":
        return S.synthetic_urban_grid()
    return S.load_geometry_npz(os.path.join(GOLDEN, f"{name}_geometry.npz"))


def _scene(sc, ego, radius=50.0, obstacles=None):
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    sm = SensorModel(sc.lanelets, None, sensor_radius=radius, sensor_angle=360.0)
    ob = FOObstacles(sc.obstacles)
    ob.update(0)
    if obstacles is None:
        sm.calc_visible_and_occluded_area(0, ego[:2], float(ego[2]), ob)
    else:
        sm.upload_obstacles(obstacles)
        sm.launch(ego[:2], float(ego[2]))
    return sm, ob


def _ref(sm, traj, stride, corn, flags, fov=360.0, n_rays=192, heading=None, rows=None):
    from frenetix_occlusion.sensor_model import ray_dirs
    w = sm.window
    x0, y0 = sm.raster_origin
    dirs = ray_dirs(n_rays, 0.0, fov)
    return RF.future_visibility(traj["x"], traj["y"], stride, dirs, sm.sensor_radius, sm.map_geometry.edges, corn, flags,
                                sm.occluded_cells().cpu().numpy(), x0, y0, sm.cell_size, w.ix0, w.iy0, w.nx,
                                full=fov >= 359.9, heading=heading, rows=rows)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _moving(ob, stride, K):
    return ob.rows_at([k * stride for k in range(K)])


@pytest.mark.parametrize("name", ["scenario1", "scenario3", "city"])
def test_one_slice_defaults_are_the_old_entry_bit_for_bit(torch_cuda, name):
    from frenetix_occlusion import synthetic as SY
    sc = _load(name)
    ego = sc.ego_initial
    sm, _ = _scene(sc, ego)
    traj = SY.make_trajectories(40, seed=21, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    for n_rays in (97, 192, 720, 768):
        rev, area = sm.future_visibility(traj["x"], traj["y"], t_stride=5, n_rays=n_rays)
        fv = sm.future_visibility_ex(traj["x"], traj["y"], t_stride=5, n_rays=n_rays)
        torch_cuda.cuda.synchronize()
        assert fv.revealed_new is None and fv.revealed_any is None
        assert torch_cuda.equal(rev, fv.revealed), n_rays
        assert torch_cuda.equal(area.view(torch_cuda.int64), fv.area.view(torch_cuda.int64)), n_rays
        assert int(rev.max()) > 0


def test_scenario_slices_match_the_oracle_pose_by_pose(torch_cuda, oracle):
    """scenario 1's five cars at their recorded states timestep + k stride: every pose equals the C oracle called with
    that pose's slice, and the moving cars change at least one count against 'now'"""
    from frenetix_occlusion import synthetic as SY
    sc = _load("scenario1")
    ego = sc.ego_initial
    sm, ob = _scene(sc, ego)
    stride, M = 5, 48
    traj = SY.make_trajectories(M, seed=7, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    K = (traj["x"].shape[1] + stride - 1) // stride
    corn, flags = _moving(ob, stride, K)
    fv = sm.future_visibility_ex(traj["x"], traj["y"], t_stride=stride, occluders=(corn, flags))
    now = sm.future_visibility_ex(traj["x"], traj["y"], t_stride=stride)
    rev, area, rev_now = _np(fv.revealed), _np(fv.area), _np(now.revealed)
    w = sm.window
    x0, y0 = sm.raster_origin
    occ = sm.occluded_cells().cpu().numpy()
    dirs = sm._fvx_dirs.cpu().numpy()
    for k in range(K):
        xs, ys = traj["x"][:, k * stride:k * stride + 1], traj["y"][:, k * stride:k * stride + 1]
        r_k, a_k = oracle.future_visibility(xs, ys, 1, dirs, sm.sensor_radius, sm.map_geometry.edges, corn[k], flags[k], occ,
                                            x0, y0, sm.cell_size, w.ix0, w.iy0, w.nx)
        assert np.array_equal(rev[:, k], r_k[:, 0]), k
        np.testing.assert_allclose(area[:, k], a_k[:, 0], rtol=1e-12, atol=1e-9)
    assert (rev != rev_now).any()


def _bus_scene(torch_cuda):
    """a standing ego behind a 12 m bus 9 m ahead on its lane; slices: the bus drives off ahead, 6 m per pose"""
    sc = _load("scenario1")
    ego = sc.ego_initial
    hx, hy = math.cos(ego[2]), math.sin(ego[2])
    from frenetix_occlusion.scenario import Obstacle

    def bus_at(d):
        pose = (ego[0] + d * hx, ego[1] + d * hy, float(ego[2]))
        return Obstacle(1, "dynamic", "bus", 12.0, 2.6, 0, np.array(pose + (0.0,)), np.zeros((0, 4))).corners(pose)
    c0 = bus_at(9.0)
    sm, _ = _scene(sc, ego, obstacles=(c0[None], np.array([[ego[0] + 9 * hx, ego[1] + 9 * hy]]), np.array([3], np.uint8)))
    K, stride = 7, 5
    corn = np.stack([bus_at(9.0 + 6.0 * k)[None] for k in range(K)])
    flags = np.full((K, 1), 3, np.uint8)
    still = {k: np.full((3, 31), v) for k, v in (("x", ego[0]), ("y", ego[1]), ("theta", ego[2]))}
    return sm, still, corn, flags, stride


def test_known_answer_an_obstacle_that_drives_off(torch_cuda):
    """fails without the feature: with the bus where it stands now a standing trajectory sees the same at every pose;
    with the bus driving off, later poses see into what it hid"""
    sm, still, corn, flags, stride = _bus_scene(torch_cuda)
    assert int(sm.n_occluded.item()) > 100
    now = _np(sm.future_visibility_ex(still["x"], still["y"], t_stride=stride).revealed)
    fv = sm.future_visibility_ex(still["x"], still["y"], t_stride=stride, occluders=(corn, flags), first_seen=True)
    rev = _np(fv.revealed)
    assert (now == now[:, :1]).all()
    assert (rev[:, 0] == now[:, 0]).all()
    assert (rev[:, -1] > rev[:, 0] + 50).all() and (np.diff(rev, axis=1) >= 0).all()
    r2, a2, n2, any2 = _ref(sm, still, stride, corn, flags)
    assert np.array_equal(rev, r2) and np.array_equal(_np(fv.revealed_new), n2) and np.array_equal(_np(fv.revealed_any), any2)


@pytest.mark.parametrize("fov", [90.0, 120.0, 270.0, 359.9])
@pytest.mark.parametrize("n_rays", [257, 720])
def test_sector_fans_match_the_checker(torch_cuda, fov, n_rays):
    from frenetix_occlusion import synthetic as SY
    sc = _load("scenario1")
    ego = sc.ego_initial
    sm, ob = _scene(sc, ego)
    stride, M = 5, 12
    traj = SY.make_trajectories(M, seed=31, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    corn, flags = _moving(ob, stride, 7)
    fv = sm.future_visibility_ex(traj["x"], traj["y"], traj["theta"], t_stride=stride, n_rays=n_rays, fov=fov,
                                 occluders=(corn, flags), first_seen=True)
    th = traj["theta"][:, ::stride]
    head = np.stack((np.cos(th), np.sin(th)), -1)
    r, a, n, an = _ref(sm, traj, stride, corn, flags, fov=fov, n_rays=n_rays, heading=head)
    assert np.array_equal(_np(fv.revealed), r)
    np.testing.assert_allclose(_np(fv.area), a, rtol=1e-12, atol=1e-9)
    assert np.array_equal(_np(fv.revealed_new), n) and np.array_equal(_np(fv.revealed_any), an)
    if fov < 180.0:
        # nothing behind the pose: the same call over the cells behind the ego only counts nothing at pose 0
        w = sm.window
        x0, y0 = sm.raster_origin
        idx = np.arange(w.nx * w.ny, dtype=np.int64)
        cx = x0 + ((w.ix0 + idx % w.nx) + 0.5) * sm.cell_size - ego[0]
        cy = y0 + ((w.iy0 + idx // w.nx) + 0.5) * sm.cell_size - ego[1]
        behind = idx[cx * math.cos(ego[2]) + cy * math.sin(ego[2]) < 0.0].astype(np.int32)
        out = _raw_call(torch_cuda, sm, traj, stride, n_rays, fov, head, corn, flags, behind)
        assert len(behind) > 1000 and (out[0][:, 0] == 0).all()


def _raw_call(torch, sm, traj, stride, n_rays, fov, head, corn, flags, occ, win=None, n_slices=None, first_seen=False):
    """fo_scene_future_visibility_ex through ctypes with an occluded list (and window) of the caller's"""
    from frenetix_occlusion import _native as N
    dev = sm.device
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dev, dt).contiguous()
    x, y = t(traj["x"]), t(traj["y"])
    M, T = x.shape
    K = (T + stride - 1) // stride
    dirs = torch.empty((n_rays, 2), dtype=torch.float64, device=dev)
    sm.ctx.call("fo_scene_fan", n_rays, 0.0, float(fov), sm.sensor_radius, 0, dirs.data_ptr(), None, None,
                N.current_stream(sm._dev_index))
    hd = None if head is None else t(head)
    dc, df = t(corn), t(flags, torch.uint8)
    oi = t(occ, torch.int32)
    n = torch.tensor([len(occ)], dtype=torch.int32, device=dev)
    rev = torch.empty((M, K), dtype=torch.int32, device=dev)
    area = torch.empty((M, K), dtype=torch.float64, device=dev)
    new = torch.empty((M, K), dtype=torch.int32, device=dev) if first_seen else None
    w = sm.window
    nx, ny = (w.nx, w.ny) if win is None else win
    args = N.FutureVisibility(M=M, T=T, t_stride=stride, n_rays=n_rays, d_x=x.data_ptr(), d_y=y.data_ptr(),
                              d_dirs=dirs.data_ptr(), r=sm.sensor_radius, fov_deg=float(fov),
                              d_heading=None if hd is None else hd.data_ptr(), O=int(dc.shape[1]),
                              n_slices=int(dc.shape[0]) if n_slices is None else n_slices, d_ocorn=dc.data_ptr(),
                              d_oflags=df.data_ptr(), d_occ_idx=oi.data_ptr(), d_n_occ=n.data_ptr(), win_ix0=w.ix0,
                              win_iy0=w.iy0, win_nx=nx, win_ny=ny, d_revealed=rev.data_ptr(), d_area=area.data_ptr(),
                              d_revealed_new=None if new is None else new.data_ptr(), d_revealed_any=None)
    sm.ctx.call("fo_scene_future_visibility_ex", C.byref(args), N.current_stream(sm._dev_index))
    torch.cuda.synchronize()
    return _np(rev), _np(area), _np(new)


def test_first_seen_properties(torch_cuda):
    from frenetix_occlusion import synthetic as SY
    sc = _load("scenario3")
    ego = sc.ego_initial
    sm, ob = _scene(sc, ego)
    stride = 5
    traj = SY.make_trajectories(64, seed=41, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    corn, flags = _moving(ob, stride, 7)
    fv = sm.future_visibility_ex(traj["x"], traj["y"], t_stride=stride, n_rays=720, occluders=(corn, flags), first_seen=True)
    rev, new, any_ = _np(fv.revealed), _np(fv.revealed_new), _np(fv.revealed_any)
    r, _, n, an = _ref(sm, traj, stride, corn, flags, n_rays=720)
    assert np.array_equal(rev, r) and np.array_equal(new, n) and np.array_equal(any_, an)
    assert np.array_equal(new.sum(axis=1), any_)
    assert (any_ >= rev.max(axis=1)).all() and (any_ <= int(sm.n_occluded.item())).all()
    assert (any_ > rev.max(axis=1)).any()      # some trajectory reveals more than its best single pose sees
    # a standing trajectory with static occluders sees everything at its first pose
    still = {k: np.repeat(v[:, :1], 31, axis=1) for k, v in traj.items()}
    fs = sm.future_visibility_ex(still["x"], still["y"], t_stride=stride, n_rays=720, first_seen=True)
    sr, sn = _np(fs.revealed), _np(fs.revealed_new)
    assert (sn[:, 1:] == 0).all() and np.array_equal(sn[:, 0], sr[:, 0]) and np.array_equal(_np(fs.revealed_any), sr[:, 0])


def _interface(tmp_path):
    from types import SimpleNamespace

    import yaml
    from frenetix_occlusion import interface, synthetic as SY
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["accelerator"]["spawn"]["mode"] = "cells"
    cfg["sensor_model"]["sensor_angle"] = 120.0
    p = tmp_path / "occ.yaml"
    p.write_text(yaml.safe_dump(cfg))
    sc = _load("scenario1")
    ego = sc.ego_initial
    ref_path = ego[None, :2] + np.linspace(0, 80, 81)[:, None] * np.array([[math.cos(ego[2]), math.sin(ego[2])]])
    veh = SimpleNamespace(**dict(zip(("length", "width", "wb_rear_axle", "mass", "a_max"), SY.VEHICLE_BMW320I)))
    return interface.FOInterface(sc, ref_path, veh, 0.1, config_path=str(p)), sc


def test_interface_occluder_sources_and_refusals(torch_cuda, tmp_path):
    from frenetix_occlusion import synthetic as SY
    fo, sc = _interface(tmp_path)
    ego = sc.ego_initial
    traj = SY.make_trajectories(16, seed=2, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    with pytest.raises(RuntimeError):
        fo.future_visibility(traj)                                          # no evaluate_scenario yet
    first, second = fo.fo_obstacles.fo_obstacles[0], fo.fo_obstacles.fo_obstacles[1]
    # one obstacle with a prediction (it drives 3 m per sample along its heading), the others without
    first.update_at_timestep(0)
    p0, yaw = np.asarray(first.current_pos), float(first.current_orientation)
    L = 12
    pos = p0[None] + 3.0 * np.arange(L)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    preds = {first.obstacle_id: {"pos_list": pos, "orientation_list": np.full(L, yaw), "v_list": np.full(L, 30.0),
                                 "cov_list": np.tile(np.eye(2) * 0.1, (L, 1, 1)),
                                 "shape": {"length": first.length, "width": first.width}}}
    fo.evaluate_scenario(preds, ego[:2], float(ego[2]), (0.0, 0.0), float(ego[3]), 0, None)
    torch_cuda.cuda.synchronize()
    out = {}
    for occ in ("now", "predicted", "scenario"):
        out[occ] = fo.future_visibility(traj, t_stride=5, n_rays=256, fov="sensor", occluders=occ)
    torch_cuda.cuda.synchronize()
    for v in out.values():
        assert v.revealed.shape == (16, 7) and v.revealed_new.shape == (16, 7) and v.revealed_any.shape == (16,)
    assert out["scenario"].slice_timesteps == [0, 5, 10, 15, 20, 25, 30]
    # the predicted slices against the checker with the packing of the predictions dict
    corn, flags = fo.fo_obstacles.predicted_rows(preds, [5 * k for k in range(7)])
    assert not np.array_equal(corn[0, 0], corn[3, 0]) and np.array_equal(corn[0, 1], corn[3, 1])
    th = traj["theta"][:, ::5]
    head = np.stack((np.cos(th), np.sin(th)), -1)
    sm = fo.sensor_model
    r, a, n, an = _ref(sm, traj, 5, corn, flags, fov=120.0, n_rays=256, heading=head)
    assert np.array_equal(_np(out["predicted"].revealed), r) and np.array_equal(_np(out["predicted"].revealed_new), n)
    # M = 0
    e = fo.future_visibility({k: v[:0] for k, v in traj.items()}, t_stride=5)
    assert e.revealed.shape == (0, 7) and e.revealed_any.shape == (0,)
    e = fo.future_visibility([], t_stride=5)
    assert e.revealed.shape[0] == 0
    # refusals
    with pytest.raises(RuntimeError):
        sm.future_visibility_ex(traj["x"], traj["y"], None, fov=120.0)       # a sector fan without headings
    with pytest.raises(RuntimeError):
        sm.future_visibility_ex(traj["x"], traj["y"], n_rays=769)
    with pytest.raises(ValueError):
        fo.future_visibility(traj, occluders="tomorrow")
    c1, f1 = fo.fo_obstacles.rows_at([0])
    occ = sm.occluded_cells().cpu().numpy()
    with pytest.raises(RuntimeError, match="n_slices"):
        _raw_call(torch_cuda, sm, traj, 5, 192, 360.0, None, c1, f1, occ, n_slices=0)
    with pytest.raises(RuntimeError, match="window"):
        _raw_call(torch_cuda, sm, traj, 5, 192, 360.0, None, c1, f1, occ, win=(400, 400), first_seen=True)
    ok = _raw_call(torch_cuda, sm, traj, 5, 192, 360.0, None, c1, f1, occ, win=(400, 400))     # no first-seen: any window
    assert ok[0].shape == (16, 7)


def test_city_grid_at_full_size_with_every_option(torch_cuda):
    """10 000 trajectories x 7 poses x 720 rays, moving slices (the parked cars shuffled along their lanes), a 120 deg
    sensor and first-seen outputs: runs, and 64 sampled rows equal the checker"""
    from frenetix_occlusion import synthetic as SY
    sc = _load("city")
    ego = sc.ego_initial
    sm, ob = _scene(sc, ego)
    M, stride, K = 10000, 5, 7
    traj = SY.make_trajectories(M, 31, 0.1, seed=20240134, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    c0, _, f0 = ob.arrays()
    rng = np.random.default_rng(3)
    shift = rng.uniform(-2.0, 2.0, size=(K, len(f0), 1, 2))
    shift[0] = 0.0
    corn = c0[None] + np.cumsum(shift, axis=0)
    flags = np.repeat(f0[None], K, axis=0)
    flags[3:, ::5] = 0                        # every fifth car leaves
    fv = sm.future_visibility_ex(traj["x"], traj["y"], traj["theta"], t_stride=stride, n_rays=720, fov=120.0,
                                 occluders=(corn, flags), first_seen=True)
    torch_cuda.cuda.synchronize()
    rows = rng.choice(M, 64, replace=False)
    th = traj["theta"][:, ::stride]
    head = np.stack((np.cos(th), np.sin(th)), -1)
    r, a, n, an = _ref(sm, traj, stride, corn, flags, fov=120.0, n_rays=720, heading=head, rows=rows)
    assert np.array_equal(_np(fv.revealed)[rows], r) and np.array_equal(_np(fv.revealed_new)[rows], n)
    assert np.array_equal(_np(fv.revealed_any)[rows], an)
    np.testing.assert_allclose(_np(fv.area)[rows], a, rtol=1e-12, atol=1e-9)
    assert int(fv.revealed_any.max()) > 0
