"""The BASELINE.json configurations as parity cases on a real MI355X (configs[2] is the bench line; the others are
exercised here): each runs through FOInterface -- visibility, phantom sampling, batched assessment -- and is compared
with the oracle fed with the same phantom predictions."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLS = ("wttc", "min_dce", "max_ego_risk_all", "max_obst_risk_all", "max_ego_harm_all", "max_obst_harm_all",
        "max_collision_probability_all", "max_obst_harm_with_cp_all", "min_ttce", "argmin_dce", "argmin_ttc", "safe")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


def _interface(tmp_path, scenario_file, ego, metrics=None, thresholds=None, spawn=None, name="occ.yaml", share=None):
    import yaml
    from frenetix_occlusion import interface
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion import synthetic as SY
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
        cfg["accelerator"]["spawn"]["mode"] = "cells"   # the BASELINE-config sampler (the YAML default is the reference's rule families)
    if metrics:
        cfg["metrics"]["activated_metrics"] = list(metrics)
    if thresholds:
        cfg["metrics"]["metric_thresholds"].update(thresholds)
    if spawn:
        cfg["accelerator"]["spawn"].update(spawn)
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    sc = S.load_geometry_npz(os.path.join(GOLDEN, scenario_file))
    ego = sc.ego_initial if ego is None else np.asarray(ego, dtype=np.float64)
    ref_path = ego[None, :2] + np.linspace(0.0, 80.0, 81)[:, None] * np.array([[math.cos(ego[2]), math.sin(ego[2])]])
    v = SY.VEHICLE_BMW320I
    veh = SimpleNamespace(length=v[0], width=v[1], wb_rear_axle=v[2], mass=v[3], a_max=v[4])
    return interface.FOInterface(sc, ref_path, veh, 0.1, config_path=str(p), share_map_with=share), sc, ego, SY


def _agents_of(fo):
    arrs = fo.agent_manager.sweep_arrays()
    return dict(zip(("pos", "yaw", "v", "cov", "shape", "raw_dims", "type", "len"), [t.cpu().numpy() for t in arrs]))


def _compare_cost(oracle, got, ref):
    for name in COLS:
        a, b = ref[:, oracle.COST[name]], got[:, oracle.COST[name]]
        assert np.array_equal(np.isinf(a), np.isinf(b)), name
        f = np.isfinite(a)
        np.testing.assert_allclose(b[f], a[f], rtol=0, atol=1e-9, err_msg=name)


def test_config1_scenario1_default_sampling_hr_ttc(torch_cuda, oracle, tmp_path):
    """configs[0]: scenario1, ~200 candidate trajectories, activated metrics ['hr', 'ttc'] (=> cp, dce, ttc, hr)."""
    thr = {"harm": 0.1, "risk": 1}
    fo, sc, ego, SY = _interface(tmp_path, "scenario1_geometry.npz", None, metrics=("hr", "ttc"), thresholds=thr)
    for timestep in (0, 5):
        e = ego.copy()
        e[0] += 0.7634 * timestep * math.cos(e[2])
        e[1] += 0.7634 * timestep * math.sin(e[2])
        fo.evaluate_scenario({}, e[:2], float(e[2]), (0.0, 0.0), float(e[3]), timestep, None)
        assert len(fo.spawn_points) > 0
        traj = SY.make_trajectories(200, seed=7 + timestep, ego_pos=e[:2], ego_yaw=float(e[2]))
        ba = fo.trajectory_safety_assessment_batch(traj, mode="pair")
        torch_cuda.cuda.synchronize()
        ref = oracle.sweep(traj, _agents_of(fo), SY.VEHICLE_BMW320I, 0.1, metrics=("hr", "ttc"), thr=thr, want_lists=False)
        got = ba.cost.cpu().numpy()
        _compare_cost(oracle, got, ref["cost"])
        assert np.array_equal(ba.safe.cpu().numpy(), ref["safe"])
        assert np.isnan(ba.result.pair_f[oracle.PF["ttce"]].cpu().numpy()).all()       # ttce was not activated


def test_config2_scenario1_2k_x_32_full_metric_set(torch_cuda, oracle, tmp_path):
    """configs[1]: scenario1, 2 000 trajectories x 32 phantom predictions, the default six metrics."""
    thr = {"harm": 0.1, "risk": 1}
    fo, sc, ego, SY = _interface(tmp_path, "scenario1_geometry.npz", None, thresholds=thr,
                                 spawn=dict(max_agents=32, all_occluded=True, max_dist=40.0))
    fo.evaluate_scenario({}, ego[:2], float(ego[2]), (0.0, 0.0), float(ego[3]), 0, None)
    assert len(fo.spawn_points) == 32
    kinds = {sp.agent_type for sp in fo.spawn_points}
    assert kinds == {"Pedestrian", "Bicycle", "Car"}
    traj = SY.make_trajectories(2000, seed=2, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    ba = fo.trajectory_safety_assessment_batch(traj, mode="full")
    torch_cuda.cuda.synchronize()
    ref = oracle.sweep(traj, _agents_of(fo), SY.VEHICLE_BMW320I, 0.1, thr=thr, nthreads=8)
    _compare_cost(oracle, ba.cost.cpu().numpy(), ref["cost"])
    assert np.array_equal(ba.safe.cpu().numpy(), ref["safe"])
    lists = ba.result.lists.permute(3, 1, 0, 2).cpu().numpy()
    assert np.array_equal(np.isnan(lists), np.isnan(ref["lists"]))
    f = np.isfinite(ref["lists"])
    assert np.abs(lists[f] - ref["lists"][f]).max() < 1e-9
    tdce = ba.result.pair_i.permute(2, 1, 0).cpu().numpy()[..., oracle.PI["time_dce"]]
    assert np.array_equal(tdce, ref["pair_i"][..., oracle.PI["time_dce"]])
    assert 0 < ref["safe"].mean() < 1


def test_config5_multi_ego_four_interfaces_share_the_gpu(torch_cuda, oracle, tmp_path):
    """configs[4]: 4 egos x 2 000 trajectories on the scenario2/3 geometry, one FOInterface (one fo_ctx) per ego.
    The XMLs hold one planning problem each: three more ego poses are placed along lanelet centre lines."""
    from frenetix_occlusion import scenario as S
    sc0 = S.load_geometry_npz(os.path.join(GOLDEN, "scenario2_geometry.npz"))
    poses = [sc0.ego_initial.copy()]
    for ll in sc0.lanelets:
        c = ll.center
        if len(c) >= 4 and len(poses) < 4:
            i = len(c) // 3
            yaw = math.atan2(c[i + 1, 1] - c[i, 1], c[i + 1, 0] - c[i, 0])
            poses.append(np.array([c[i, 0], c[i, 1], yaw, 6.0]))
    assert len(poses) == 4
    thr = {"harm": 0.1, "risk": 1}
    egos = []
    for i, p in enumerate(poses):    # egos 0/2 plan on scenario 2, egos 1/3 on scenario 3: the second of each pair reads
        share = egos[i - 2][0] if i >= 2 else None      # the first one's static map (one copy in HBM)
        egos.append(_interface(tmp_path, "scenario2_geometry.npz" if i % 2 == 0 else "scenario3_geometry.npz", p,
                               thresholds=thr, spawn=dict(max_agents=16, all_occluded=True, max_dist=40.0),
                               name=f"occ{i}.yaml", share=share))
    assert egos[2][0].sensor_model.map_geometry is egos[0][0].sensor_model.map_geometry
    results = []
    for fo, sc, ego, SY in egos:          # all four steps are queued before anything is read back
        fo.evaluate_scenario({}, ego[:2], float(ego[2]), (0.0, 0.0), float(ego[3]), 0, None)
        traj = SY.make_trajectories(2000, seed=11, ego_pos=ego[:2], ego_yaw=float(ego[2]))
        results.append((traj, fo.trajectory_safety_assessment_batch(traj, mode="reduced")))
    torch_cuda.cuda.synchronize()
    n_with_agents = 0
    for (fo, sc, ego, SY), (traj, ba) in zip(egos, results):
        if ba is None:                    # an ego pose without occluded cells ahead: nothing to assess (metric.py:44-45)
            assert not fo.agent_manager.has_phantoms()
            continue
        n_with_agents += 1
        sub = {k: v[:300] for k, v in traj.items()}
        ref = oracle.sweep(sub, _agents_of(fo), SY.VEHICLE_BMW320I, 0.1, thr=thr, want_lists=False, nthreads=8)
        _compare_cost(oracle, ba.cost.cpu().numpy()[:300], ref["cost"])
    assert n_with_agents >= 2


@pytest.mark.parametrize("lists", ["f64", "f32", "f32x"])
def test_config3_headline_step_full_outputs_vs_oracle_on_every_pair(torch_cuda, oracle, lists):
    """configs[2] exactly as bench.py times it -- urban grid, 720 rays, fo_scene_spawn of 256 phantoms (all_occluded,
    max_dist 45), fo_sweep_run with full outputs on 10 000 candidates -- against the oracle on ALL 10 000 x 256 pairs
    (chunked: the oracle's lists for the whole batch would be 3 GB of host memory).  Float outputs <= 1e-9 (float32
    lists <= 1e-6), time_dce / argmin / argmax indices / safe exact (plateau rule of oracle/fo_compare.py).
    `f32x` is the format bench.py defaults to -- the headline: float64 arithmetic for every list entry, float32 elements in
    memory -- and is held to 1e-9 on the float64 value BEHIND each entry (the deviation from the oracle beyond half a float32
    ulp of the oracle's value, `list_err_beyond_f32_rounding`; the tolerance of _assert_rounded_float64 in test_sweep_gpu)."""
    import yaml
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import interface
    from frenetix_occlusion import scenario as SC
    from frenetix_occlusion import synthetic as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.sweep import MetricSweep
    from oracle import fo_compare as CMP
    M, A, T = 10000, 256, 31
    thr = {"harm": 0.1, "risk": 1}
    ctx = N.Context(0)
    sc = SC.synthetic_urban_grid()
    ego = sc.ego_initial
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
        cfg["accelerator"]["spawn"]["mode"] = "cells"   # the BASELINE-config sampler (the YAML default is the reference's rule families)
    cfg["accelerator"]["spawn"].update(max_agents=A, all_occluded=True, max_dist=45.0)
    ref_path = ego[None, :2] + np.linspace(0.0, 80.0, 81)[:, None] * np.array([[math.cos(ego[2]), math.sin(ego[2])]])
    sm = SensorModel(sc.lanelets, ref_path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, cell_size=0.5, ctx=ctx)
    sm.upload_obstacles(sc.obstacle_arrays(0)[:3])
    sl = SpawnLocator(None, ref_path, cfg, sm, dt=0.1, horizon=(T - 1) * 0.1)
    sw = MetricSweep(S.VEHICLE_BMW320I, 0.1, thresholds=thr, ctx=ctx)
    traj = S.make_trajectories(M, T, 0.1, seed=20240131 + 3, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    sm.launch(ego[:2], float(ego[2]))
    batch = sl.sample(ego[:2], float(ego[2]), float(ego[3]))
    sw.set_agents(*batch.sweep_args())
    out = sw.run(traj["x"], traj["y"], traj["theta"], traj["v"], traj["a"], mode="full", lists=lists)
    torch.cuda.synchronize()
    agents = {k: getattr(batch, k).cpu().numpy() for k in ("pos", "yaw", "v", "cov", "shape", "raw_dims", "type", "len")}
    assert int((agents["len"] > 0).sum()) == A
    views, acc, bufs = out.list_views(), None, None
    for lo in range(0, M, 500):
        hi = lo + 500
        ref = oracle.sweep({k: v[lo:hi] for k, v in traj.items()}, agents, S.VEHICLE_BMW320I, 0.1, thr=thr, nthreads=8, out=bufs)
        bufs = ref
        got = {"cost": out.cost[lo:hi].cpu().numpy(), "safe": out.safe[lo:hi].cpu().numpy(),
               "pair_f": out.pair_f[:, :, lo:hi].permute(2, 1, 0).cpu().numpy(),
               "pair_i": out.pair_i[:, :, lo:hi].permute(2, 1, 0).cpu().numpy(),
               "lists": torch.stack([v[:, :, lo:hi] for v in views]).permute(3, 1, 0, 2).cpu().numpy()}
        acc = CMP.merge(acc, CMP.compare(ref, got))
    assert acc["pairs"] == M * A
    assert acc["int_mismatches"] == 0 and acc["pattern_mismatches"] == 0, acc
    assert acc["float_max_abs_err"] <= 1e-9, acc
    if lists == "f32x":
        assert out.lists.dtype == torch.float32
        assert acc["list_err_beyond_f32_rounding"] <= 1e-9, acc      # the float64 result behind every entry
        assert acc["list_max_abs_err"] <= 6.1e-8, acc                 # and no entry further off than half a float32 ulp of 1
    else:
        assert acc["list_max_abs_err"] <= (1e-6 if lists == "f32" else 1e-9), acc
    # the batch exercises every branch: pairs inside the 5 m gate, colliding pairs, both verdicts
    pf = out.pair_f
    assert float((pf[N.PF["max_collision_probability"]] > 0).double().mean()) > 0.02
    assert float((pf[N.PF["dce"]] == 0).double().mean()) > 0.001
    assert 0.0 < float(out.safe.double().mean()) < 1.0


def test_failed_planning_step_leaves_no_half_written_agent_set(torch_cuda):
    """fo_step_run announces the agent set to the sweep before the scene kernels write it (the prediction kernel fills the
    table); when the scene stage fails, a sweep that follows must not read that table: it evaluates no agents."""
    import yaml
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import interface
    from frenetix_occlusion import scenario as SC
    from frenetix_occlusion import synthetic as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.step import PlanningStep
    from frenetix_occlusion.sweep import MetricSweep
    M, A, T = 300, 8, 31
    sc = SC.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    ego0 = sc.ego_initial
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
        cfg["accelerator"]["spawn"]["mode"] = "cells"   # the BASELINE-config sampler (the YAML default is the reference's rule families)
    cfg["accelerator"]["spawn"].update(max_agents=A, all_occluded=True)
    yaw0 = float(ego0[2])
    ref = ego0[None, :2] + np.linspace(0.0, 80.0, 81)[:, None] * np.array([[math.cos(yaw0), math.sin(yaw0)]])
    traj = S.make_trajectories(M, T, 0.1, seed=5, ego_pos=ego0[:2], ego_yaw=yaw0)
    ctx = N.Context(0)
    sm = SensorModel(sc.lanelets, ref, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, cell_size=0.5, ctx=ctx)
    sm.upload_obstacles(sc.obstacle_arrays(0)[:3])
    sl = SpawnLocator(None, ref, cfg, sm, dt=0.1, horizon=(T - 1) * 0.1)
    sw = MetricSweep(S.VEHICLE_BMW320I, 0.1, thresholds={"harm": 0.1, "risk": 1}, ctx=ctx)
    tr = [torch.as_tensor(traj[k]).cuda() for k in ("x", "y", "theta", "v", "a")]
    ps = PlanningStep(sm, sl, sw, *tr, mode="reduced")
    out = ps.run(ego0[:2], yaw0, 5.0)
    torch.cuda.synchronize()
    assert int(sl.batch.n.item()) > 0 and not bool(out.safe.bool().all())     # phantoms, and some candidate is unsafe
    ps._s.n_path = 1                                                             # fo_scene_spawn rejects a one-point path
    with pytest.raises(RuntimeError):
        ps.run(ego0[:2], yaw0, 5.0)
    res = sw.run(*tr, mode="reduced")
    torch.cuda.synchronize()
    assert bool(res.safe.bool().all())                                           # no agents evaluated


@pytest.mark.parametrize("routes,footprint", [(0, "polygon"), (2, "circle")])
def test_planning_step_in_one_native_call_equals_the_stage_calls(torch_cuda, routes, footprint):
    _planning_step_in_one_native_call_equals_the_stage_calls(torch_cuda, routes, footprint, 31)


@pytest.mark.parametrize("T", [64, 65, 130])
@pytest.mark.parametrize("routes,footprint", [(0, "polygon"), (2, "circle")])
def test_planning_step_in_one_native_call_equals_the_stage_calls_at_long_horizons(torch_cuda, routes, footprint, T):
    _planning_step_in_one_native_call_equals_the_stage_calls(torch_cuda, routes, footprint, T)


def _planning_step_in_one_native_call_equals_the_stage_calls(torch_cuda, routes, footprint, T):
    """fo_step_run / PlanningStep (one FFI crossing per planning step, eight launches: the fan and the tile table inside the ray kernel, the
    candidate flags inside the first compaction, the agent table written by the prediction kernel) gives the bits of the
    five stage calls: cost vectors, flags, pair scalars, phantom set and cell classes, over several ego poses (window
    origin, spawn range and heading change from step to step); with and without route predictions (R slots per
    phantom), polygonal and circular sensor footprint (range and half-fan tables written or not).  Horizons of 64 / 65 / 130
    samples, with the full per-step lists: beyond 64 samples the prediction kernel reads its own predictions back for the agent
    table's rows instead of writing them from registers (tests/test_rules_step_gpu.py has the rule stage's half)"""
    import yaml
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import interface
    from frenetix_occlusion import scenario as SC
    from frenetix_occlusion import synthetic as S
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.spawn_locator import SpawnLocator
    from frenetix_occlusion.step import PlanningStep
    from frenetix_occlusion.sweep import MetricSweep
    M, A = (2000 if T == 31 else 256), 32
    out_mode = "pair" if T == 31 else "full"
    sc = SC.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    ego0 = sc.ego_initial
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
        cfg["accelerator"]["spawn"]["mode"] = "cells"   # the BASELINE-config sampler (the YAML default is the reference's rule families)
    cfg["accelerator"]["spawn"].update(max_agents=A // max(routes, 1), all_occluded=True, routes=routes)
    if routes:
        cfg["accelerator"]["spawn"]["pattern"] = ["Car", "Bicycle", "Pedestrian", "Car"]
    yaw0 = float(ego0[2])
    ref = ego0[None, :2] + np.linspace(0.0, 80.0, 81)[:, None] * np.array([[math.cos(yaw0), math.sin(yaw0)]])
    traj = S.make_trajectories(M, T, 0.1, seed=5, ego_pos=ego0[:2], ego_yaw=yaw0)
    results = {}
    for how in ("stages", "one-call"):
        ctx = N.Context(0)
        sm = SensorModel(sc.lanelets, ref, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, cell_size=0.5, ctx=ctx,
                         routes=routes, footprint=footprint)
        sm.upload_obstacles(sc.obstacle_arrays(0)[:3])
        sl = SpawnLocator(None, ref, cfg, sm, dt=0.1, horizon=(T - 1) * 0.1 + 0.05)
        assert sl.R == max(routes, 1) and sl.T == T
        sw = MetricSweep(S.VEHICLE_BMW320I, 0.1, thresholds={"harm": 0.1, "risk": 1}, ctx=ctx)
        tr = [torch.as_tensor(traj[k]).cuda() for k in ("x", "y", "theta", "v", "a")]
        ps = PlanningStep(sm, sl, sw, *tr, mode=out_mode) if how == "one-call" else None
        got = []
        for i in range(4):
            ego = ego0[:2] + 1.3 * i * np.array([math.cos(yaw0), math.sin(yaw0)])
            yaw, v = yaw0 + 0.02 * i + (0.33 if i == 3 else 0.0), 5.0 + 2.0 * i
            if ps is not None:
                out = ps.run(ego, yaw, v)
            else:
                sm.launch(ego, yaw)
                sw.set_agents(*sl.sample(ego, yaw, v).sweep_args(), check=False)
                out = sw.run(*tr, mode=out_mode)
            torch.cuda.synchronize()
            # (the fan tables too: the one-call step writes them inside the ray kernel, whose workgroups may be a single wave
            # -- a table left partly unwritten would only show at the few rim cells that consult it)
            fan_d, fan_r, fan_h = sm._fan_buffers()
            tables = np.concatenate([t.cpu().numpy().ravel() for t in ([fan_d, fan_r, fan_h] if footprint == "polygon" else [fan_d])])
            got.append((out.cost.cpu().numpy().copy(), out.safe.cpu().numpy().copy(), out.pair_f.cpu().numpy().copy(),
                        sm.cell_class.cpu().numpy().copy(), sl.batch.pos.cpu().numpy().copy(), int(sl.batch.n.item()), tables)
                       + ((out.lists_raw.cpu().numpy().copy(), sl.batch.len.cpu().numpy().copy(), sl.batch.yaw.cpu().numpy().copy(),
                           sl.batch.v.cpu().numpy().copy(), out.pair_i.cpu().numpy().copy()) if T != 31 else ()))
        results[how] = got
    for a, b in zip(results["stages"], results["one-call"]):
        assert a[5] == b[5] and a[5] > 0
        for x, y in zip(a[:5] + a[6:], b[:5] + b[6:]):
            assert np.array_equal(x, y, equal_nan=True)
    assert not np.array_equal(results["stages"][0][3], results["stages"][3][3])      # the steps did differ


def test_one_call_step_equals_the_stage_calls_over_random_poses(torch_cuda, monkeypatch, capsys):
    """a short run of tools/step_soak.py (random positions, headings and speeds along scenario 1; seed 9 holds the pose
    that exposed the partly written half-fan table of the one-wave ray workgroups): every output bit for bit"""
    import runpy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(sys, "argv", ["step_soak.py", "40", "9"])
    runpy.run_path(os.path.join(root, "tools", "step_soak.py"), run_name="__main__")
    assert "agree bit for bit" in capsys.readouterr().out
