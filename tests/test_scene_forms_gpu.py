"""Every form of the scene stage (csrc/fo_scene.hip) at its switch points, bit-exact against the CPU oracle: one- and five-wave
ray / settle kernels with and without a hole-skip table, the one- and two-launch compaction.  The scenes and the host rules
that pick the form are in tests/scene_forms.py; tests/test_scene_forms_cpu.py shows on the oracle alone that every scene is
what it is meant to be.  Each test asserts the form it means to run (expected_form on the sizes the device side reports), so
a scene that drifts off its switch point fails instead of testing nothing.  Needs a real MI355X: `pytest -m gpu`."""
import math
import os

import numpy as np
import pytest

import ref_occlusion_memory as OM
import ref_occlusion_memory_road as OMR
import scene_forms as F
from test_scene_gpu import _check_step

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUFFERS = ("range", "hit_id", "ring", "cell_class", "occluded", "visible", "spawn_cell")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


def _form_of(st, forced):
    return F.expected_form(st["E"], st["O"], st["skip_passed"], st["nx"] * st["ny"], forced)


def _in_both_shapes(monkeypatch, run, want):
    """run() -> _check_step's dict, once as the library picks the wave shape and once forced to five waves; want = the form
    (NW, SKIP, two_launch) of the library's choice.  Both equal the oracle (inside run); here: the form each ran in, and
    the device buffers of the two equal to each other."""
    got = {}
    for name, env in F.SCENE_FORMS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            st = run()
        assert _form_of(st, bool(env)) == ((5,) + want[1:] if env else want), name
        got[name] = st
    a, b = got["library"], got["five_waves"]
    for k in BUFFERS:
        assert np.array_equal(a["got"][k], b["got"][k]), k
    return a


# ------------------------------------------------------------------------------------------------ 1. trusted scenes, both shapes
def _scenario(k):
    from frenetix_occlusion import scenario as S
    return S.load_geometry_npz(os.path.join(GOLDEN, f"scenario{k}_geometry.npz"))


@pytest.mark.parametrize("timestep", [0, 25])
def test_scenario1_in_both_wave_shapes(torch_cuda, oracle, monkeypatch, timestep):
    sc = _scenario(1)
    ego = sc.ego_initial.copy()
    ego[:2] += 0.7 * timestep * np.array([math.cos(ego[2]), math.sin(ego[2])])
    st = _in_both_shapes(monkeypatch, lambda: _check_step(torch_cuda, oracle, sc, ego, 7.63, timestep),
                         (1, timestep == 0, False))
    assert st["n_occ"] > 0 and st["n_exact"] > 20
    if timestep == 0:
        assert st["skipped"] == 7      # <true, 5> has the sliver hole's seven pieces to leave out


def test_scenario3_and_odd_fans_in_both_wave_shapes(torch_cuda, oracle, monkeypatch):
    sc3, sc1 = _scenario(3), _scenario(1)
    _in_both_shapes(monkeypatch, lambda: _check_step(torch_cuda, oracle, sc3, sc3.ego_initial, float(sc3.ego_initial[3]), 0),
                    (1, False, False))
    _in_both_shapes(monkeypatch, lambda: _check_step(torch_cuda, oracle, sc1, sc1.ego_initial, 7.63, 0, sensor_angle=90.0,
                                                     n_rays=181, radius=30.0), (1, False, False))
    _in_both_shapes(monkeypatch, lambda: _check_step(torch_cuda, oracle, sc1, sc1.ego_initial, 7.63, 3, sensor_angle=360.0,
                                                     n_rays=97, radius=25.0, max_agents=5), (1, False, False))


def test_obstacle_scenes_in_both_wave_shapes(torch_cuda, oracle, monkeypatch):
    """the obstacle lit between its probe points, and the bicycle in front of the ego (tests/test_scene_gpu.py)"""
    from frenetix_occlusion import scenario as S
    xs = np.linspace(-5.0, 40.0, 2)
    room = S.Lanelet(1, np.stack((xs, np.full(2, 15.0)), -1), np.stack((xs, np.full(2, -15.0)), -1))
    mk = lambda i, x, y, l, w: S.Obstacle(i, "static", "car", l, w, 0, np.array([x, y, 0.0, 0.0]), np.zeros((0, 4)))
    sc = S.Scenario(0.1, [room], [mk(1, 30, 0, 2.0, 20.0), mk(2, 10, -3.3, 1.0, 1.2), mk(3, 10, 0.0, 1.0, 1.0),
                                  mk(4, 10, 3.3, 1.0, 1.2)])
    st = _in_both_shapes(monkeypatch, lambda: _check_step(torch_cuda, oracle, sc, np.array([0.0, 0.0, 0.0, 5.0]), 5.0, 0),
                         (1, False, False))
    assert st["got"]["visible"].tolist() == [1, 1, 1, 1]
    sc1 = _scenario(1)
    sc1.obstacles = [S.Obstacle(555, "static", "bicycle", 2.0, 0.9, 0, np.array([8.0, 0.0, 0.0, 0.0]), np.zeros((0, 4)))]
    st = _in_both_shapes(monkeypatch, lambda: _check_step(torch_cuda, oracle, sc1, sc1.ego_initial, 7.63, 0), (1, True, False))
    assert (st["got"]["hit_id"] < st["E"]).all() and st["got"]["visible"].tolist() == [1]


# ------------------------------------------------------------------------------------------------ 2. the one-wave rule's boundary
@pytest.mark.parametrize("name", list(F.L_ROADS))
def test_piece_counts_around_64_chunks(torch_cuda, oracle, monkeypatch, name):
    n_main, E, chunks, ego = F.L_ROADS[name]
    sc = F.scene(F.l_road(n_main))
    ego = np.array(ego + (5.0,))
    run = lambda: _check_step(torch_cuda, oracle, sc, ego, 5.0, 0)
    if chunks <= 64:                       # legal in both shapes
        st = _in_both_shapes(monkeypatch, run, (1, False, False))
    else:                                  # the library picks five waves itself
        st = run()
        assert _form_of(st, False) == (5, False, False)
    assert st["E"] == E and F.n_chunks(st["E"]) == chunks
    assert st["hit_max"] // 64 == chunks - 1          # rays end on pieces of the last chunk
    assert st["n_occ"] > 0 and st["n_exact"] > 0
    if chunks > 320:
        assert F.second_trip_waves(st["got"]["hit_id"], st["E"]) == set(range(5))    # hits in every wave's second trip


@pytest.mark.parametrize("shadow_length", [100.0, math.inf])
@pytest.mark.parametrize("radius", list(F.FRAME_RADII))
@pytest.mark.parametrize("O", [16, 17])
def test_sixteen_and_seventeen_obstacles(torch_cuda, oracle, monkeypatch, O, radius, shadow_length):
    """16 obstacles: the last one-wave count; 17: five waves on a map of two chunks.  Overlapping skins, a bicycle, an absent
    obstacle, obstacles seen by their probes only; with the block transparent (hole-skip table) and occluding."""
    sc = F.scene(F.frame_map(), F.frame_obstacles(O))
    run = lambda: _check_step(torch_cuda, oracle, sc, F.FRAME_EGO, 5.0, 0, n_rays=F.FRAME_RAYS, radius=radius,
                              shadow_length=shadow_length)
    skip = F.FRAME_RADII[radius]
    if O <= 16:
        st = _in_both_shapes(monkeypatch, run, (1, skip, False))
    else:
        st = run()
        assert _form_of(st, False) == (5, skip, False)
    assert st["O"] == O and (st["skipped"] > 0) == skip and st["n_exact"] > 0
    vis, hid = st["got"]["visible"], st["got"]["hit_id"]
    by_ray = set((hid[hid >= st["E"]] - st["E"]).tolist())
    assert by_ray and any(vis[o] and o not in by_ray for o in range(O)) and not vis[3]


# ------------------------------------------------------------------------------------------------ 3. the two-launch compaction
def _oracle_of(oracle, sm, geo, obstacles, ego, timestep=0):
    """the oracle's step for what `sm` has just run, fed the fan the device wrote"""
    fan = tuple(t.cpu().numpy() for t in (sm.dirs, sm.rmax, sm.half_dirs))
    return F.oracle_step(oracle, geo, obstacles, ego, timestep=timestep, n_rays=sm.n_rays, radius=sm.sensor_radius, fan=fan)


def _equals_oracle(torch, sm, s):
    """the buffers of the step `sm` has just run against s: an oracle_step, or the hit_id / cls / occ a _check_step has shown
    equal to the oracle's for the same call"""
    torch.cuda.synchronize()
    w = sm.window
    assert (w.nx, w.ny) == (s["n"], s["n"]) and ("frame" not in s or (w.ix0, w.iy0) == s["frame"][2:])
    cls = sm.cell_class.cpu().numpy()
    assert np.array_equal(sm.hit_id.cpu().numpy(), s["hid"]) and np.array_equal(cls, s["cls"])
    occ = sm.occluded_cells().cpu().numpy()
    assert np.array_equal(occ, s["occ"]) and np.array_equal(occ, np.flatnonzero(cls.reshape(-1) & 4))
    assert int(sm.n_occluded.item()) == len(s["occ"])


def _large_small_large(torch, oracle, sc, radius, n_rays, st):
    """one sensor model: the large window, then a small one, then the large one again.  The scan kernel rewrites the block
    counts in place; nothing of that may reach the next step.  st: _check_step's dict of the large window (device == oracle
    shown there, so its buffers stand for the oracle's)"""
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    sm = SensorModel(sc.lanelets, None, sensor_radius=radius, sensor_angle=360.0, n_rays=n_rays)
    obst = FOObstacles(sc.obstacles)
    obst.update(0)
    ego = np.asarray(sc.ego_initial, dtype=np.float64)
    large = dict(n=st["nx"], hid=st["got"]["hit_id"], cls=st["got"]["cell_class"], occ=st["got"]["occluded"])
    for r in (radius, 20.0, radius):
        sm.sensor_radius = r
        sm.calc_visible_and_occluded_area(0, ego[:2], float(ego[2]), obst)
        _equals_oracle(torch, sm, large if r == radius else _oracle_of(oracle, sm, sm.map_geometry, sc.obstacles, ego))


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("radius", list(F.LARGE_WINDOWS))
def test_windows_around_2048_compaction_blocks(torch_cuda, oracle, monkeypatch, radius, forced):
    """a window of 724 (2048 blocks: the last one-launch window), 725 and 901 cells per side without a hole-skip table; the
    candidate compaction of the cell sampler goes through the same compact() (checked by _check_step); then a small window
    on the same sensor model"""
    sc = F.large_window_scene(radius)
    n, nb = F.LARGE_WINDOWS[radius]
    if forced:
        monkeypatch.setenv("FO_SCENE_FIVE_WAVES", "1")
    st = _check_step(torch_cuda, oracle, sc, sc.ego_initial, float(sc.ego_initial[3]), 0, radius=radius, all_occluded=True)
    assert (st["nx"], st["ny"]) == (n, n) and F.n_blocks(n * n) == nb
    assert _form_of(st, forced) == (5 if forced else 1, False, nb > 2048)
    assert len(F.scan_rounds(st["got"]["occluded"])) >= 2 and st["n_cand"] > 0
    assert np.array_equal(st["got"]["occluded"], np.flatnonzero(st["got"]["cell_class"].reshape(-1) & 4))
    _large_small_large(torch_cuda, oracle, sc, radius, 720, st)


@pytest.mark.parametrize("O", [16, 17])
def test_hole_skip_table_in_the_first_two_launch_window(torch_cuda, oracle, monkeypatch, O):
    """SKIP with the scan + scatter compaction: the frame road in a window of 725 cells per side, whose footprint encloses
    the block.  16 obstacles as the library picks the wave shape (1, SKIP, two launches) and forced to five waves, 17 as
    the library picks it (5, SKIP, two launches)"""
    sc = F.scene(F.frame_map(), F.frame_obstacles(O))
    sc.ego_initial = F.FRAME_EGO
    run = lambda: _check_step(torch_cuda, oracle, sc, F.FRAME_EGO, 5.0, 0, n_rays=F.FRAME_RAYS, radius=F.FRAME_LARGE_RADIUS,
                              all_occluded=True)
    if O <= 16:
        st = _in_both_shapes(monkeypatch, run, (1, True, True))
    else:
        st = run()
        assert _form_of(st, False) == (5, True, True)
    assert (st["nx"], st["ny"]) == (725, 725) and st["O"] == O and st["skipped"] > 0 and st["n_exact"] > 0
    assert F.scan_rounds(st["got"]["occluded"]) == {0, 1} and st["n_cand"] > 0
    assert np.array_equal(st["got"]["occluded"], np.flatnonzero(st["got"]["cell_class"].reshape(-1) & 4))
    _large_small_large(torch_cuda, oracle, sc, F.FRAME_LARGE_RADIUS, F.FRAME_RAYS, st)


@pytest.mark.parametrize("metric", ["euclid", "road"])
def test_occlusion_memory_drive_in_the_first_two_launch_window(torch_cuda, oracle, metric):
    """three steps of the occlusion memory at the 725-cell window: its kernels lower the block counts the two-launch
    compaction then scans.  Classes, hidden set and the ascending index list against tests/ref_occlusion_memory*.py over the
    oracle's memoryless classes."""
    from frenetix_occlusion.sensor_model import SensorModel
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    sc = _scenario(2)
    radius = 120.6
    sm = SensorModel(sc.lanelets, None, sensor_radius=radius, sensor_angle=360.0, n_rays=720)
    sm.enable_occlusion_memory(True, v_max=13.9, dt=0.1, metric=metric)
    ref = (OMR if metric == "road" else OM).Memory(13.9, 0.1, sm.cell_size)
    road = sm.road_raster()
    geo, ego0 = sm.map_geometry, sc.ego_initial
    obst = FOObstacles(sc.obstacles)
    cleared = 0
    for timestep in (0, 1, 3):
        ego = ego0.copy()
        ego[:2] += np.array([3.0, -1.0]) * timestep     # (the ego leaves the road: cells it saw fall into shadow and are cleared)
        obst.update(timestep)
        sm.upload_obstacles(obst)
        sm.launch(ego[:2], float(ego[2]), timestep=timestep)
        torch_cuda.cuda.synchronize()
        s = _oracle_of(oracle, sm, geo, sc.obstacles, ego, timestep)
        w = sm.window
        assert (w.nx, w.ny) == (725, 725) and F.expected_form(len(geo.edges), s["O"], False, w.nx * w.ny, False)[2]
        H, out, reason = ref.advance(s["cls"], (w.ix0, w.iy0, w.nx, w.ny), road, timestep)
        assert reason == sm.occlusion_memory_reset_reason and (reason is None) == (timestep > 0)
        cls = sm.cell_class.cpu().numpy()
        assert np.array_equal(cls, out) and np.array_equal(sm.occlusion_memory_hidden, H)
        occ = sm.occluded_cells().cpu().numpy()
        assert np.array_equal(occ, np.flatnonzero(out.reshape(-1) & 4)) and int(sm.n_occluded.item()) == len(occ)
        cleared += int(((s["cls"] & 4) != 0).sum()) - len(occ)
        assert F.scan_rounds(occ, 0) == {0, 1}
    assert cleared > 0          # the memory took cells out of the occluded set: the counts the scan reads were lowered


# ------------------------------------------------------------------------------------------------ 4. the fused step in every form
def _fused_settings():
    """name -> (lanelets, obstacles, intersections, ego (x, y, yaw, v), radius, rays, environment, form (NW, two_launch)): where
    the one-call step's own work differs by form -- the ray kernel writes the fan and the sweep's tile table in the one- or
    the five-wave shape (the host re-slices the table's horizon under one wave only), and the compaction flags the
    sampler's candidates itself or, in a large window, leaves that to a launch of its own"""
    sc1, sc2 = _scenario(1), _scenario(2)
    return {"scenario 1, forced five waves": (sc1.lanelets, sc1.obstacles, sc1.intersections, sc1.ego_initial, 50.0, 720,
                                              {"FO_SCENE_FIVE_WAVES": "1"}, (5, False)),
            "17 obstacles": (list(F.frame_lanelets()), F.frame_obstacles(17), None, F.FRAME_EGO, 50.0, F.FRAME_RAYS, {}, (5, False)),
            "window of 725 cells": (sc2.lanelets, sc2.obstacles, sc2.intersections, sc2.ego_initial, 120.6, 720, {}, (1, True))}


FUSED_BATCHES = [(T, M) for T in (1, 2, 3, 31) for M in (1, 65)]


@pytest.mark.parametrize("name", ["scenario 1, forced five waves", "17 obstacles", "window of 725 cells"])
def test_fused_step_equals_the_stage_calls_in_every_form(torch_cuda, monkeypatch, name):
    """fo_step_run against the stage calls queued one by one (the comparison of
    test_rules_step_gpu.py::test_one_call_step_with_rules_equals_the_stage_calls, with its helpers), bit for bit on the
    fan tables, ranges, hit ids, classes, occluded list, spawn cells, agents and sweep outputs -- two steps on one context
    with a heading jump of 1.1 rad between them, for candidate batches of T in {1, 2, 3, 31} samples and M in {1, 65}
    trajectories (spawn mode both: the sampler's cells and the rule families).  And the one-call step's cost / safe / pair
    outputs against fo_sweep_run over the same trajectories and the agents the step left on the context: that sweep writes
    its tile table itself, the step's was written by the ray kernel's spare workgroups."""
    from test_rules_step_gpu import _stack
    from frenetix_occlusion import synthetic as SY
    from frenetix_occlusion.step import PlanningStep
    torch = torch_cuda
    lanelets, obstacles, inter, ego0, radius, n_rays, env, (nw, two_launch) = _fused_settings()[name]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    ego0 = np.asarray(ego0, dtype=np.float64)
    yaw0, v_ego = float(ego0[2]), float(ego0[3])
    path = ego0[None, :2] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw0), math.sin(yaw0)]])
    poses = [(ego0[:2], yaw0), (ego0[:2] + 0.8 * np.array([math.cos(yaw0), math.sin(yaw0)]), yaw0 + 1.1)]
    stacks = {how: _stack(torch, lanelets, obstacles, path, inter, 0, M=65, T=31, mode="both", ego=ego0[:2], yaw=yaw0,
                          radius=radius, n_rays=n_rays) for how in ("stages", "one-call")}
    for k in stacks.values():
        k.sm.upload_obstacles(k.obs)
    # a planner's candidates start at the ego's pose: another batch per step, so that a tile-table row the step failed to
    # write holds the previous step's values, not by chance the right ones
    batches = []
    for i, (ego, yaw) in enumerate(poses):
        traj = SY.make_trajectories(65, 31, 0.1, seed=3 + i, ego_pos=ego, ego_yaw=yaw)
        batches.append([torch.as_tensor(traj[q]).cuda() for q in ("x", "y", "theta", "v", "a")])
    n_agents = n_cells = 0
    for T, M in FUSED_BATCHES:
        got = {}
        for how, k in stacks.items():
            tr = [q[:M, :T].clone() for q in batches[0]]             # (the step is bound to these tensors: refilled per step)
            ps = PlanningStep(k.sm, k.sl, k.sw, *tr, mode="pair") if how == "one-call" else None
            res = []
            for (ego, yaw), batch in zip(poses, batches):
                for q, src in zip(tr, batch):
                    q.copy_(src[:M, :T])
                if ps is not None:
                    out = ps.run(ego, yaw, v_ego)
                else:
                    k.sm.launch(ego, yaw)
                    k.sl.find_spawn_points(ego, yaw, None, v_ego, lazy=True)
                    k.sw.set_agents(*k.sl.batch.sweep_args(), check=False)
                    out = k.sw.run(*tr, mode="pair")
                torch.cuda.synchronize()
                sm, b, w = k.sm, k.sl.batch, k.sm.window
                form = F.expected_form(len(sm.map_geometry.edges), len(k.obs), sm.edge_skip is not None, w.nx * w.ny, bool(env))
                assert (form[0], form[2]) == (nw, two_launch), (name, how, form)
                live = (b.len.cpu().numpy() > 0)
                dirs, rmax, half = sm._fan_buffers()          # (both ways write the sensor model's own fan tables)
                r = dict(dirs=dirs, rmax=rmax, half=half, ring=sm._buf["ring"], range=sm.range, hit_id=sm.hit_id, cls=sm.cell_class,
                         occ=sm.occluded_cells(), n_occ=sm.n_occluded, cell=b.cell, n=b.n, len=b.len, type=b.type, head=b.head,
                         cost=out.cost, safe=out.safe, pair_f=out.pair_f, pair_i=out.pair_i)
                r = {q: t.cpu().numpy().copy() for q, t in r.items()}
                for q in ("pos", "yaw", "v", "cov"):                       # (rows of slots nobody spawned into are not written)
                    r[q] = getattr(b, q).cpu().numpy()[live].copy()
                if ps is not None:
                    ref = k.sw.run(*tr, mode="pair")
                    torch.cuda.synchronize()
                    for q in ("cost", "safe", "pair_f", "pair_i"):
                        assert np.array_equal(r[q], getattr(ref, q).cpu().numpy(), equal_nan=True), (name, T, M, q, "fo_sweep_run")
                    n_agents += int(live.sum())
                    n_cells += int(r["n"].sum())
                res.append(r)
            got[how] = res
        for step, (a, b_) in enumerate(zip(got["stages"], got["one-call"])):
            assert a.keys() == b_.keys()
            for q in a:
                assert np.array_equal(a[q], b_[q], equal_nan=True), (name, T, M, step, q)
        assert not np.array_equal(got["one-call"][0]["half"], got["one-call"][1]["half"])      # the heading did jump
    assert n_agents > 0 and n_cells > 0, (name, n_agents, n_cells)


# ------------------------------------------------------------------------------------------------ the form that actually ran
_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import os
import numpy as np, torch
import scene_forms as F
from frenetix_occlusion import scenario as S
from frenetix_occlusion.sensor_model import SensorModel
from frenetix_occlusion.utils.fo_obstacle import FOObstacles
sc2 = S.load_geometry_npz(os.path.join({tests!r}, "golden", "scenario2_geometry.npz"))
calls = [(F.l_road(F.L_ROADS[k][0]), [], np.array(F.L_ROADS[k][3]), 50.0, 720) for k in ("64 full chunks", "65 chunks")]
calls += [(F.frame_map(), F.frame_obstacles(O), F.FRAME_EGO, r, F.FRAME_RAYS) for O, r in ((16, 50.0), (17, 50.0), (16, 18.0), (17, 18.0))]
calls += [(sc2.lanelets, sc2.obstacles, sc2.ego_initial, r, 720) for r in (120.5, 120.6)]
calls += [(F.frame_map(), F.frame_obstacles(O), F.FRAME_EGO, F.FRAME_LARGE_RADIUS, F.FRAME_RAYS) for O in (16, 17)]
for net, obstacles, ego, r, n_rays in calls:
    sm = SensorModel(net, None, sensor_radius=r, sensor_angle=360.0, n_rays=n_rays)
    ob = FOObstacles(obstacles)
    ob.update(0)
    sm.calc_visible_and_occluded_area(0, ego[:2], float(ego[2]), ob)
    torch.cuda.synchronize()
    print("call", len(sm.map_geometry.edges), len(obstacles), int(sm.edge_skip is not None), sm.window.nx * sm.window.ny)
print("child ok")
'''


@pytest.mark.parametrize("form,env", F.SCENE_FORMS)
def test_kernel_trace_shows_the_form_the_host_rules_name(torch_cuda, tmp_path, monkeypatch, form, env):
    """expected_form restates the host rules; only the launches themselves say what the library ran.  Ten scene-stage
    calls on either side of every switch point under a kernel trace: the template arguments of the ray and settle kernels
    and the compaction kernels of each call are those expected_form names for the sizes the call reports.

    The trace names a kernel by its demangled signature, `void (anonymous namespace)::fo_rays_kernel<true, 5>(int, ...)`;
    the pattern below also takes the arguments written with their types, `<(bool)true, (int)5>`.  A name it does not match
    leaves the lists short, and the comparison with `want` fails."""
    import csv
    import glob
    import re
    import shutil
    import subprocess
    import sys
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    child = tmp_path / "child_forms.py"
    child.write_text(_TRACE_CHILD.format(root=root, pkg=os.path.join(root, "frenetix-occlusion_amd"), tests=tests))
    d = tmp_path / "trace"
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += [(int(q["Start_Timestamp"]), q["Kernel_Name"]) for q in csv.DictReader(fh)]
    names = [n for _, n in sorted(rows)]
    tpl = lambda kernel: [(m.group(1) == "true", int(m.group(2))) for n in names
                          for m in [re.search(kernel + r"<\(?(?:bool\))?(true|false), \(?(?:int\))?(\d+)>", n)] if m]
    rays, settle = tpl("fo_rays_kernel"), tpl("fo_settle_kernel")
    compaction = [("fo_flag_scan_kernel" in n) for n in names if "fo_flag_scan_kernel" in n or "fo_flag_compact_kernel" in n]
    calls = [tuple(int(x) for x in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("call ")]
    want = [F.expected_form(E, O, bool(skip), cells, bool(env)) for E, O, skip, cells in calls]
    print(form, calls, want, rays, compaction)
    assert len(calls) == 10 and len({(nw, sk) for nw, sk, _ in want}) == (2 if env else 4)
    assert {(sk, tl) for _, sk, tl in want} == {(False, False), (False, True), (True, False), (True, True)}
    assert rays == [(sk, nw) for nw, sk, _ in want]
    assert settle == rays
    assert compaction == [tl for _, _, tl in want]
