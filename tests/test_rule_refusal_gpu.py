"""Refused spawn-rule steps (include/fo_hip.h, "A refused rule list"): every table limit of the rule kernels on both sides, a
refused step through every consumer of the sweep, and the selection kernel's visiting order.

A refusal is a defined return value of healthy kernels: a rule that runs out of table space writes -1 into its validity word,
fo_spawn_rules_select_kernel answers with a count of -1 and no list, and from there on the library fails closed -- NaN costs,
safe = 0 -- without any host read.  The scenes (tests/rule_refusal_cases.py) are the known-answer scenes of
tests/test_spawn_rules_gpu.py with one quantity moved onto a limit; where they stand is asserted from the sample-count formula
or from the checker's own counts (oracle/fo_spawn_rules_ref.SpawnRules, which has no table limits), never assumed."""
import copy
import os

import numpy as np
import pytest

import rule_refusal_cases as RC
import test_spawn_rules_gpu as TS

pytestmark = pytest.mark.gpu

METRIC_SETS = [("hr", "ttc", "dce", "cp"), ("dce",), ("ttc",), ("be",)]
THR = {"harm": 0.1, "risk": 1}
REFUSING_CELL = 0.25     # the turn case of test_table_space_of_the_rules_is_enough_or_refused: 1 281 samples over the 40 m window


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch


def _cfg(**spawn_locator):
    cfg = copy.deepcopy(TS.CFG)
    cfg["spawn_locator"].update(spawn_locator)
    return cfg


def _passes(torch, sc, cfg=None, cosy=None):
    """the device's list is the checker's; returns the stage"""
    st = RC.stage(torch, sc, cfg, cosy)
    assert st.raw >= 0
    dev = list(st.pts)
    assert st.sl.last_intention == st.rules.last_intention
    TS._same(dev, st.ref, st.view)
    return st


def _refuses(torch, sc, cfg=None, cosy=None):
    """the raw count is exactly -1 and the list raises when it is read; returns the stage (the checker's list with it)"""
    st = RC.stage(torch, sc, cfg, cosy)
    assert st.raw == -1
    with pytest.raises(RuntimeError, match="table space"):
        list(st.pts)
    return st


def assert_refused(out, M=RC.M):
    """the contract of a sweep over a refused rule list, for every trajectory"""
    from frenetix_occlusion import _native as N
    cost, safe = out.cost.cpu().numpy(), out.safe.cpu().numpy()
    assert cost.shape == (M, N.NC) and safe.shape == (M,)
    assert not safe.any()
    assert np.array_equal(cost[:, N.COST["safe"]], np.zeros(M))
    assert np.array_equal(cost[:, 14:16], np.zeros((M, 2)))                     # FO_C_RES0, FO_C_RES1
    others = [c for c in range(14) if c != N.COST["safe"]]
    assert np.isnan(cost[:, others]).all(), np.argwhere(~np.isnan(cost[:, others]))[:5]


def assert_bit_equal(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# ================================================================================================ (a) each limit on both sides
def test_turn_rule_window_of_1024_and_of_1025_samples(torch_cuda):
    """ns = ceil((total + step / 2) / step), step = cell / 8, over the right turn's 40 m window: the cell size puts the same
    window on 1 024 samples (the list is the checker's) and on 1 025 (count -1; the checker still finds the pedestrian)"""
    total = RC.turn_window_length()
    assert 38.0 < total < 40.5
    fits, over = RC.turn_cell_size(1023.5), RC.turn_cell_size(1024.7)
    assert RC.samples(total, fits) == RC.MAXSAMP == 1024 and RC.samples(total, over) == 1025
    st = _passes(torch_cuda, RC.turn_scene(fits))
    assert len(st.ref) == 1 and st.ref[0].source == "right turn"
    st = _refuses(torch_cuda, RC.turn_scene(over))
    assert len(st.ref) == 1 and st.ref[0].source == "right turn"               # the point the device would have lost


def _wall_facts(st, ob_index=0):
    """what the static rule asks of an obstacle before it measures the cross line, by the checker's own predicates"""
    ob = list(st.obs)[ob_index]
    assert ob.current_visible and ob.obstacle_role == "static"
    assert np.linalg.norm(st.rules.ego_pos - ob.current_pos) <= RC.MAX_DIST_OBST
    ccl = np.array(st.rules.cosy_cl.convert_list_of_points_to_curvilinear_coords(
        [np.array([[x], [y]]) for x, y in ob.current_corner_points], 4))        # (raises when a corner does not project)
    assert ccl.shape == (4, 2)
    ob_s = st.rules.cosy_cl.convert_to_curvilinear_coords(ob.current_pos[0], ob.current_pos[1])[0]
    assert st.ego_cl[0] + 3.0 <= ob_s <= st.ego_cl[0] + st.rules.s_threshold
    return float(ccl[:, 1].max() - ccl[:, 1].min() + 1.6)


def test_static_rule_cross_line_of_1024_and_of_1025_samples(torch_cuda):
    """a static obstacle turned 90 degrees to a straight path (intention 0: the turn rule is off), its length chosen so that
    the cross line -- the d-extent + 1.6 m -- takes 1 024 and 1 025 samples at 0.25 m cells (30.369 m against 30.406 m)"""
    cs = RC.STATIC_CELL
    for ns_plus, want in ((1023.5, 1024), (1024.7, 1025)):
        ob = RC.wall(17.0, RC.total_for(ns_plus, cs))
        sc = RC.static_scene([ob], cs)
        assert RC.samples(RC.cross_line_total(ob, sc.path), cs) == want
        st = _passes(torch_cuda, sc) if want == 1024 else _refuses(torch_cuda, sc)
        assert st.rules.last_intention == "straight ahead"
        assert RC.samples(_wall_facts(st), cs) == want                          # visible, near enough, every corner projects
        assert len(st.ref) == 1 and st.ref[0].source.startswith("behind static obstacle")


def _lanelet_counts(st, ob_index=0):
    """(lanelets under the obstacle's centre, relevant ones among them) as the checker counts them"""
    ob = list(st.obs)[ob_index]
    under = st.rules._lanelets_at(ob.current_pos)
    _, relevant, _ = st.rules._relevant_lanelet_ids()
    return len(under), sum(ll.lanelet_id in relevant for ll in under)


@pytest.mark.parametrize("form", ["runs", "nodes"])
def test_sixteen_and_seventeen_lanelets_under_a_trucks_centre(torch_cuda, monkeypatch, form):
    """the oncoming truck with k copies of the oncoming lanelet under it: sixteen is what the rule holds, seventeen takes the
    re-collection branch (the first sixteen in list order) and refuses the step.  One of them is relevant either way."""
    if form == "nodes":
        monkeypatch.setenv("FO_SCENE_RULE_NODES", "1")
    st = _passes(torch_cuda, RC.truck_scene(16))
    assert _lanelet_counts(st) == (16, 1)
    assert [p.agent_type for p in st.ref] == ["Car", "Bicycle"]
    if form == "runs":
        st = _refuses(torch_cuda, RC.truck_scene(17))
        assert _lanelet_counts(st) == (17, 1)
        assert [p.agent_type for p in st.ref] == ["Car", "Bicycle"]


@pytest.mark.parametrize("form", ["runs", "nodes"])
def test_seven_and_eight_relevant_lanelets_under_a_trucks_centre(torch_cuda, monkeypatch, form):
    """eight lanelets under the truck, seven or all eight of them incomings of the intersection the ego approaches (what makes
    a lanelet relevant with an intersection: fo_spawn_rules_ref.py:397-404)"""
    if form == "nodes":
        monkeypatch.setenv("FO_SCENE_RULE_NODES", "1")
    st = _passes(torch_cuda, RC.truck_scene(8, relevant=7))
    assert _lanelet_counts(st) == (8, 7)
    assert len(st.ref) >= 1
    if form == "runs":
        st = _refuses(torch_cuda, RC.truck_scene(8, relevant=8))
        assert _lanelet_counts(st) == (8, 8)
        assert len(st.ref) >= 1


# ================================================================================================ (c) the selection's visiting order
def test_a_static_obstacle_behind_the_maximum_cannot_refuse_the_step(torch_cuda):
    """max_static = 0: the selection appends the nearest obstacle's pedestrian and breaks at the second.  With the FAR obstacle's
    cross line overflowing the list is the checker's -- before the selection kernel looked only at what it visits, this step was
    refused for an obstacle the reference's list does not depend on.  With the NEAR one overflowing the step is refused."""
    cfg, cs = _cfg(max_static_spawn_points=0), RC.STATIC_CELL
    over = RC.total_for(1024.7, cs)
    st = _passes(torch_cuda, RC.static_scene([RC.parked_car(14.0), RC.wall(24.0, over, oid=78)], cs), cfg)
    assert len(st.ref) == 1 and st.ref[0].source == "behind static obstacle 70"
    assert RC.samples(_wall_facts(st, 1), cs) == 1025                           # the far one is visible and would have been measured
    d = [np.linalg.norm(st.rules.ego_pos - o.current_pos) for o in st.obs]
    assert d[0] < d[1]
    st = _refuses(torch_cuda, RC.static_scene([RC.wall(17.0, over, oid=78), RC.parked_car(27.0)], cs), cfg)
    assert RC.samples(_wall_facts(st, 0), cs) == 1025
    d = [np.linalg.norm(st.rules.ego_pos - o.current_pos) for o in st.obs]
    assert d[0] < d[1] <= RC.MAX_DIST_OBST


def test_a_truck_behind_the_maximum_cannot_refuse_the_step(torch_cuda):
    """the same pair for the dynamic rule, max_dynamic = 0: two oncoming trucks, seventeen lanelets under the far one's centre
    (refused before the selection kernel looked only at what it visits), then under the near one's (refused)"""
    cfg = _cfg(max_dynamic_spawn_points=0)
    trucks = [RC.truck(10.0, 31), RC.truck(28.0, 32)]
    st = _passes(torch_cuda, RC.truck_scene(17, trucks=trucks, x0=22.0, x1=70.0), cfg)
    assert _lanelet_counts(st, 0) == (1, 1) and _lanelet_counts(st, 1) == (17, 1)
    assert all(o.current_visible for o in st.obs)
    assert np.linalg.norm(st.rules.ego_pos - list(st.obs)[1].current_pos) <= RC.MAX_DIST_OBST
    assert len(st.ref) >= 1 and all(p.source.startswith("behind_dynamic") or "dynamic" in p.source for p in st.ref)
    st = _refuses(torch_cuda, RC.truck_scene(17, trucks=trucks, x0=-10.0, x1=19.0), cfg)
    assert _lanelet_counts(st, 0) == (17, 1) and _lanelet_counts(st, 1) == (1, 1)


def test_a_second_cross_line_that_overflows_refuses_the_visited_obstacle(torch_cuda):
    """both cross-line words of a visited static obstacle count.  In the polyline frame the two lines of an obstacle have one
    length; through a caller's frame whose d-lines fan out (RC.FanFrame) the rear line is 1.2 % longer than the front one: a
    wall whose front line fits and whose rear line does not is refused, one a few centimetres shorter gives the checker's list"""
    cs, cosy = RC.STATIC_CELL, RC.FanFrame()
    fit, over = RC.fan_wall_totals(cosy, cs)
    assert fit is not None and over is not None and 0.0 < over - fit < 0.5
    for total, want in ((fit, (True, True)), (over, (True, False))):
        sc = RC.static_scene([RC.wall(17.0, total)], cs)
        st = _passes(torch_cuda, sc, cosy=cosy) if all(want) else _refuses(torch_cuda, sc, cosy=cosy)
        assert st.sl.frame == "caller" and st.sl.frame_fit_m < 1e-9            # the device's table IS the frame
        ob = list(st.obs)[0]
        assert ob.current_visible and np.linalg.norm(st.rules.ego_pos - ob.current_pos) <= RC.MAX_DIST_OBST
        n = [RC.samples(t, cs) for t in RC.frame_cross_lines(cosy, ob.current_corner_points)]
        assert tuple(q <= RC.MAXSAMP for q in n) == want and all(abs(q - RC.MAXSAMP) >= 3 for q in n), n
        assert len(st.ref) == 1 and st.ref[0].source.startswith("behind static obstacle")


# ================================================================================================ (b) a refused step through every consumer
@pytest.fixture(scope="module")
def stacks(torch_cuda):
    """one stack per spawn mode over the refusing scene (built once: the map upload is the expensive part)"""
    made = {}

    def get(spawn_mode):
        if spawn_mode not in made:
            made[spawn_mode] = RC.stack(torch_cuda, RC.turn_scene(REFUSING_CELL), spawn_mode)
        return made[spawn_mode]
    return get


def test_the_refusing_scene_refuses(torch_cuda):
    assert RC.samples(RC.turn_window_length(), REFUSING_CELL) > RC.MAXSAMP
    st = _refuses(torch_cuda, RC.turn_scene(REFUSING_CELL))
    assert len(st.ref) == 1


@pytest.mark.parametrize("metrics", METRIC_SETS, ids=["+".join(m) for m in METRIC_SETS])
@pytest.mark.parametrize("mode", ["reduced", "pair", "full"])
@pytest.mark.parametrize("spawn_mode", ["rules", "both"])
def test_a_refused_step_delivers_no_verdict(torch_cuda, stacks, monkeypatch, spawn_mode, mode, metrics):
    """PlanningStep.run in its fused form and with FO_STEP_STAGES=1: NaN costs, safe = 0, bit-equal to each other, reported by
    fo_sweep_check -- whatever the output mode and the metric mask (masks without CP / HR included: the covariance poison is
    gated on them, this one is not), with and without the cell sampler's agents in the set"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    from frenetix_occlusion.step import PlanningStep
    k = stacks(spawn_mode)
    sc = k.sc
    k.sw.configure(RC.VEH, THR, metrics=metrics)
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode=mode)
    got = []
    for stages in ("0", "1"):
        monkeypatch.setenv("FO_STEP_STAGES", stages)
        out = ps.run(sc.ego, sc.yaw, sc.v)
        torch.cuda.synchronize()
        assert int(k.sl.batch.rule_n.cpu().item()) == -1
        if spawn_mode == "both":
            assert int(k.sl.batch.n.cpu().item()) > 0                           # the cell sampler did add agents
        assert_refused(out)
        got.append((out.cost.clone(), out.safe.clone()))
        with pytest.raises(N.NativeError, match="rule tables"):
            k.ctx.call("fo_sweep_check", N.current_stream(0))
    assert_bit_equal(got[0][0], got[1][0])
    assert torch.equal(got[0][1], got[1][1])
    hb = k.sl.batch.host_body()
    assert (hb["len"] >= 0).all()                                              # no negative length reaches a host view
    with pytest.raises(RuntimeError, match="table space"):
        k.sl.batch.live_agents()


def test_python_stage_path_with_nobody_reading_the_list(torch_cuda):
    """find_spawn_points(lazy=True) -> MetricSweep.set_agents -> run: the first rule slot's length carries the refusal into
    fo_prep_agents_kernel"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sc = RC.turn_scene(REFUSING_CELL)
    k = RC.stack(torch, sc)
    k.sm.launch(sc.ego, sc.yaw)
    pts = k.sl.find_spawn_points(sc.ego, sc.yaw, None, sc.v, lazy=True)
    k.sw.set_agents(*k.sl.batch.sweep_args(), check=False)
    for mode in ("reduced", "pair", "full"):
        out = k.sw.run(*k.tr, mode=mode)
        torch.cuda.synchronize()
        assert_refused(out)
    assert not pts.materialised
    with pytest.raises(N.NativeError, match="rule tables"):
        k.sw.set_agents(*k.sl.batch.sweep_args())                              # (check=True: fo_sweep_check behind the upload)


def test_interface_delivers_what_the_sweep_delivers(torch_cuda, tmp_path):
    """FOInterface.evaluate_scenario + trajectory_safety_assessment_batch(mode='reduced') over the refusing scene: no host read
    of its own, NaN rows and no safe trajectory"""
    import yaml
    from types import SimpleNamespace
    from frenetix_occlusion import interface
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion import synthetic as SY
    sc = RC.turn_scene(REFUSING_CELL)
    with open(os.path.join(os.path.dirname(interface.__file__), "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["accelerator"]["spawn"].update(mode="rules")
    cfg["accelerator"]["cell_size"] = REFUSING_CELL
    cfg["sensor_model"]["sensor_radius"] = 50.0
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    scen = S.Scenario(0.1, sc.lanelets, [], [], np.array([sc.ego[0], sc.ego[1], sc.yaw, sc.v]), "rule refusal")
    veh = SimpleNamespace(length=RC.VEH[0], width=RC.VEH[1], wb_rear_axle=RC.VEH[2], mass=RC.VEH[3], a_max=RC.VEH[4])
    fo = interface.FOInterface(scen, sc.path, veh, 0.1, config_path=str(cfg_path))
    assert fo.sensor_model.cell_size == REFUSING_CELL and fo.spawn_locator.mode == "rules"
    fo.evaluate_scenario({}, sc.ego, sc.yaw, None, sc.v, 0)
    traj = SY.make_trajectories(RC.M, RC.T, 0.1, seed=1, ego_pos=sc.ego, ego_yaw=sc.yaw)
    ba = fo.trajectory_safety_assessment_batch(traj, mode="reduced")
    torch_cuda.cuda.synchronize()
    assert int(fo.spawn_locator.batch.rule_n.cpu().item()) == -1
    assert_refused(ba)
    assert not fo.spawn_points.materialised


def test_sharded_step_carries_the_nan_rows_and_nothing_is_selected(torch_cuda, stacks):
    """PlanningStep(shard=...) at world size 1: cost_all is the refused matrix, select_trajectory raises instead of taking
    index 0 from an argmin over NaN"""
    from types import SimpleNamespace
    from frenetix_occlusion import distributed as D
    from frenetix_occlusion.step import PlanningStep
    k = stacks("rules")
    k.sw.configure(RC.VEH, THR, metrics=METRIC_SETS[0])
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", shard=True)
    out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch_cuda.cuda.synchronize()
    assert out.rows == (0, RC.M) and out.cost_all.shape == (RC.M, 16)
    assert_refused(SimpleNamespace(cost=out.cost_all, safe=out.safe))
    with pytest.raises(RuntimeError, match="no verdict"):
        D.select_trajectory(out.cost_all)


def test_the_next_step_on_the_same_context_is_clean(torch_cuda):
    """the mark carries the generation of its agent set.  One PlanningStep, three steps: the wall of 1 025 samples (refused),
    the wall of 1 024 (its costs hold no NaN and are a fresh context's, bit for bit -- 'never' stays inf), the first again"""
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    from frenetix_occlusion.step import PlanningStep
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    cs = RC.STATIC_CELL
    walls = {w: RC.wall(17.0, RC.total_for(w, cs)) for w in (1023.5, 1024.7)}

    def put(k, ns_plus):
        obs = FOObstacles([walls[ns_plus]])
        obs.update(0)
        k.obs = k.sl.fo_obstacles = obs
        k.sm.upload_obstacles(obs)
    for spawn_mode in ("rules", "both"):
        k = RC.stack(torch, RC.static_scene([walls[1024.7]], cs), spawn_mode)
        sc = k.sc
        ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="pair")
        assert_refused(ps.run(sc.ego, sc.yaw, sc.v))
        put(k, 1023.5)
        out = ps.run(sc.ego, sc.yaw, sc.v)
        torch.cuda.synchronize()
        k.ctx.call("fo_sweep_check", N.current_stream(0))                      # nothing to report
        clean = [t.clone() for t in (out.cost, out.safe, out.pair_f, out.pair_i)]
        assert int(k.sl.batch.rule_n.cpu().item()) == 1
        assert not torch.isnan(clean[0]).any()
        fresh = RC.stack(torch, RC.static_scene([walls[1023.5]], cs), spawn_mode)
        ref = PlanningStep(fresh.sm, fresh.sl, fresh.sw, *fresh.tr, mode="pair").run(sc.ego, sc.yaw, sc.v)
        torch.cuda.synchronize()
        for a, b in zip(clean, (ref.cost, ref.safe, ref.pair_f, ref.pair_i)):
            assert_bit_equal(a, b)
        put(k, 1024.7)
        assert_refused(ps.run(sc.ego, sc.yaw, sc.v))


def test_the_passing_turn_scene_on_a_context_that_refused(torch_cuda):
    """the same pair as in (a) on ONE context: the turn scene at 0.25 m cells (refused), then the scene at the cell size of
    1 024 samples through a new stack on that context -- equal to a fresh context's, bit for bit"""
    torch = torch_cuda
    from frenetix_occlusion.step import PlanningStep
    k = RC.stack(torch, RC.turn_scene(REFUSING_CELL))
    assert_refused(PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced").run(k.sc.ego, k.sc.yaw, k.sc.v))
    sc = RC.turn_scene(RC.turn_cell_size(1023.5))
    outs = []
    for ctx in (k.ctx, None):
        q = RC.stack(torch, sc, ctx=ctx)
        out = PlanningStep(q.sm, q.sl, q.sw, *q.tr, mode="reduced").run(sc.ego, sc.yaw, sc.v)
        torch.cuda.synchronize()
        assert int(q.sl.batch.rule_n.cpu().item()) == 1
        outs.append((out.cost.clone(), out.safe.clone()))
    assert not torch.isnan(outs[0][0]).any()
    assert_bit_equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


# ================================================================================================ no launch was added
# kernels of the child below (set-up + ONE rules step), counted by name, on the parent of the commit that made refused steps
# fail closed (97fa796, "Hidden-traffic brake clearance for mixed road users in one walk")
PARENT_KERNELS = {"fo_erf_table_kernel": 1, "fo_exp_table_kernel": 1, "fo_raster_kernel": 1,                # set-up
                  "fo_rays_kernel": 1, "fo_settle_kernel": 1, "fo_grid_kernel": 1, "fo_flag_compact_kernel": 1,      # scene stage
                  "fo_spawn_rules_kernel": 1, "fo_spawn_rules_select_kernel": 1, "fo_spawn_rule_predict_kernel": 1,  # rule stage
                  "fo_sweep_queue_kernel": 1, "fo_reduce_kernel": 1}                                                 # sweep

_TRACE_CHILD = '''
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import torch
import rule_refusal_cases as RC
from frenetix_occlusion.step import PlanningStep
sc = RC.truck_scene(1)
k = RC.stack(torch, sc)
out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced").run(sc.ego, sc.yaw, sc.v)
torch.cuda.synchronize()
print("rule points", int(k.sl.batch.rule_n.cpu().item()))
print("child ok")
'''


def test_kernel_trace_of_a_rules_step_is_the_parents(torch_cuda, tmp_path):
    """the refusal costs no launch: the library's kernels of one rules step (the oncoming truck, two rule agents) under a kernel
    trace, a fresh child process, counted by name -- the multiset recorded on the parent commit"""
    import collections
    import csv
    import glob
    import re
    import shutil
    import subprocess
    import sys
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        pytest.fail("rocprofv3 is needed for the kernel trace")
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    child = tmp_path / "child_rules_step.py"
    child.write_text(_TRACE_CHILD.format(root=root, pkg=os.path.join(root, "frenetix-occlusion_amd"), tests=tests))
    d = tmp_path / "trace"
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(d), "--", sys.executable, str(child)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout and "rule points 2" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    files = glob.glob(os.path.join(str(d), "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace written"
    names = collections.Counter()
    for f in files:
        with open(f, newline="") as fh:
            for q in csv.DictReader(fh):
                m = re.search(r"\b(fo_[a-z0-9_]+_kernel)\b", q["Kernel_Name"])
                if m:
                    names[m.group(1)] += 1
    print("kernels of one rules step:", dict(sorted(names.items())))
    assert names["fo_spawn_rules_select_kernel"] == 1 and names["fo_spawn_rule_predict_kernel"] == 1 and names["fo_reduce_kernel"] == 1
    assert dict(names) == PARENT_KERNELS
