"""Time the hidden-traffic reach forecast (fo_scene_hidden_reach) with HIP events: the arrival map alone, the
whole call, next to the visibility stage the forecast
follows and the 720-ray first-seen future-visibility call on the same batch.

    python tools/hidden_reach_bench.py [M] [--scene city_grid|scenario1] [--memory] [--calls 25] [--metric euclid|road]
                                       [--flow any|lanes] [--clearance] [--witness] [--brake [A]]
                                       [--brake-classes v1,v2,...] [--brake-users v:metric:flow,...] [--brake-ladder K]
                                       [--brake-ladder-users] [--brake-verdict B] [--brake-ladder-verdict B]
                                       [--brake-impact B] [--brake-harm-ladder B [--harm-limit H]]

``--flow lanes`` (with ``--metric road``): the reach follows the driving direction of the lanes (§5.10 "Lane flow").

``--clearance``: one ``hidden_clearance`` call at ``v_cap = --v-max`` plus ``.reach`` for three speeds (2, 7 m/s and the cap)
against three ``hidden_reach`` calls at those speeds, and the clearance split by stage (key map alone, whole call with and
without heading reuse, the three derivations).

``--witness`` (with ``--metric road``): ``hidden_witness`` -- the forecast plus the route behind every candidate's finding (§5.10
"Witnesses") -- joins the timed loop, next to the forecast alone; also the number of distinct sources and the longest walk.

``--brake [A]``: ``hidden_brake`` -- the forecast plus the brake clearance of every (candidate, brake start) at A m/s^2 (§5.10
"Brake clearance"; default: the vehicle's ``a_max``) -- joins the timed loop; also the manoeuvre poses the kernel scanned (from its
outputs: up to the first hit, one scan for a standing ego), the longest manoeuvre and the candidates by ``commit`` class.

``--brake-classes v1,v2,...``: ``hidden_brake_classes`` for these hidden-user speeds (m/s) at the deceleration of ``--brake`` (§5.10
"Brake clearance by classes") -- one clearance at the fastest speed plus ONE walk that decides every class -- next to one
``hidden_brake`` call per speed in the same process; every class's rows are compared with that call's (exact integers); also the
poses the walk scanned (per manoeuvre the longest of its classes' walks), the poses the per-class walks scan together and the
longest walk.

``--brake-users v:metric:flow,...`` (say ``2:road:any,7:road:lanes,13.9:road:lanes``): ``hidden_brake_users`` for these hidden road
users at the deceleration of ``--brake`` (§5.10 "Brake clearance by road users") -- one clearance per distinct forecast plus ONE walk
-- next to one ``hidden_brake_classes`` call per forecast in the same process, with and without the headings handed over; in every
run every user's rows are compared with its forecast's own call (exact integers); also the poses the one walk scanned and the poses
the per-forecast walks scan.

``--brake-ladder K``: ``hidden_brake_ladder`` at the K decelerations ``linspace(0.5, A, K)`` (A: the deceleration of ``--brake``; K = 23
at the vehicle's ``a_max`` = 11.5 is the interface's default ladder 0.5, 1.0, ...) from every brake start (§5.10 "Brake ladder") --
the forecast plus ONE launch -- next to K ``hidden_brake`` calls in the same process; every level's slice is compared with that
call's (exact integers); also the poses the ladder scanned, the histogram of ``required`` and the non-monotone pairs.

``--brake-ladder-users``: ``hidden_brake_ladder_users`` for the README's road users -- 2.0 road/any, 7.0 road/lanes, 13.9 road/lanes --
at the interface's default ladder 0.5, 1.0, ... 11.5 from every brake start (§5.10 "Brake ladder by road users"): the clearances plus
ONE launch, with the detail and without it, next to one ``hidden_brake_ladder`` call per user in the same process.  In every run both
ties are asserted (exact integers): every level's slice is ``hidden_brake_users`` at that deceleration, every user's rows are
``hidden_brake_ladder`` on that user's forecast.  Also the pairs whose ``required_all`` lies above every user's own ``required``
and how ``blocking`` is spread over the users.

``--brake-verdict B``: ``hidden_brake_verdict`` for the README's road users over the first B brake starts and over all of them (§5.10
"Fail-safe verdict") -- the device pose preparation, the clearances and ONE launch, with and without the poses handed over -- next to
``hidden_brake_users`` on the same device tensors with its host heading pass.  In every run the tie is asserted (exact integers):
``commit`` is ``hidden_brake_users``' where it is below B, ``first`` is its ``first``, ``fail_safe`` and ``user`` are their fold.  Also
the poses the walks scanned.

``--brake-ladder-verdict B``: ``hidden_brake_ladder_verdict`` for the README's road users at the interface's default ladder 0.5, 1.0, ...
11.5 over the first B brake starts (§5.10 "Ladder verdict") -- the whole call, the call with the poses handed over, and the ONE launch
alone (the structure a call left, fold included, handed to the C entry again) -- next to what the launch replaces: ``hidden_brake_ladder_users``
at the same B followed by the torch reduction over b, and ``hidden_brake_verdict`` at the single level ``a_max``.  In every run the tie
is asserted (exact integers, ``decel`` bit for bit): the outputs are that reduction of the ladder-users entry's.  Also the distribution
of ``need``.

``--approach lanes`` (with ``--brake-impact B``): also ``approach="lanes"`` -- its launch next to the head-on launch in the same
process (one profiler trace holds both kernels), and what it does to the grading: the distribution of the obstacle harm against
head-on, the candidates whose user or start changes, the distinct values.  Every ``--brake-impact`` run asserts
``closing <= speed + speed_of`` and ``harm <= head-on harm``.
``--brake-impact B``: ``hidden_brake_impact`` for the README's road users -- a pedestrian, a cyclist and a car of the dimensions the
agent manager gives its phantoms -- over the first B brake starts (§5.10 "Impact verdict"), next to ``hidden_brake_verdict`` at the same
B: the whole call, the call with the poses handed over, and the ONE launch of either alone (the structure a call left handed to the C
entry again).  In every run the tie is asserted: ``commit`` and ``first`` are the verdict's, ``speed`` (bit for bit) and ``at`` are steps
1 - 3 of the definition on ``hidden_brake_users``' ``brake_first`` / ``stop`` / ``first``.  Also the distribution of the obstacle's harm
over the candidates and how many distinct values it takes.

``--brake-harm-ladder B``: ``hidden_brake_harm_ladder`` for the same road users and kinds at the default ladder 0.5, 1.0, ... 11.5 over the
first B brake starts, at ``--harm-limit`` (§5.10 "Harm ladder") -- the whole call, the call with the poses handed over and the ONE launch
alone, next to the launch of ``hidden_brake_ladder_verdict`` in the same process (one profiler trace holds both kernels) and to the 23
``hidden_brake_impact`` calls it replaces.  In every run three consequences of the definition are asserted: at ``harm_limit = 0`` the
shared outputs are the ladder verdict's bit for bit; a level whose ``harm_at`` is within the limit suffices and "no level" means every
level is over it; ``harm_at[:, l]`` is the impact verdict's obstacle harm at ``a_brake = levels[l]`` to 1e-9.  Also the distribution of
``need`` and ``decel`` and where ``harm_at`` rises with harder braking.

``--approach lanes`` (with ``--brake-harm-ladder B``): also ``hidden_brake_harm_ladder_lanes`` at ``--heading-slack`` (§5.10 "Harm ladder
by approach angle") -- its launch next to the head-on launch in the same process, once with the cyclist and the car lane-bound and once
with ``dir_mask = 0`` (the kernel before any further scan), the whole call, and the 23 ``hidden_brake_impact(approach="lanes")`` calls it
replaces.  In every run: with ``dir_mask = 0`` every output is the head-on entry's bit for bit; nothing is above head-on; ``harm_at[:,
l]`` is the impact verdict by approach angle at ``a_brake = levels[l]`` to 1e-9.  Also how many of the head-on stage's "no level"
candidates get a level, the distribution of ``need`` and the ``harm_at`` quantiles against head-on.

Kernel by kernel: run it under ``rocprofv3 --kernel-trace --stats -- python tools/hidden_reach_bench.py ...``."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "frenetix-occlusion_amd")]
from frenetix_occlusion import _native as N  # noqa: E402
from frenetix_occlusion import scenario as SC, synthetic as SY  # noqa: E402
from frenetix_occlusion.hidden_traffic import default_brake_ladder  # noqa: E402
from frenetix_occlusion.sensor_model import SensorModel  # noqa: E402
from frenetix_occlusion.utils.fo_obstacle import FOObstacles  # noqa: E402


def _median_ms(fn, calls):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("M", nargs="?", type=int, default=10000)
    ap.add_argument("--scene", default="city_grid", choices=("city_grid", "scenario1"))
    ap.add_argument("--memory", action="store_true", help="occlusion memory on: the sources are its hidden set")
    ap.add_argument("--steps", type=int, default=5, help="steps of the drive before the timed calls")
    ap.add_argument("--v-max", type=float, default=13.9)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--metric", default="euclid", choices=("euclid", "road"), help="road: the reach follows the road (§5.10)")
    ap.add_argument("--flow", default="any", choices=("any", "lanes"), help="lanes: hidden vehicles follow the lanes (needs --metric road)")
    ap.add_argument("--clearance", action="store_true", help="time hidden_clearance + .reach x 3 against three hidden_reach calls")
    ap.add_argument("--witness", action="store_true", help="time hidden_witness next to hidden_reach (needs --metric road)")
    ap.add_argument("--brake", nargs="?", type=float, const=SY.VEHICLE_BMW320I[4], default=None, metavar="A",
                    help="time hidden_brake at A m/s^2 (default: the vehicle's a_max) next to hidden_reach")
    ap.add_argument("--brake-classes", default=None, metavar="V1,V2,...",
                    help="time hidden_brake_classes for these hidden-user speeds (m/s) next to one hidden_brake call per speed")
    ap.add_argument("--brake-users", default=None, metavar="V:METRIC:FLOW,...",
                    help="time hidden_brake_users for these hidden road users next to one hidden_brake_classes call per forecast")
    ap.add_argument("--brake-ladder", type=int, default=None, metavar="K",
                    help="time hidden_brake_ladder at K decelerations up to the one of --brake next to K hidden_brake calls")
    ap.add_argument("--brake-ladder-users", action="store_true",
                    help="time hidden_brake_ladder_users for the README's three road users next to one hidden_brake_ladder call per user")
    ap.add_argument("--brake-verdict", type=int, default=None, metavar="B",
                    help="time hidden_brake_verdict over the first B brake starts (and over all) next to hidden_brake_users")
    ap.add_argument("--brake-ladder-verdict", type=int, default=None, metavar="B",
                    help="time hidden_brake_ladder_verdict over the first B brake starts next to hidden_brake_ladder_users + its reduction "
                         "and to hidden_brake_verdict at one level")
    ap.add_argument("--brake-impact", type=int, default=None, metavar="B",
                    help="time hidden_brake_impact over the first B brake starts next to hidden_brake_verdict")
    ap.add_argument("--brake-harm-ladder", type=int, default=None, metavar="B",
                    help="time hidden_brake_harm_ladder over the first B brake starts next to hidden_brake_ladder_verdict and to one "
                         "hidden_brake_impact call per level")
    ap.add_argument("--harm-limit", type=float, default=0.1,
                    help="with --brake-harm-ladder: harm_limit (default: metric_thresholds.harm of the reference's example configuration)")
    ap.add_argument("--approach", default="head_on", choices=("head_on", "lanes"),
                    help="with --brake-impact or --brake-harm-ladder: lanes also times the stage by approach angle and records what it does to the grading")
    ap.add_argument("--heading-slack", type=float, default=0.0, help="with --approach lanes: heading_slack in radians")
    a = ap.parse_args()
    if a.flow == "lanes" and a.metric != "road":
        ap.error("--flow lanes needs --metric road")
    if a.witness and a.metric != "road":
        ap.error("--witness needs --metric road")
    if a.scene == "city_grid":
        sc = SC.synthetic_urban_grid()
    else:
        sc = SC.load_geometry_npz(os.path.join(ROOT, "tests", "golden", "scenario1_geometry.npz"))
    ego0 = np.asarray(sc.ego_initial, dtype=np.float64)
    yaw = float(ego0[2])
    sm = SensorModel(sc.lanelets, None, sensor_radius=50.0, sensor_angle=360.0, n_rays=720)
    if a.memory:
        sm.enable_occlusion_memory(v_max=a.v_max, dt=0.1)
    obs = FOObstacles(sc.obstacles)
    for step in range(a.steps):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        obs.update(step)
        sm.calc_visible_and_occluded_area(step, ego, yaw, obs)
    M, T, dev = a.M, 31, sm.device
    traj = SY.make_trajectories(M, T, 0.1, seed=20240134, ego_pos=ego, ego_yaw=yaw)
    tx, ty, tth = (torch.as_tensor(traj[k]).to(dev) for k in ("x", "y", "theta"))
    veh = SY.VEHICLE_BMW320I[:3]
    e = torch.empty((0, T), dtype=torch.float64, device=dev)
    step_no = [a.steps]

    def stage():        # (with the memory on, every stage is a memory step of one timestep)
        sm.launch(ego, yaw, timestep=step_no[0])
        step_no[0] += 1

    res = {"scene": a.scene, "metric": a.metric, "flow": a.flow, "M": M, "T": T, "memory": bool(a.memory), "window": [sm.window.nx, sm.window.ny],
           "build": N.build_id()[:12], "device": torch.cuda.get_device_name(0)}
    res["visibility_stage_ms"] = _median_ms(stage, a.calls)
    out = sm.hidden_reach(tx, ty, tth, vehicle=veh, v_max=a.v_max, dt=0.1, metric=a.metric, flow=a.flow)
    res["halo_cells"] = int(math.isqrt(int(out.r2[-1])))
    res["map_only_ms"] = _median_ms(lambda: sm.hidden_reach(e, e, e, vehicle=veh, v_max=a.v_max, dt=0.1, metric=a.metric, flow=a.flow), a.calls)
    res["call_ms"] = _median_ms(lambda: sm.hidden_reach(tx, ty, tth, vehicle=veh, v_max=a.v_max, dt=0.1, metric=a.metric, flow=a.flow), a.calls)
    res["future_visibility_720_first_seen_ms"] = _median_ms(
        lambda: sm.future_visibility_ex(tx, ty, None, t_stride=5, n_rays=720, first_seen=True), a.calls)
    if a.witness:
        hw = lambda: sm.hidden_witness(tx, ty, tth, vehicle=veh, v_max=a.v_max, dt=0.1, flow=a.flow)
        w = hw()
        res["witness_call_ms"] = _median_ms(hw, a.calls)
        steps, src = w.steps.cpu().numpy(), w.source.cpu().numpy()
        res["path_cap"] = int(w.path_cap)
        res["witnesses"] = int((steps >= 0).sum())
        res["distinct_sources"] = int(len(np.unique(src[steps >= 0], axis=0)))
        res["longest_walk"] = int(steps.max(initial=-1))
        res["walk_steps_total"] = int(steps[steps > 0].sum())
        res["agents_selected"] = len(w.select())
    if a.brake is not None:
        tv = torch.as_tensor(traj["v"]).to(dev)
        hbk = lambda: sm.hidden_brake(tx, ty, tth, tv, vehicle=veh, v_max=a.v_max, dt=0.1, a_brake=a.brake, metric=a.metric, flow=a.flow)
        b_out = hbk()
        res["brake_call_ms"] = _median_ms(hbk, a.calls)
        bf, st, commit = (t.cpu().numpy().astype(np.int64) for t in (b_out.brake_first, b_out.stop, b_out.commit))
        b = np.arange(T)[None, :]
        i0 = np.maximum(st, b + 1)                  # the sample at which the standing pose is first taken
        moving = np.minimum(i0, T) - (b + 1)        # poses before it
        scans = np.where((bf >= 0) & (bf < i0), bf - b, moving + (i0 < T))
        res["a_brake"] = float(a.brake)
        res["manoeuvres"] = int(M * T)
        res["manoeuvre_poses_scanned"] = int(scans.sum())
        res["manoeuvre_poses_defined"] = int(M * T * (T - 1) // 2)
        res["longest_manoeuvre_scanned"] = int(scans.max(initial=0))
        res["commit_classes"] = {"never": int((commit < 0).sum()), "now": int((commit == 0).sum()), "later": int((commit > 0).sum())}
        res["commit_median_of_later"] = float(np.median(commit[commit > 0])) if (commit > 0).any() else None
        res["decided_until_min"] = int(b_out.decided_until().min()) if M else None
    if a.brake_classes:
        cls_speeds = tuple(float(v) for v in a.brake_classes.split(","))
        a_brake = SY.VEHICLE_BMW320I[4] if a.brake is None else a.brake
        tv = torch.as_tensor(traj["v"]).to(dev)
        hbc = lambda **kw: sm.hidden_brake_classes(tx, ty, tth, tv, vehicle=veh, speeds=cls_speeds, dt=0.1, a_brake=a_brake, metric=a.metric,
                                                   flow=a.flow, **kw)
        per_speed = lambda: [sm.hidden_brake(tx, ty, tth, tv, vehicle=veh, v_max=v, dt=0.1, a_brake=a_brake, metric=a.metric, flow=a.flow)
                             for v in cls_speeds]
        c_out, singles = hbc(), per_speed()
        res["brake_class_speeds"] = list(cls_speeds)
        res["brake_classes_call_ms"] = _median_ms(hbc, a.calls)
        res["brake_classes_call_reused_heading_ms"] = _median_ms(lambda: hbc(heading=c_out.clearance.heading), a.calls)
        res["hidden_brake_call_per_speed_ms"] = _median_ms(per_speed, a.calls)
        for c, one in enumerate(singles):           # the tie: every class is that speed's own call, bit for bit
            assert torch.equal(c_out.brake_first[c], one.brake_first) and torch.equal(c_out.commit[c], one.commit), cls_speeds[c]
            assert torch.equal(c_out.first[c], one.reach.first) and torch.equal(c_out.stop, one.stop), cls_speeds[c]
        bf, st = c_out.brake_first.cpu().numpy().astype(np.int64), c_out.stop.cpu().numpy().astype(np.int64)
        b = np.arange(T)[None, :]
        i0 = np.maximum(st, b + 1)                  # the sample at which the standing pose is first taken
        moving = np.minimum(i0, T) - (b + 1)        # poses before it
        per_class = np.where((bf >= 0) & (bf < i0[None]), bf - b[None], (moving + (i0 < T))[None])      # [C, M, T]
        res["class_walk_poses_scanned"] = int(per_class.max(axis=0).sum())
        res["per_class_poses_scanned"] = [int(v) for v in per_class.sum(axis=(1, 2))]
        res["longest_class_walk"] = int(per_class.max(initial=0))
        res["commit_never_per_class"] = [int(v) for v in (c_out.commit < 0).sum(dim=1).cpu()]
        vc = c_out.critical_speed()
        res["candidates_by_critical_speed"] = {str(v): int((vc == v).sum()) for v in sorted(set(cls_speeds))}
    if a.brake_users:
        users = tuple((float(s), m, f) for s, m, f in (u.split(":") for u in a.brake_users.split(",")))
        a_brake = SY.VEHICLE_BMW320I[4] if a.brake is None else a.brake
        tv = torch.as_tensor(traj["v"]).to(dev)
        hbu = lambda **kw: sm.hidden_brake_users(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, a_brake=a_brake, **kw)
        u_out = hbu()
        groups = [[c for c in range(len(users)) if u_out.map_of[c] == k] for k in range(len(u_out.clearances))]

        def per_map(heading=None):      # what the call replaces: one hidden_brake_classes call per forecast, the headings handed over
            outs = []
            for k, members in enumerate(groups):
                _, m, f = users[members[0]]
                outs.append(sm.hidden_brake_classes(tx, ty, tth, tv, vehicle=veh, speeds=tuple(users[c][0] for c in members), dt=0.1,
                                                    a_brake=a_brake, metric=m, flow=f, heading=heading))
                heading = outs[-1].clearance.heading
            return outs

        parts = per_map()
        for members, part in zip(groups, parts):    # the tie, in every run: every user's rows are its forecast's own classes call's
            for n, c in enumerate(members):
                assert torch.equal(u_out.brake_first[c], part.brake_first[n]) and torch.equal(u_out.commit[c], part.commit[n]), users[c]
                assert torch.equal(u_out.first[c], part.first[n]) and torch.equal(u_out.stop, part.stop), users[c]
        res["brake_users"] = [list(u) for u in users]
        res["brake_users_maps"] = [list(m) for m in dict.fromkeys((m, f) for _, m, f in users)]
        res["brake_users_call_ms"] = _median_ms(hbu, a.calls)
        res["brake_users_call_reused_heading_ms"] = _median_ms(lambda: hbu(heading=u_out.clearances[0].heading), a.calls)
        res["brake_classes_call_per_map_ms"] = _median_ms(per_map, a.calls)
        res["brake_classes_call_per_map_reused_heading_ms"] = _median_ms(lambda: per_map(u_out.clearances[0].heading), a.calls)
        bf, st = u_out.brake_first.cpu().numpy().astype(np.int64), u_out.stop.cpu().numpy().astype(np.int64)
        b = np.arange(T)[None, :]
        i0 = np.maximum(st, b + 1)                  # the sample at which the standing pose is first taken
        moving = np.minimum(i0, T) - (b + 1)        # poses before it
        per_user = np.where((bf >= 0) & (bf < i0[None]), bf - b[None], (moving + (i0 < T))[None])        # [C, M, T]
        res["users_walk_poses_scanned"] = int(per_user.max(axis=0).sum())
        res["per_map_walk_poses_scanned"] = [int(per_user[members].max(axis=0).sum()) for members in groups]
        res["longest_users_walk"] = int(per_user.max(initial=0))
        res["commit_never_per_user"] = [int(v) for v in (u_out.commit < 0).sum(dim=1).cpu()]
        cu = u_out.critical_user()
        res["candidates_by_critical_user"] = {str(c): int((cu == c).sum()) for c in range(-1, len(users))}
    if a.brake_verdict:
        users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
        a_brake = SY.VEHICLE_BMW320I[4] if a.brake is None else a.brake
        tv = torch.as_tensor(traj["v"]).to(dev)
        if not 1 <= a.brake_verdict <= T:
            ap.error(f"--brake-verdict B: 1 <= B <= {T}")
        hbv = lambda B, **kw: sm.hidden_brake_verdict(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, a_brake=a_brake, starts=B,
                                                      commit_min=B, **kw)
        # hidden_brake_users on the same tensors, with its host heading pass -- and, for the tie, on the verdict's own headings and on
        # host x, y, whose arc numpy sums as the device does (torch's scan of device tensors may round otherwise)
        hbu = lambda: sm.hidden_brake_users(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, a_brake=a_brake)
        first_out = hbv(a.brake_verdict)
        u_out = sm.hidden_brake_users(traj["x"], traj["y"], None, tv, vehicle=veh, users=users, dt=0.1, a_brake=a_brake,
                                      heading=first_out.poses.heading)
        assert torch.equal(u_out.arc, first_out.poses.arc)
        bf, st = u_out.brake_first.cpu().numpy().astype(np.int64), u_out.stop.cpu().numpy().astype(np.int64)
        b = np.arange(T)[None, :]
        i0 = np.maximum(st, b + 1)
        moving = np.minimum(i0, T) - (b + 1)
        walk = np.where((bf >= 0) & (bf < i0[None]), bf - b[None], (moving + (i0 < T))[None]).max(axis=0)      # [M, T], as --brake-users
        res["brake_verdict_users"] = [list(u) for u in users]
        res["users_walk_poses_scanned"] = int(walk.sum())
        for B in sorted({a.brake_verdict, T}):
            v_out = hbv(B, poses=first_out.poses)
            commit = torch.where((u_out.commit >= 0) & (u_out.commit < B), u_out.commit, -1)          # the tie of step 1, in every run
            assert torch.equal(v_out.commit, commit) and torch.equal(v_out.first, u_out.first), B
            fail_safe = torch.where(commit >= 0, commit, B).amin(dim=0)
            assert torch.equal(v_out.fail_safe, fail_safe.to(torch.int32)), B
            user = torch.where(fail_safe < B, (torch.where(commit >= 0, commit, B) == fail_safe[None]).to(torch.int8).argmax(dim=0), -1)
            assert torch.equal(v_out.user.to(torch.int64), torch.where(v_out.poses.finite != 0, user, -2)), B
            res[f"brake_verdict_call_B{B}_ms"] = _median_ms(lambda: hbv(B), a.calls)
            res[f"brake_verdict_call_B{B}_reused_poses_ms"] = _median_ms(lambda: hbv(B, poses=first_out.poses), a.calls)
            res[f"verdict_walk_poses_scanned_B{B}"] = int(walk[:, :B].sum())
            res[f"candidates_by_fail_safe_B{B}"] = {str(k): int((v_out.fail_safe == k).sum()) for k in range(B + 1)}
            res[f"candidates_by_user_B{B}"] = {str(c): int((v_out.user == c).sum()) for c in range(-2, len(users))}
        res["hidden_poses_call_ms"] = _median_ms(lambda: sm.hidden_poses(tx, ty, tth, tv), a.calls)
        res["brake_users_call_ms"] = _median_ms(hbu, a.calls)
    if a.brake_impact:
        users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
        kinds = (("Pedestrian", 0.3 * 1.2, 0.5 * 1.3), ("Bicycle", 2.0 * 1.4, 0.9 * 2.5), ("Car", 4.8 * 1.2, 2.0 * 1.3))   # length, width x size factors
        a_brake = SY.VEHICLE_BMW320I[4] if a.brake is None else a.brake
        B = a.brake_impact
        if not 1 <= B <= T:
            ap.error(f"--brake-impact B: 1 <= B <= {T}")
        tv = torch.as_tensor(traj["v"]).to(dev)
        hbi = lambda **kw: sm.hidden_brake_impact(tx, ty, tth, tv, vehicle=veh, ego_mass=SY.VEHICLE_BMW320I[3], users=users, kinds=kinds, dt=0.1,
                                                  a_brake=a_brake, starts=B, harm_limit=math.inf, **kw)
        hbv = lambda **kw: sm.hidden_brake_verdict(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, a_brake=a_brake, starts=B, commit_min=B, **kw)
        i_out = hbi()
        v_out = hbv(poses=i_out.poses)
        # the tie, in every run: the verdict entry, and the users entry on the stage's own headings and on host x, y (whose arc numpy sums
        # as the device does), then steps 1 - 3 in numpy float64
        assert torch.equal(i_out.commit, v_out.commit) and torch.equal(i_out.first, v_out.first)
        u_out = sm.hidden_brake_users(traj["x"], traj["y"], None, tv, vehicle=veh, users=users, dt=0.1, a_brake=a_brake, heading=i_out.poses.heading)
        assert torch.equal(u_out.arc, i_out.poses.arc)
        bf, st, fm = (t.cpu().numpy().astype(np.int64) for t in (u_out.brake_first[:, :, :B], u_out.stop[:, :B], u_out.first))
        vh = np.asarray(traj["v"], dtype=np.float64)
        b = np.arange(B)[None, None, :]
        met = (fm[:, :, None] >= 0) & (fm[:, :, None] <= b)
        hit = met | ((bf >= 0) & (bf < st[None]))
        left = vh[None, :, :B] - a_brake * ((bf - b) * 0.1)
        u = np.where(met, np.take_along_axis(vh, np.clip(fm, 0, None).T, axis=1).T[:, :, None], np.where(left > 0.0, left, 0.0))
        u = np.where(hit, u, -np.inf)
        speed, at = u.max(axis=2), u.argmax(axis=2)
        none = ~hit.any(axis=2)
        speed, at = np.where(none, 0.0, speed), np.where(none, -1, at)
        assert np.array_equal(i_out.at.cpu().numpy(), at) and i_out.speed.cpu().numpy().tobytes() == speed.tobytes()
        # the launches alone: a call that folds into a scratch cost / safe pair, then the structure it left handed to the C entry again
        scratch = (torch.zeros((M, N.NC), dtype=torch.float64, device=dev), torch.ones((M,), dtype=torch.uint8, device=dev))
        keep_v = hbv(poses=i_out.poses, cost=scratch[0], safe=scratch[1])
        launch_v = (C.byref(sm._hbv_args), N.current_stream(sm._dev_index))
        res["brake_verdict_launch_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_verdict", *launch_v), a.calls)
        keep_i = hbi(poses=i_out.poses, cost=scratch[0], safe=scratch[1])
        launch_i = (C.byref(sm._hbi_args), N.current_stream(sm._dev_index))
        res["brake_impact_launch_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_impact", *launch_i), a.calls)
        assert torch.equal(keep_i.harm, i_out.harm) and torch.equal(keep_v.fail_safe, v_out.fail_safe)
        assert torch.equal(scratch[0][:, 14].view(torch.int64), i_out.harm[:, 0].contiguous().view(torch.int64))
        res["brake_impact_users"] = [list(u_) for u_ in users]
        res["brake_impact_kinds"] = [list(k) for k in kinds]
        res["brake_impact_B"] = B
        res["brake_impact_call_ms"] = _median_ms(hbi, a.calls)
        res["brake_impact_call_reused_poses_ms"] = _median_ms(lambda: hbi(poses=i_out.poses), a.calls)
        res["brake_verdict_call_ms"] = _median_ms(hbv, a.calls)
        res["brake_verdict_call_reused_poses_ms"] = _median_ms(lambda: hbv(poses=i_out.poses), a.calls)
        harm = i_out.harm[:, 0].cpu().numpy()
        res["obstacle_harm_quantiles"] = {str(q): float(np.quantile(harm, q)) for q in (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)}
        res["obstacle_harm_distinct_values"] = int(len(np.unique(harm)))
        res["obstacle_harm_zero"] = int((harm == 0.0).sum())
        res["candidates_by_impact_user"] = {str(c): int((i_out.user == c).sum()) for c in range(-2, len(users))}
        res["candidates_by_fail_safe"] = {str(k): int((v_out.fail_safe == k).sum()) for k in range(B + 1)}
        # by approach angle: in every run never above head-on, per user and per candidate
        l_out = hbi(poses=i_out.poses, approach="lanes", heading_slack=a.heading_slack)
        w_head = torch.stack([i_out.closing_speed(c) for c in range(len(users))])
        assert bool((l_out.closing <= w_head).all()) and bool((l_out.harm[:, 0] <= i_out.harm[:, 0]).all())
        assert torch.equal(l_out.commit, i_out.commit) and torch.equal(l_out.first, i_out.first)
        assert torch.equal(l_out.closing[0], w_head[0]) and bool((l_out.cosine[0] == 1.0).all())         # the pedestrian is not lane-bound
        if a.approach == "lanes":
            keep_l = hbi(poses=i_out.poses, cost=scratch[0], safe=scratch[1], approach="lanes", heading_slack=a.heading_slack)
            launch_l = (C.byref(sm._hbi_args), N.current_stream(sm._dev_index))
            res["brake_impact_lanes_launch_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_impact_lanes", *launch_l), a.calls)
            unbound = N.HiddenBrakeImpactLanes.from_buffer_copy(sm._hbi_args)        # the same launch with nobody lane-bound: the kernel
            unbound.dir_mask = 0                                                    # before any further scan (the outputs are head-on's)
            launch_u = (C.byref(unbound), N.current_stream(sm._dev_index))
            res["brake_impact_lanes_launch_unbound_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_impact_lanes", *launch_u), a.calls)
            sm.ctx.call("fo_scene_hidden_brake_impact_lanes", *launch_l)
            res["brake_impact_launch_again_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_impact", *launch_i), a.calls)
            assert torch.equal(keep_l.harm, l_out.harm)
            res["brake_impact_lanes_call_reused_poses_ms"] = _median_ms(
                lambda: hbi(poses=i_out.poses, approach="lanes", heading_slack=a.heading_slack), a.calls)
            lharm = l_out.harm[:, 0].cpu().numpy()
            cosn, lat = l_out.cosine.cpu().numpy(), l_out.at.cpu().numpy()
            res["heading_slack"] = a.heading_slack
            res["lanes_obstacle_harm_quantiles"] = {str(q): float(np.quantile(lharm, q)) for q in (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)}
            res["lanes_obstacle_harm_distinct_values"] = int(len(np.unique(lharm)))
            res["lanes_obstacle_harm_ratio_quantiles"] = {str(q): float(np.quantile(lharm[harm > 0] / harm[harm > 0], q))
                                                          for q in (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)} if (harm > 0).any() else {}
            res["lanes_candidates_below_head_on"] = int((lharm < harm).sum())
            res["lanes_candidates_changing_user"] = int((l_out.user != i_out.user).sum())
            res["lanes_candidates_changing_start"] = int((l_out.at != i_out.at).any(dim=0).sum())
            res["lanes_candidates_by_impact_user"] = {str(c): int((l_out.user == c).sum()) for c in range(-2, len(users))}
            res["lanes_hits_below_head_on_by_user"] = [int(((cosn[c] < 1.0) & (lat[c] >= 0)).sum()) for c in range(len(users))]
            res["lanes_hits_by_user"] = [int((lat[c] >= 0).sum()) for c in range(len(users))]
    if a.brake_ladder_verdict:
        users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
        a_max = SY.VEHICLE_BMW320I[4]
        B = a.brake_ladder_verdict
        if not 1 <= B <= T:
            ap.error(f"--brake-ladder-verdict B: 1 <= B <= {T}")
        levels = np.array(default_brake_ladder(a_max, "hidden_brake_ladder_verdict"))
        L = len(levels)
        tv = torch.as_tensor(traj["v"]).to(dev)
        hblv = lambda **kw: sm.hidden_brake_ladder_verdict(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, levels=levels, starts=B,
                                                           a_limit=a_max, **kw)
        hblu = lambda **kw: sm.hidden_brake_ladder_users(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, decelerations=levels, starts=B, **kw)
        hbv = lambda **kw: sm.hidden_brake_verdict(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, a_brake=a_max, starts=B, commit_min=B, **kw)
        levels_inf = torch.as_tensor(np.append(levels, np.inf), device=dev)

        def reduce_over_b(lu, finite=None):         # steps 1 - 6 as torch ops on the ladder-users outputs (no lengths here: ends = B)
            rank = torch.where(lu.required_all >= 0, lu.required_all, L)
            need = rank.amax(dim=1)
            at = (rank == need[:, None]).to(torch.int8).argmax(dim=1)
            blocking = lu.blocking.gather(1, at[:, None])[:, 0]
            low = blocking & -blocking
            user = torch.where(blocking != 0, torch.log2(low.clamp(min=1).to(torch.float64)).to(torch.int64), -1)
            need_of = torch.where(lu.required >= 0, lu.required, L).amax(dim=2)
            if finite is not None:
                bad = finite == 0
                need, at, blocking, user = need.masked_fill(bad, L), at.masked_fill(bad, 0), blocking.masked_fill(bad, 0), user.masked_fill(bad, -2)
            return need, at, blocking, user, levels_inf[need.to(torch.int64)], need_of

        v_out = hblv()
        # the tie, in every run: the ladder-users entry on the verdict's own headings and on host x, y, whose arc numpy sums as the device does
        lu = sm.hidden_brake_ladder_users(traj["x"], traj["y"], None, tv, vehicle=veh, users=users, dt=0.1, decelerations=levels, starts=B,
                                          heading=v_out.poses.heading)
        assert torch.equal(lu.arc, v_out.poses.arc)
        need, at, blocking, user, decel, need_of = reduce_over_b(lu, v_out.poses.finite)
        for name, want in (("need", need), ("at", at), ("blocking", blocking), ("user", user), ("need_of", need_of), ("first", lu.first)):
            assert torch.equal(getattr(v_out, name).to(torch.int64), want.to(torch.int64)), name
        assert torch.equal(v_out.decel.view(torch.int64), decel.view(torch.int64))
        # the launch alone: one more call that folds into a scratch cost / safe pair, then the structure it left handed to the C entry again
        # (its tensors stay referenced by sm and by keep while it is timed); the fold's stores are part of the figure
        scratch = (torch.zeros((M, N.NC), dtype=torch.float64, device=dev), torch.ones((M,), dtype=torch.uint8, device=dev))
        keep = hblv(poses=v_out.poses, cost=scratch[0], safe=scratch[1])
        launch = (C.byref(sm._hblv_args), N.current_stream(sm._dev_index))
        assert torch.equal(scratch[0][:, 14].view(torch.int64), v_out.decel.view(torch.int64)) and int(scratch[1].sum()) == int((v_out.decel <= a_max).sum())
        res["brake_ladder_verdict_users"] = [list(u) for u in users]
        res["brake_ladder_verdict_levels"] = [float(v) for v in levels]
        res["brake_ladder_verdict_B"] = B
        res["brake_ladder_verdict_launch_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_ladder_verdict", *launch), a.calls)
        assert all(torch.equal(getattr(keep, n), getattr(v_out, n)) for n in ("need", "at", "blocking", "user", "decel", "need_of", "first"))
        res["brake_ladder_verdict_call_ms"] = _median_ms(hblv, a.calls)
        res["brake_ladder_verdict_call_reused_poses_ms"] = _median_ms(lambda: hblv(poses=v_out.poses), a.calls)
        res["brake_ladder_users_call_ms"] = _median_ms(hblu, a.calls)
        res["brake_ladder_users_call_plus_reduction_ms"] = _median_ms(lambda: reduce_over_b(hblu()), a.calls)
        res["brake_ladder_users_call_reused_heading_plus_reduction_ms"] = _median_ms(lambda: reduce_over_b(hblu(heading=v_out.poses.heading)), a.calls)
        res["brake_verdict_call_ms"] = _median_ms(hbv, a.calls)
        res["brake_verdict_call_reused_poses_ms"] = _median_ms(lambda: hbv(poses=v_out.poses), a.calls)
        res["candidates_by_need"] = {str(k): int((v_out.need == k).sum()) for k in range(-1, L + 1)}
        res["candidates_by_ladder_user"] = {str(c): int((v_out.user == c).sum()) for c in range(-2, len(users))}
        res["candidates_above_a_limit"] = int((v_out.decel > a_max).sum())
        res["candidates_by_at"] = {str(k): int((v_out.at == k).sum()) for k in range(-1, B)}
    if a.brake_harm_ladder:
        users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
        kinds = (("Pedestrian", 0.3 * 1.2, 0.5 * 1.3), ("Bicycle", 2.0 * 1.4, 0.9 * 2.5), ("Car", 4.8 * 1.2, 2.0 * 1.3))   # length, width x size factors
        a_max, mass = SY.VEHICLE_BMW320I[4], SY.VEHICLE_BMW320I[3]
        B = a.brake_harm_ladder
        if not 1 <= B <= T:
            ap.error(f"--brake-harm-ladder B: 1 <= B <= {T}")
        levels = np.array(default_brake_ladder(a_max, "hidden_brake_harm_ladder"))
        L = len(levels)
        tv = torch.as_tensor(traj["v"]).to(dev)
        hbhl = lambda limit=a.harm_limit, **kw: sm.hidden_brake_harm_ladder(tx, ty, tth, tv, vehicle=veh, ego_mass=mass, users=users, kinds=kinds,
                                                                          dt=0.1, levels=levels, starts=B, harm_limit=limit, a_limit=a_max, **kw)
        hblv = lambda **kw: sm.hidden_brake_ladder_verdict(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, levels=levels, starts=B,
                                                           a_limit=a_max, **kw)
        hbi = lambda a_brake, **kw: sm.hidden_brake_impact(tx, ty, tth, tv, vehicle=veh, ego_mass=mass, users=users, kinds=kinds, dt=0.1,
                                                           a_brake=a_brake, starts=B, harm_limit=math.inf, **kw)
        shared = ("need", "at", "blocking", "user", "decel", "need_of", "first")
        h_out = hbhl()
        poses = h_out.poses
        v_out = hblv(poses=poses)
        # (a), in every run: at harm_limit = 0 every hit counts -- the ladder verdict bit for bit
        zero = hbhl(0.0, poses=poses)
        for name in shared:
            got, want = getattr(zero, name), getattr(v_out, name)
            assert torch.equal(got.view(torch.int64) if got.dtype == torch.float64 else got, want.view(torch.int64) if want.dtype == torch.float64 else want), name
        assert torch.equal(zero.harm_at, h_out.harm_at) and torch.equal(zero.user_at, h_out.user_at)      # the curve does not depend on the limit
        # (c), in every run: a level whose harm is within the limit suffices, and "no level" means every level is over it
        below = h_out.harm_at <= a.harm_limit
        lowest = torch.where(below.any(dim=1), below.to(torch.int8).argmax(dim=1), L)
        asked = h_out.need >= 0
        assert bool((h_out.need[asked] <= lowest[asked]).all()) and bool((h_out.harm_at[h_out.need == L] > a.harm_limit).all())
        assert bool((h_out.need <= v_out.need).all())
        # (e), in every run: level l of the curve is the impact verdict at a_brake = levels[l]
        worst, other_user = 0.0, 0
        for l, level in enumerate(levels):
            i_out = hbi(float(level), poses=poses)
            worst = max(worst, float((h_out.harm_at[:, l] - i_out.harm[:, 0]).abs().max()))
            other_user += int((h_out.user_at[:, l] != i_out.user).sum())
        assert worst <= 1e-9, worst
        res["brake_harm_ladder_worst_difference_to_impact"] = worst
        res["brake_harm_ladder_users_differing_from_impact"] = other_user
        # the launches alone, both in this process so that one profiler trace holds both kernels: a call that folds into a scratch cost /
        # safe pair, then the structure it left handed to the C entry again
        scratch = (torch.zeros((M, N.NC), dtype=torch.float64, device=dev), torch.ones((M,), dtype=torch.uint8, device=dev))
        keep_v = hblv(poses=poses, cost=scratch[0], safe=scratch[1])
        launch_v = (C.byref(sm._hblv_args), N.current_stream(sm._dev_index))
        res["brake_ladder_verdict_launch_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_ladder_verdict", *launch_v), a.calls)
        keep_h = hbhl(poses=poses, cost=scratch[0], safe=scratch[1])
        launch_h = (C.byref(sm._hbhl_args), N.current_stream(sm._dev_index))
        res["brake_harm_ladder_launch_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_harm_ladder", *launch_h), a.calls)
        res["brake_ladder_verdict_launch_again_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_ladder_verdict", *launch_v), a.calls)
        assert torch.equal(keep_h.harm_at, h_out.harm_at) and torch.equal(keep_v.need, v_out.need)
        sm.ctx.call("fo_scene_hidden_brake_harm_ladder", *launch_h)
        torch.cuda.synchronize()
        assert torch.equal(scratch[0][:, 14].view(torch.int64), h_out.decel.view(torch.int64))
        res["brake_harm_ladder_users"] = [list(u) for u in users]
        res["brake_harm_ladder_kinds"] = [list(k) for k in kinds]
        res["brake_harm_ladder_levels"] = [float(v) for v in levels]
        res["brake_harm_ladder_B"] = B
        res["brake_harm_ladder_harm_limit"] = a.harm_limit
        res["brake_harm_ladder_call_ms"] = _median_ms(hbhl, a.calls)
        res["brake_harm_ladder_call_reused_poses_ms"] = _median_ms(lambda: hbhl(poses=poses), a.calls)
        res["brake_ladder_verdict_call_reused_poses_ms"] = _median_ms(lambda: hblv(poses=poses), a.calls)

        def impact_per_level():
            for level in levels:
                hbi(float(level), poses=poses)
        res["brake_impact_calls_per_level_reused_poses_ms"] = _median_ms(impact_per_level, max(a.calls // 5, 3))
        decel = h_out.decel.cpu().numpy()
        res["decel_distinct_values"] = int(len(np.unique(decel)))
        res["candidates_by_need"] = {str(k): int((h_out.need == k).sum()) for k in range(-1, L + 1)}
        res["candidates_no_level"] = int((h_out.need == L).sum())
        res["candidates_by_need_ladder_verdict"] = {str(k): int((v_out.need == k).sum()) for k in range(-1, L + 1)}
        res["candidates_by_harm_ladder_user"] = {str(c): int((h_out.user == c).sum()) for c in range(-2, len(users))}
        mono = h_out.monotone()
        res["candidates_not_monotone"] = int((~mono).sum())
        rises = (h_out.harm_at[:, 1:] > h_out.harm_at[:, :-1]).sum(dim=0).cpu().numpy()
        res["candidates_rising_into_level"] = {str(l + 1): int(n) for l, n in enumerate(rises) if n}
        ha = h_out.harm_at.cpu().numpy()
        res["harm_at_quantiles_by_level"] = {str(l): [float(np.quantile(ha[:, l], q)) for q in (0.0, 0.5, 1.0)] for l in (0, L // 2, L - 1)}
        if a.approach == "lanes":
            # by approach angle (§5.10 "Harm ladder by approach angle"): the cyclist and the car are lane-bound
            hbll = lambda limit=a.harm_limit, **kw: sm.hidden_brake_harm_ladder_lanes(
                tx, ty, tth, tv, vehicle=veh, ego_mass=mass, users=users, kinds=kinds, dt=0.1, levels=levels, starts=B, harm_limit=limit,
                a_limit=a_max, heading_slack=a.heading_slack, **kw)
            every = shared + ("harm_at", "user_at")
            bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
            l_out = hbll(poses=poses)
            # (b), in every run: never above head-on
            assert bool((l_out.harm_at <= h_out.harm_at).all()) and bool((l_out.need <= h_out.need).all()) and bool((l_out.decel <= h_out.decel).all())
            assert bool((l_out.need_of <= h_out.need_of).all()) and torch.equal(l_out.first, h_out.first)
            # (c), in every run: level l of the curve is the impact verdict by approach angle at a_brake = levels[l]
            worst, other_user = 0.0, 0
            for l, level in enumerate(levels):
                i_out = hbi(float(level), poses=poses, approach="lanes", heading_slack=a.heading_slack)
                worst = max(worst, float((l_out.harm_at[:, l] - i_out.harm[:, 0]).abs().max()))
                other_user += int((l_out.user_at[:, l] != i_out.user).sum())
            assert worst <= 1e-9, worst
            res["brake_harm_ladder_lanes_worst_difference_to_impact_lanes"] = worst
            res["brake_harm_ladder_lanes_users_differing_from_impact_lanes"] = other_user
            # the launches alone, next to the head-on launch in this process: with the users' mask, and -- the same structure with
            # dir_mask = 0, the kernel before any further scan -- (a), in every run: every output is the head-on entry's bit for bit
            keep_l = hbll(poses=poses, cost=scratch[0], safe=scratch[1])
            args_l = sm._hbhl_args
            launch_l = (C.byref(args_l), N.current_stream(sm._dev_index))
            mask = int(args_l.dir_mask)
            assert mask == 0b110 or a.heading_slack >= 7.0 * math.pi / 8.0
            res["brake_harm_ladder_lanes_launch_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_harm_ladder_lanes", *launch_l), a.calls)
            res["brake_harm_ladder_launch_again_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_harm_ladder", *launch_h), a.calls)
            args_l.dir_mask = 0
            res["brake_harm_ladder_lanes_launch_dir_mask_0_ms"] = _median_ms(lambda: sm.ctx.call("fo_scene_hidden_brake_harm_ladder_lanes", *launch_l), a.calls)
            torch.cuda.synchronize()
            for name in every:
                assert torch.equal(bits(getattr(keep_l, name)), bits(getattr(h_out, name))), name
            args_l.dir_mask = mask
            sm.ctx.call("fo_scene_hidden_brake_harm_ladder_lanes", *launch_l)
            torch.cuda.synchronize()
            for name in every:
                assert torch.equal(bits(getattr(keep_l, name)), bits(getattr(l_out, name))), name
            # (for whoever reads a kernel trace of this run: in launch order the new kernel's dispatches [first, last) are those with dir_mask = 0)
            res["brake_harm_ladder_lanes_dispatches_with_dir_mask_0"] = [2 + (a.calls + 1), 2 + 2 * (a.calls + 1)]
            res["heading_slack"] = a.heading_slack
            res["brake_harm_ladder_lanes_call_ms"] = _median_ms(hbll, a.calls)
            res["brake_harm_ladder_lanes_call_reused_poses_ms"] = _median_ms(lambda: hbll(poses=poses), a.calls)

            def impact_lanes_per_level():
                for level in levels:
                    hbi(float(level), poses=poses, approach="lanes", heading_slack=a.heading_slack)
            res["brake_impact_lanes_calls_per_level_reused_poses_ms"] = _median_ms(impact_lanes_per_level, max(a.calls // 5, 3))
            # the grading against head-on
            none_head = h_out.need == L
            res["lanes_candidates_by_need"] = {str(k): int((l_out.need == k).sum()) for k in range(-1, L + 1)}
            res["lanes_candidates_no_level"] = int((l_out.need == L).sum())
            res["lanes_candidates_no_level_head_on_that_get_a_level"] = int((none_head & (l_out.need < L)).sum())
            res["lanes_candidates_with_lower_need"] = int((l_out.need < h_out.need).sum())
            res["lanes_candidates_by_harm_ladder_user"] = {str(c): int((l_out.user == c).sum()) for c in range(-2, len(users))}
            res["lanes_candidates_not_monotone"] = int((~l_out.monotone()).sum())
            la = l_out.harm_at.cpu().numpy()
            res["lanes_harm_at_quantiles_by_level"] = {str(l): [float(np.quantile(la[:, l], q)) for q in (0.0, 0.5, 1.0)] for l in (0, L // 2, L - 1)}
            hit = ha > 0
            res["lanes_harm_at_ratio_quantiles"] = ({str(q): float(np.quantile(la[hit] / ha[hit], q)) for q in (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)}
                                                    if hit.any() else {})
            res["lanes_pairs_below_head_on"] = int((la < ha).sum())
    if a.brake_ladder:
        a_top = SY.VEHICLE_BMW320I[4] if a.brake is None else a.brake
        levels = np.linspace(0.5, a_top, a.brake_ladder) if a.brake_ladder > 1 else np.array([a_top])
        tv = torch.as_tensor(traj["v"]).to(dev)
        hbl = lambda: sm.hidden_brake_ladder(tx, ty, tth, tv, vehicle=veh, v_max=a.v_max, dt=0.1, decelerations=levels, metric=a.metric,
                                             flow=a.flow)
        per_level = lambda: [sm.hidden_brake(tx, ty, tth, tv, vehicle=veh, v_max=a.v_max, dt=0.1, a_brake=float(lv), metric=a.metric, flow=a.flow)
                             for lv in levels]
        l_out, singles = hbl(), per_level()
        for k, one in enumerate(singles):           # the tie: every level is that deceleration's own call, bit for bit
            bf_k, st_k, cm_k = l_out.level(k)
            assert torch.equal(bf_k, one.brake_first) and torch.equal(st_k, one.stop) and torch.equal(cm_k, one.commit), float(levels[k])
        res["brake_ladder_levels"] = [float(lv) for lv in levels]
        res["brake_ladder_call_ms"] = _median_ms(hbl, a.calls)
        res["hidden_brake_call_per_level_ms"] = _median_ms(per_level, a.calls)
        bf, st = (t.cpu().numpy().astype(np.int64) for t in (l_out.brake_first, l_out.stop))      # [M, B, K]
        b = np.arange(T)[None, :, None]
        i0 = np.maximum(st, b + 1)                  # the sample at which the standing pose is first taken
        moving = np.minimum(i0, T) - (b + 1)        # poses before it
        scans = np.where((bf >= 0) & (bf < i0), bf - b, moving + (i0 < T))
        req, lu = (t.cpu().numpy().astype(np.int64) for t in (l_out.required, l_out.last_unclear))
        res["ladder_manoeuvres"] = int(M * T * len(levels))
        res["ladder_poses_scanned"] = int(scans.sum())
        res["ladder_poses_scanned_per_level"] = [int(v) for v in scans.sum(axis=(0, 1))]
        res["longest_ladder_manoeuvre_scanned"] = int(scans.max(initial=0))
        res["required_histogram"] = {str(k): int((req == k).sum()) for k in range(-1, len(levels))}
        fm = l_out.reach.first.cpu().numpy().astype(np.int64)[:, None]
        blocked = (fm >= 0) & (fm <= np.arange(T)[None, :])       # the candidate itself is in reached road: no level can be clear
        res["pairs_blocked_by_first"] = int(blocked.sum())
        res["pairs_without_a_clear_level_unblocked"] = int(((req < 0) & ~blocked).sum())
        res["non_monotone_pairs"] = int((~l_out.monotone()).sum())
        res["non_monotone_required_below_last_unclear"] = int(((req >= 0) & (req < lu)).sum())
    if a.brake_ladder_users:
        users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
        levels = np.array([0.5 * (k + 1) for k in range(23)])          # FOInterface's default ladder at a_max = 11.5
        tv = torch.as_tensor(traj["v"]).to(dev)
        hblu = lambda **kw: sm.hidden_brake_ladder_users(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, decelerations=levels, **kw)
        per_user = lambda: [sm.hidden_brake_ladder(tx, ty, tth, tv, vehicle=veh, v_max=s, dt=0.1, decelerations=levels, metric=m, flow=f)
                            for s, m, f in users]
        d_out, s_out, ladders = hblu(detail=True), hblu(), per_user()
        for k in ("required", "last_unclear", "commit", "first", "required_all", "last_unclear_all", "blocking"):
            assert torch.equal(getattr(d_out, k), getattr(s_out, k)), k         # the detail changes nothing else
        for n, lv in enumerate(levels):             # the tie by levels: every slice is hidden_brake_users at that deceleration
            one = sm.hidden_brake_users(tx, ty, tth, tv, vehicle=veh, users=users, dt=0.1, a_brake=float(lv), heading=d_out.clearances[0].heading)
            bf_n, st_n, cm_n = d_out.level(n)
            assert torch.equal(bf_n, one.brake_first) and torch.equal(st_n, one.stop) and torch.equal(cm_n, one.commit), float(lv)
            assert torch.equal(d_out.first, one.first), float(lv)
        for c, one in enumerate(ladders):           # the tie by users: every row is hidden_brake_ladder on that user's forecast
            assert torch.equal(d_out.required[c], one.required) and torch.equal(d_out.last_unclear[c], one.last_unclear), users[c]
            assert torch.equal(d_out.commit[c], one.commit) and torch.equal(d_out.brake_first[c], one.brake_first), users[c]
            assert torch.equal(d_out.stop, one.stop) and torch.equal(d_out.first[c], one.reach.first), users[c]
        res["brake_ladder_users"] = [list(u) for u in users]
        res["brake_ladder_users_levels"] = [float(lv) for lv in levels]
        res["brake_ladder_users_call_ms"] = _median_ms(hblu, a.calls)
        res["brake_ladder_users_call_detail_ms"] = _median_ms(lambda: hblu(detail=True), a.calls)
        res["brake_ladder_users_call_reused_heading_ms"] = _median_ms(lambda: hblu(heading=d_out.clearances[0].heading), a.calls)
        res["hidden_brake_ladder_call_per_user_ms"] = _median_ms(per_user, a.calls)
        req, ra, blocking = (t.cpu().numpy().astype(np.int64) for t in (s_out.required, s_out.required_all, s_out.blocking))
        own = np.where(req < 0, len(levels), req)
        above = (req >= 0).all(axis=0) & (np.where(ra < 0, len(levels), ra) > own.max(axis=0))
        res["pairs"] = int(M * T)
        res["pairs_required_all_above_every_user"] = int(above.sum())
        res["pairs_required_all_above_the_users_maximum"] = int((np.where(ra < 0, len(levels), ra) > own.max(axis=0)).sum())
        res["required_all_histogram"] = {str(k): int((ra == k).sum()) for k in range(-1, len(levels))}
        res["non_monotone_pairs_all_users"] = int((~s_out.monotone()).sum())
        res["non_monotone_pairs_per_user"] = [int((~s_out.monotone(c)).sum()) for c in range(len(users))]
        res["pairs_blocked_by_user"] = [int((blocking >> c & 1).sum()) for c in range(len(users))]
        res["pairs_by_blocking_mask"] = {format(k, "03b"): int((blocking == k).sum()) for k in range(1 << len(users))}
    if a.clearance:
        speeds = (2.0, 7.0, a.v_max)
        hc = lambda **kw: sm.hidden_clearance(tx, ty, tth, vehicle=veh, v_cap=a.v_max, dt=0.1, metric=a.metric, flow=a.flow, **kw)
        got = hc()

        def three_reach_calls():
            for v in speeds:
                sm.hidden_reach(tx, ty, tth, vehicle=veh, v_max=v, dt=0.1, metric=a.metric, flow=a.flow)

        def derive(c=got):
            for v in speeds:
                c.reach(v)

        res["speeds"] = list(speeds)
        res["three_hidden_reach_calls_ms"] = _median_ms(three_reach_calls, a.calls)
        res["clearance_plus_three_reach_ms"] = _median_ms(lambda: derive(hc()), a.calls)
        res["clearance_reused_heading_plus_three_reach_ms"] = _median_ms(lambda: derive(hc(heading=got.heading)), a.calls)
        res["clearance_call_ms"] = _median_ms(hc, a.calls)
        res["clearance_call_reused_heading_ms"] = _median_ms(lambda: hc(heading=got.heading), a.calls)
        res["clearance_map_only_ms"] = _median_ms(
            lambda: sm.hidden_clearance(e, e, e, vehicle=veh, v_cap=a.v_max, dt=0.1, metric=a.metric, flow=a.flow), a.calls)
        res["three_reach_derivations_ms"] = _median_ms(derive, a.calls)
        res["critical_speed_ms"] = _median_ms(got.critical_speed, a.calls)
        # the two ways agree (exact integers), and what the critical speed says of the batch
        for v in speeds:
            r = sm.hidden_reach(tx, ty, tth, vehicle=veh, v_max=v, dt=0.1, metric=a.metric, flow=a.flow)
            hit, f, sl = got.reach(v)
            assert torch.equal(hit, r.cells > 0) and torch.equal(f, r.first) and torch.equal(sl, r.slack), v
        vc = got.critical_speed()
        fin = vc[torch.isfinite(vc)]
        res["trajectories_with_finite_critical_speed"] = int(fin.numel())
        res["critical_speed_quartiles"] = [float(torch.quantile(fin, q)) for q in (0.25, 0.5, 0.75)] if fin.numel() else None
    torch.cuda.synchronize()
    first = out.first.cpu().numpy()
    res["trajectories_meeting_hidden_traffic"] = int((first >= 0).sum())
    res["arrival_cells_reached"] = int((out.arrival.cpu().numpy() != 255).sum())
    if a.metric == "road":
        res["road_reach_units"] = int(out.reach[-1])
        res["road_cells_within_reach"] = int((out.road_dist.cpu().numpy() != 65535).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
