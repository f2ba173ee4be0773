"""Occlusion memory on a drive through scenario 1: the planning step with the memory off and on.

Per step: HIP-event time of the one-call step (PlanningStep.run, the reference's size: 2 000 candidates x 31 samples, the
default rule families) and of the visibility stage alone (SensorModel.launch) with the memory off and on -- the difference of
the latter is the memory kernel plus its argument call --, the occluded-cell count and the phantom count of both runs.  Prints
one line per step and a JSON summary.  For the memory kernel's own duration run it under
``rocprofv3 --kernel-trace --stats -- python tools/occlusion_memory_bench.py``.

    python tools/occlusion_memory_bench.py [--steps 60] [--v-max 13.9] [--metric euclid|road] [--scene scenario1|city_grid]
        [--vehicles off|lanes] [--quiet]

``--vehicles lanes`` keeps the vehicle layer V next to H (§5.9 "Vehicle layer": one more launch, fo_occlusion_memory_flow_kernel)
and adds the cells of H that V does not hold to every row.
"""
import argparse
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "frenetix-occlusion_amd"))
from frenetix_occlusion import _native as N  # noqa: E402
from frenetix_occlusion import scenario as S  # noqa: E402
from frenetix_occlusion import synthetic as SY  # noqa: E402
from frenetix_occlusion.sensor_model import SensorModel  # noqa: E402
from frenetix_occlusion.spawn_locator import SpawnLocator  # noqa: E402
from frenetix_occlusion.step import PlanningStep  # noqa: E402
from frenetix_occlusion.sweep import MetricSweep  # noqa: E402
from frenetix_occlusion.utils.fo_obstacle import FOObstacles  # noqa: E402

CFG = {"spawn_locator": {"spawn_points_behind_turn": True, "spawn_point_behind_static_obstacle": True,
                         "spawn_point_behind_dynamic_obstacle": True, "max_static_spawn_points": 1,
                         "max_dynamic_spawn_points": 1},
       "agent_manager": {"pedestrian": {"width": 0.5, "length": 0.3, "default_velocity": 1.4},
                         "bicycle": {"width": 0.9, "length": 2.0, "default_velocity": 5.0},
                         "car": {"width": 2.0, "length": 4.8, "default_velocity": 10.0},
                         "truck": {"width": 2.5, "length": 9.0, "default_velocity": 8.0},
                         "prediction": {"variance_factor": 1.05, "size_factor_length_s": 1.2, "size_factor_width_s": 1.3,
                                        "size_factor_length_l": 1.4, "size_factor_width_l": 2.5}},
       "accelerator": {"spawn": {"mode": "rules", "routes": 3, "max_rule_points": 8}}}
DT = 0.1


def stack(sc, path, ego, yaw, v_max, M, T, metric="euclid", vehicles="off"):
    ctx = N.Context(0)
    obs = FOObstacles(sc.obstacles)
    sm = SensorModel(sc.lanelets, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, ctx=ctx, routes=3,
                     intersections=getattr(sc, "intersections", None))
    if v_max is not None:
        sm.enable_occlusion_memory(v_max=v_max, dt=DT, metric=metric, vehicles=vehicles)
    sl = SpawnLocator(None, path, CFG, sm, fo_obstacles=obs, dt=DT, horizon=(T - 1) * DT)
    sw = MetricSweep(SY.VEHICLE_BMW320I, DT, thresholds={"harm": 0.1, "risk": 1}, ctx=ctx)
    traj = SY.make_trajectories(M, T, DT, seed=20240134, ego_pos=ego, ego_yaw=yaw)
    tr = [torch.as_tensor(traj[k]).cuda() for k in ("x", "y", "theta", "v", "a")]
    return SimpleNamespace(obs=obs, sm=sm, sl=sl, ps=PlanningStep(sm, sl, sw, *tr, mode="reduced"))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--v-max", type=float, default=13.9)
    ap.add_argument("--M", type=int, default=2000)
    ap.add_argument("--metric", choices=("euclid", "road"), default="euclid")
    ap.add_argument("--scene", choices=("scenario1", "city_grid"), default="scenario1")
    ap.add_argument("--vehicles", choices=("off", "lanes"), default="off")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    if a.scene == "scenario1":
        sc = S.load_geometry_npz(os.path.join(ROOT, "tests", "golden", "scenario1_geometry.npz"))
    else:
        sc = S.synthetic_urban_grid()
    ego0 = np.asarray(sc.ego_initial, dtype=np.float64)
    yaw, v = float(ego0[2]), float(ego0[3])
    path = ego0[None, :2] + np.linspace(-5.0, 80.0, 171)[:, None] * np.array([[math.cos(yaw), math.sin(yaw)]])
    T = 31
    runs = {"off": stack(sc, path, ego0[:2], yaw, None, a.M, T), "on": stack(sc, path, ego0[:2], yaw, a.v_max, a.M, T, a.metric, a.vehicles)}
    # the visibility stage alone, on sensor models of their own (the memory advances once per step on each)
    vis = {}
    for name, v_max in (("off", None), ("on", a.v_max)):
        vis[name] = SensorModel(None, path, sensor_radius=50.0, sensor_angle=360.0, n_rays=720, routes=3,
                                share_map_with=runs["off"].sm)
        if v_max is not None:
            vis[name].enable_occlusion_memory(v_max=v_max, dt=DT, metric=a.metric, vehicles=a.vehicles)
    rows = []
    for step in range(a.steps):
        ego = ego0[:2] + 0.7634 * step * np.array([math.cos(yaw), math.sin(yaw)])
        row = {"step": step}
        for name, k in runs.items():
            k.obs.update(step)
            k.sm.upload_obstacles(k.obs)
            vis[name].upload_obstacles(k.obs)
            row[f"vis_{name}_ms"] = timed(lambda: vis[name].launch(ego, yaw, timestep=step))
            row[f"step_{name}_ms"] = timed(lambda: k.ps.run(ego, yaw, v, timestep=step))
            h = k.sl.batch.host_head()
            row[f"occ_{name}"] = int(k.sm.n_occluded.item())
            row[f"phantoms_{name}"] = int(h["rule_n"])
        row["reset"] = runs["on"].sm.occlusion_memory_reset_reason
        if a.vehicles != "off":     # (read back after the timed calls)
            row["h_minus_v"] = int((runs["on"].sm.occlusion_memory_hidden != runs["on"].sm.occlusion_memory_hidden_vehicles).sum())
        rows.append(row)
        if not a.quiet:
            print(json.dumps(row))
    warm = rows[3:] if len(rows) > 6 else rows
    med = lambda key: float(np.median([r[key] for r in warm]))
    summary = {"steps": a.steps, "v_max": a.v_max, "M": a.M, "metric": a.metric, "vehicles": a.vehicles, "scene": a.scene, "device": torch.cuda.get_device_name(0)}
    for key in ("vis_off_ms", "vis_on_ms", "step_off_ms", "step_on_ms"):
        summary[key + "_median"] = round(med(key), 4)
    summary["vis_delta_us_median"] = round(1e3 * float(np.median([r["vis_on_ms"] - r["vis_off_ms"] for r in warm])), 2)
    summary["step_delta_us_median"] = round(1e3 * float(np.median([r["step_on_ms"] - r["step_off_ms"] for r in warm])), 2)
    for key in ("occ_off", "occ_on", "phantoms_off", "phantoms_on"):
        summary[key + "_mean"] = round(float(np.mean([r[key] for r in rows])), 2)
    if a.vehicles != "off":
        summary["h_minus_v_mean"] = round(float(np.mean([r["h_minus_v"] for r in rows])), 2)
    summary["resets"] = sum(r["reset"] is not None for r in rows)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
