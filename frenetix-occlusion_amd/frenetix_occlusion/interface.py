"""``FOInterface`` -- the plugin surface the Frenetix-Motion-Planner loop talks to (ref: interface.py:18-238).

Same constructor, same ``evaluate_scenario`` / ``trajectory_safety_assessment`` / ``set_coordinate_system``
signatures and the same instance attributes as the reference, so the planner sees a drop-in; behind it every
per-step stage runs in libfo_hip.so on one MI355X:

    evaluate_scenario           obstacle poses -> ray fan + cell classes (fo_scene_visibility) -> phantom sampling and
                                predictions in the occluded cells (fo_scene_spawn) -> agent table (fo_sweep_set_agents)
    trajectory_safety_assessment_batch   all candidate trajectories x all phantom predictions in one launch
    trajectory_safety_assessment         the reference's per-trajectory call, served from the cached batch

Deviations from the reference (documented in DESIGN.md): ``visible_area`` is a ring polygon + cell mask
(:class:`~frenetix_occlusion.sensor_model.VisibleArea`) instead of a shapely geometry; spawn points come from the
reference's three rule families evaluated on the cell classes (``accelerator.spawn.mode: rules``, the default:
fo_scene_spawn_rules -> fo_scene_spawn_rule_agents, device resident -- the spawn points never leave HBM on their way into
the sweep, ``spawn_points`` is a list that reads them back when first looked at) and / or from the occluded-cell frontier
(``cells`` / ``both``: the sampler of the BASELINE configurations, not what the reference spawns); no matplotlib
(``plot`` is accepted and ignored); metric ``'be'`` implies ``'ttc'`` (the reference raises KeyError when ``'be'`` is
activated without it).
"""
import os
import time

import numpy as np
import torch
import yaml

from . import _native as N
from .agent import FOAgentManager
from .metrics.metric import Metric
from .hidden_traffic import default_brake_ladder as _default_brake_ladder
from .sensor_model import SensorModel
from .spawn_locator import SpawnLocator
from .utils.fo_obstacle import FOObstacles


def occlusion_memory_config(acc):
    """``accelerator.occlusion_memory`` of a loaded configuration with its defaults: ``enabled`` False, ``v_max`` 13.9 m/s,
    ``margin`` None (= sqrt(2) cell sizes)"""
    om = (acc or {}).get("occlusion_memory") or {}
    margin = om.get("margin")
    out = {"enabled": bool(om.get("enabled", False)), "v_max": float(om.get("v_max", 13.9)),
           "margin": None if margin is None else float(margin)}
    if not out["v_max"] >= 0.0 or (out["margin"] is not None and not out["margin"] >= 0.0):
        raise ValueError("accelerator.occlusion_memory: v_max and margin must be >= 0")
    return out


def occlusion_memory_metric(acc):
    """``accelerator.occlusion_memory_metric`` of a loaded configuration: ``"euclid"`` (the default) or ``"road"``"""
    metric = (acc or {}).get("occlusion_memory_metric", "euclid")
    if metric is None:
        metric = "euclid"
    if metric not in ("euclid", "road"):
        raise ValueError(f"accelerator.occlusion_memory_metric: 'euclid' or 'road', not {metric!r}")
    return metric


def occlusion_memory_vehicles(acc):
    """``accelerator.occlusion_memory_vehicles`` of a loaded configuration: ``"off"`` (the default) or ``"lanes"``; YAML reads a
    bare ``off`` as False, which counts as ``"off"``"""
    vehicles = (acc or {}).get("occlusion_memory_vehicles", "off")
    if vehicles is None or vehicles is False:
        vehicles = "off"
    if vehicles not in ("off", "lanes"):
        raise ValueError(f"accelerator.occlusion_memory_vehicles: 'off' or 'lanes', not {vehicles!r}")
    return vehicles


class FOInterface:
    def __init__(self, scenario, reference_path, vehicle_params, dt, config_path=None, cosy_cl=None, share_map_with=None):
        """Signature of the reference (interface.py:69) plus ``share_map_with``: another FOInterface of the same scenario
        on the same GPU (the planner of another ego) whose static map this one reads instead of building and uploading
        its own (BASELINE configs[4])."""
        self.config = self._load_config(config_path)
        acc = self.config.get("accelerator") or {}
        if not torch.cuda.is_available():
            raise RuntimeError("FOInterface needs a ROCm GPU: this build has no CPU path")
        self.device = torch.device("cuda", int(acc.get("device", 0)))

        # things that never change (interface.py:74-82)
        self.cr_scenario = scenario
        self.lanelet_network = scenario.lanelet_network
        self.ego_reference_path = np.asarray(reference_path, dtype=np.float64)
        self.cosy_cl = cosy_cl
        self.vehicle_params = vehicle_params
        self.dt = dt
        self.plot = self.config.get("plot", False)
        self.debug = self.config.get("debug", False)

        # per-step state (interface.py:85-90)
        self.predictions = None
        self.ego_pos = None
        self.ego_orientation = None
        self.ego_pos_cl = None
        self.timestep = None
        self.spawn_points = []

        self.sensor_radius = self.config["sensor_model"]["sensor_radius"]
        self.sensor_angle = self.config["sensor_model"]["sensor_angle"]
        self.visualization = None   # debug drawing is out of scope (forces TkAgg upstream)
        self.include_real_agents = bool(acc.get("include_real_agents", False))
        self._timing_sync = str(acc.get("timing", "issue")) == "device"
        self.step_timing = {}
        self._one_call = bool(acc.get("one_call", True))
        self._scene_step = None

        self.ctx = N.Context(self.device.index)
        self.fo_obstacles = FOObstacles(self.cr_scenario.obstacles)
        spawn_acc = acc.get("spawn") or {}
        routes = int(spawn_acc.get("routes", 0))
        if routes == 0 and str(spawn_acc.get("mode", "rules")) != "cells":
            routes = 3     # the rule families' vehicles follow the routes of their lanelet (agent.py:283-312)
        self.sensor_model = SensorModel(lanelet_network=self.lanelet_network, ref_path=self.ego_reference_path,
                                        sensor_radius=self.sensor_radius, sensor_angle=self.sensor_angle,
                                        visualization=None, debug=self.debug, ctx=self.ctx,
                                        n_rays=int(acc.get("rays", 720)), cell_size=float(acc.get("cell_size", 0.5)),
                                        device=self.device.index, routes=routes,
                                        footprint=str(acc.get("footprint", "polygon")),
                                        enclosed_holes=str(acc.get("enclosed_holes", "transparent")),
                                        cell_visibility=str(acc.get("cell_visibility", "exact")),
                                        shadow_length=float(acc.get("shadow_length", 100.0)),
                                        share_map_with=share_map_with.sensor_model if share_map_with is not None else None,
                                        intersections=getattr(self.cr_scenario, "intersections", None) or
                                        getattr(self.lanelet_network, "intersections", None))
        self.agent_manager = FOAgentManager(scenario=self.cr_scenario, reference_path=self.ego_reference_path,
                                            config=self.config["agent_manager"], visualization=None,
                                            timestep=self.timestep, dt=self.dt, debug=self.debug,
                                            fo_obstacles=self.fo_obstacles, device=self.device)
        self.spawn_locator = SpawnLocator(agent_manager=self.agent_manager, ref_path=self.ego_reference_path,
                                          config=self.config, cosy_cl=self.cosy_cl, sensor_model=self.sensor_model,
                                          fo_obstacles=self.fo_obstacles, visualization=None, debug=self.debug,
                                          dt=self.dt)
        self.metrics = Metric(self.config["metrics"], self.vehicle_params, self.agent_manager, dt=self.dt,
                              device=self.device.index, ctx=self.ctx, list_storage=str(acc.get("list_storage", "f64")))
        # EXTENSION (accelerator.occlusion_memory, off by default): occluded cells seen empty since a hidden road user
        # could have got there are no longer occluded (SensorModel.enable_occlusion_memory)
        self.occlusion_memory = occlusion_memory_config(acc)
        self.occlusion_memory_metric = occlusion_memory_metric(acc)
        self.occlusion_memory_vehicles = occlusion_memory_vehicles(acc)
        if self.occlusion_memory["enabled"]:
            self.sensor_model.enable_occlusion_memory(v_max=self.occlusion_memory["v_max"],
                                                      margin=self.occlusion_memory["margin"], dt=self.dt,
                                                      metric=self.occlusion_memory_metric,
                                                      vehicles=self.occlusion_memory_vehicles)

    # ---------------------------------------------------------------------------------------- reference API
    def reset_occlusion_memory(self):
        """EXTENSION: the next evaluate_scenario forgets what was seen before (its occluded area is that of a step without
        occlusion memory); a no-op while ``accelerator.occlusion_memory.enabled`` is False"""
        self.sensor_model.reset_occlusion_memory()

    def set_coordinate_system(self, cosy_cl):
        self.cosy_cl = cosy_cl
        self.spawn_locator.cosy_cl = cosy_cl

    def _add_real_agents(self):
        if self.config.get("agents") is None:
            return
        for agent in self.config["agents"]:
            self.agent_manager.add_agent(pos=agent["position"], velocity=agent["velocity"],
                                         agent_type=agent["agent_type"], add_to_scenario=True,
                                         timestep=agent["timestep"], horizon=agent["horizon"])

    def _tick(self, name, t0):
        """stage timer of ``step_timing``: host wall time since t0; with ``accelerator.timing: device`` the stream is
        drained first, so the figure is the stage's own GPU + host time instead of the time to issue it"""
        if self._timing_sync:
            torch.cuda.current_stream(self.device).synchronize()
        t1 = time.perf_counter()
        self.step_timing[name] = (t1 - t0) * 1e3
        return t1

    def evaluate_scenario(self, predictions, ego_pos, ego_orientation, ego_pos_cl, ego_v, timestep, cosy_cl=None):
        """ref: interface.py:148-214.  Besides the visible area (the return value) the call leaves
        ``self.step_timing``: milliseconds per stage of this planning step -- ``obstacles_ms`` (state cache),
        ``visibility_ms`` (ray fan, cell classes), ``spawn_ms`` (phantom sampling / rule families + predictions),
        ``agents_ms`` (registry), ``evaluate_scenario_ms`` (all of it), later ``assessment_batch_ms`` /
        ``assessment_single_ms`` (metric sweep calls; the latter accumulates over the per-trajectory calls of the step
        and counts them in ``assessment_single_calls``).  Host wall times of asynchronous work = the time to ISSUE it,
        unless ``accelerator.timing: device`` (see :meth:`_tick`)."""
        t_all = t0 = time.perf_counter()
        self.step_timing = {"timestep": int(timestep), "mode": "device" if self._timing_sync else "issue"}
        self.set_coordinate_system(cosy_cl)
        self._update_time_step(timestep)
        self._add_real_agents()
        self.predictions = predictions
        self.ego_pos = np.asarray(ego_pos, dtype=np.float64)
        self.ego_orientation = float(ego_orientation)
        self.ego_pos_cl = ego_pos_cl
        self.agent_manager.reset()
        self.metrics.invalidate()
        self.spawn_points = []

        self.fo_obstacles.update(self.timestep)
        t0 = self._tick("obstacles_ms", t0)
        # The GPU side of the step -- ray fan, cell classes, visible objects, phantom sampling and / or the reference's rule
        # families, their agents and predictions, the sweep's agent table -- is ONE native call (fo_step_run through a
        # PlanningStep without candidate trajectories; ``accelerator.one_call: False`` queues the stage calls instead).
        # Nothing of interface.py:186-198's find_spawn_points -> add_agent loop runs on the host; the spawn-point list is the
        # reference's host view, read back when somebody looks at it.
        sm, sl = self.sensor_model, self.spawn_locator
        if self._one_call:
            if self._scene_step is None:
                from .step import PlanningStep
                empty = torch.empty((0, sl.T), dtype=torch.float64, device=self.device)
                self._scene_step = PlanningStep(sm, sl, self.metrics.sweep, empty, empty, empty, empty, empty, mode="reduced",
                                                mirror=True)
            sm.timestep = self.timestep
            sl.spawn_points, sl._rule_points, sl._n_cell_points = [], [], 0   # (last step's list: only an outside holder keeps it alive)
            # (the obstacle rows travel with the step, and so does the copy of the hit ids / visibility flags back: the
            # reference's visible-object bookkeeping -- visible_objects_timestep, current_visible, obstacle_occlusions, the
            # visible multipolygon -- is applied when somebody looks at it, or when the obstacles move on to the next step)
            sm.stage_obstacles(self.fo_obstacles)
            self._scene_step.run(self.ego_pos, self.ego_orientation, ego_v, self.ego_pos_cl, timestep=self.timestep)
            sm.adopt_step(self.ego_pos, self.ego_orientation)
            sm.defer_visible_objects(self.timestep, self.fo_obstacles)
            t0 = self._tick("visibility_ms", t0)
            self.spawn_points = sl.lazy_spawn_points()
        else:
            sm.calc_visible_and_occluded_area(timestep=self.timestep, ego_pos=self.ego_pos,
                                              ego_orientation=self.ego_orientation, obstacles=self.fo_obstacles)
            self.fo_obstacles.update_multipolygon()
            t0 = self._tick("visibility_ms", t0)
            self.spawn_points = sl.find_spawn_points(self.ego_pos, self.ego_orientation, self.ego_pos_cl, ego_v, lazy=True)
        t0 = self._tick("spawn_ms", t0)
        self.agent_manager.attach_batch(self.spawn_locator.batch)
        if self.debug:
            for sp in self.spawn_points:
                print("Phantom agent of type {} added to scenario at position {}".format(sp.agent_type, sp.position))
        self.agent_manager.update_real_agents(self.predictions)
        if self.include_real_agents and self.predictions:
            # EXTENSION (accelerator.include_real_agents, off by default): the real agents' predictions join the sweep
            types = {}
            for oid in self.predictions:
                ob = self.cr_scenario.obstacle_by_id(oid) if hasattr(self.cr_scenario, "obstacle_by_id") else None
                t = getattr(ob, "obstacle_type", None)
                types[oid] = getattr(t, "value", t) or "car"
            self.agent_manager.set_external_predictions(self.predictions, types)
        if self._one_call and not (self.agent_manager._manual or self.agent_manager._external):
            self.metrics.agents_uploaded()        # fo_step_run wrote the sweep's agent table from the device batch
        self._tick("agents_ms", t0)
        if self._timing_sync:          # (counting them reads the device)
            self.step_timing["n_spawn_points"] = len(self.spawn_points)
        self._tick("evaluate_scenario_ms", t_all)
        return self.sensor_model.visible_area

    def trajectory_safety_assessment(self, trajectory):
        t0 = time.perf_counter()
        metrics, safety_assessment = self.metrics.evaluate_metrics(trajectory)
        st = self.step_timing
        st["assessment_single_ms"] = st.get("assessment_single_ms", 0.0) + (time.perf_counter() - t0) * 1e3
        st["assessment_single_calls"] = st.get("assessment_single_calls", 0) + 1
        return metrics, safety_assessment

    # ---------------------------------------------------------------------------------------- batched entry (new)
    def trajectory_safety_assessment_batch(self, trajectories, mode="reduced", shard=None):
        """All candidates of a planning step in one launch.  ``trajectories``: list of trajectory objects
        (``.cartesian.{x,y,theta,v,a}``) or a dict of [M,T] arrays / device tensors.  Returns a
        :class:`~frenetix_occlusion.metrics.metric.BatchAssessment` (``.cost [M,16]``, ``.safe [M]`` on the device), or
        None when the host knows that there are no phantom agents (every trajectory is then safe, metric.py:44-45;
        while the phantom set of the step has not been looked at from the host, its size stays in HBM and the sweep runs
        over a possibly empty set -- every trajectory safe as well).  With
        ``mode='full'`` and a list input, later ``trajectory_safety_assessment(t)`` calls for the same objects are
        served from this batch.

        ``shard`` (one process per GPU, BASELINE configs[3]): True (the default ``torch.distributed`` group), a process
        group or a :class:`~frenetix_occlusion.distributed.CostGather` -- every rank runs the same planning step
        (``evaluate_scenario`` is replicated: cheaper than a broadcast) and calls this with the same candidates; each
        evaluates its block of them and ONE all-gather of the cost rows gives every rank ``cost [M,16]`` / ``safe [M]`` of
        all candidates (``distributed.select_trajectory`` then picks the same trajectory everywhere)."""
        remember = trajectories if (mode == "full" and not isinstance(trajectories, dict)) else None
        t0 = time.perf_counter()
        ba = self.metrics.evaluate_batch(trajectories, mode=mode, remember=remember, shard=shard)
        self._tick("assessment_batch_ms", t0)
        self.step_timing["assessment_batch_size"] = 0 if ba is None else len(ba)
        return ba

    def future_visibility_batch(self, trajectories, t_stride=5, n_rays=192):
        """EXTENSION, not part of the reference: per candidate trajectory and every ``t_stride``-th sample, the number
        of currently occluded cells the ego would see from there and the visible polygon's area
        (:meth:`SensorModel.future_visibility`); a planner can turn it into the ``occ_*`` cost terms the reference
        leaves unused.  Returns device tensors ``(revealed [M,K] int32, area [M,K] float64)``."""
        from .metrics.metric import trajectories_to_arrays
        arr = trajectories_to_arrays(trajectories)
        return self.sensor_model.future_visibility(arr["x"], arr["y"], t_stride=t_stride, n_rays=n_rays)

    def future_visibility(self, trajectories, t_stride=5, n_rays=192, fov="full", occluders="now", first_seen=True):
        """EXTENSION, not part of the reference: :meth:`future_visibility_batch` with moving occluders, the sensor's field
        of view and first-seen counts (:meth:`SensorModel.future_visibility_ex`; returns its
        :class:`~frenetix_occlusion.sensor_model.FutureVisibility`).  Pose k is trajectory sample k ``t_stride``.

        ``fov``: ``"full"`` (world-aligned full circle), ``"sensor"`` (``sensor_model.sensor_angle``) or degrees; an open
        fan turns with the trajectory's ``theta`` at the pose.  ``occluders``: ``"now"`` (the obstacles of the last
        ``evaluate_scenario``, one slice), ``"predicted"`` (that call's ``predictions``: obstacle id at ``pos_list[k
        t_stride]`` / ``orientation_list[k t_stride]``, held at the last entry; obstacles without a prediction stay where
        they are), ``"scenario"`` (the recorded states at ``timestep + k t_stride``, ``FOObstacles.rows_at``) or
        ``(corners [S, O, 4, 2], flags [S, O])``.  ``first_seen``: ``revealed_new`` / ``revealed_any`` as well."""
        from .metrics.metric import trajectories_to_arrays
        from .sensor_model import FutureVisibility
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("future_visibility needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        M, T = np.shape(arr["x"])
        K = (T + t_stride - 1) // t_stride
        if isinstance(fov, str):
            if fov not in ("full", "sensor"):
                raise ValueError(f"fov: 'full', 'sensor' or degrees, not {fov!r}")
            fov_deg = 360.0 if fov == "full" else float(self.sensor_model.sensor_angle)
        else:
            fov_deg = float(fov)
        samples = [k * t_stride for k in range(K)]
        slice_ts = [self.timestep]
        if isinstance(occluders, str):
            if occluders == "now":
                occ = None
            elif occluders == "predicted":
                occ = self.fo_obstacles.predicted_rows(self.predictions, samples)
                slice_ts = [self.timestep + j for j in samples]
            elif occluders == "scenario":
                slice_ts = [self.timestep + j for j in samples]
                occ = self.fo_obstacles.rows_at(slice_ts)
            else:
                raise ValueError(f"occluders: 'now', 'predicted', 'scenario' or (corners, flags), not {occluders!r}")
        else:
            occ, slice_ts = occluders, None
        if M == 0:
            dev = self.sensor_model.device
            e = lambda *shape, dt=torch.int32: torch.empty(shape, dtype=dt, device=dev)
            return FutureVisibility(e(0, K), e(0, K, dt=torch.float64), e(0, K) if first_seen else None,
                                    e(0) if first_seen else None, slice_ts)
        theta = arr["theta"] if fov_deg < 359.9 else None
        out = self.sensor_model.future_visibility_ex(arr["x"], arr["y"], theta, t_stride=t_stride, n_rays=n_rays, fov=fov_deg,
                                                     occluders=occ, first_seen=first_seen)
        out.slice_timesteps = slice_ts
        return out

    def hidden_reach(self, trajectories, v_max=None, margin=None, inflate=0.0, metric="euclid", flow="any"):
        """EXTENSION, not part of the reference: where road users the ego cannot see may be during the planning horizon, and
        which candidate trajectories drive through such road (:meth:`SensorModel.hidden_reach`; returns its
        :class:`~frenetix_occlusion.sensor_model.HiddenReach`: ``arrival`` map, ``cells [M, T]``, ``first [M]``,
        ``slack [M]``).  ``trajectories`` as for :meth:`future_visibility`, sample k at ``k dt``; the footprint is the ego
        rectangle of ``vehicle_params`` grown by ``inflate`` (m).  ``v_max`` / ``margin`` default to
        ``accelerator.occlusion_memory``'s values, so that the forecast and the memory speak of the same road user; with the
        memory enabled the sources are its hidden set of this step, otherwise all road that is not visible.  ``metric``:
        "euclid" -- the reach is a disc around every hidden cell, also across what is not road -- or "road": no cell is reached
        earlier than the distance along the road allows (hidden road behind a building block does not arrive through it).
        ``flow`` (with "road"): "any" -- along the road in any direction, the call for pedestrians -- or "lanes": hidden VEHICLES
        follow the driving direction of the lanes (no arrival down the ego's own lane or against a one-way street)."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_reach needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vehicle = _vehicle_tuple(self.vehicle_params)[:3]      # length, width, wb_rear_axle
        return self.sensor_model.hidden_reach(arr["x"], arr["y"], arr["theta"], vehicle=vehicle,
                                              v_max=om["v_max"] if v_max is None else v_max,
                                              margin=om["margin"] if margin is None else margin, dt=self.dt, inflate=inflate,
                                              metric=metric, flow=flow)

    def hidden_clearance(self, trajectories, v_cap=None, margin=None, inflate=0.0, metric="euclid", flow="any"):
        """EXTENSION, not part of the reference: one device pass that answers :meth:`hidden_reach` for every hidden-user speed
        up to ``v_cap`` and grades each candidate by the slowest hidden road user that could meet it
        (:meth:`SensorModel.hidden_clearance`; returns its :class:`~frenetix_occlusion.sensor_model.HiddenClearance`: ``key``
        map, ``qmin [M, T]``, ``.reach(v_max)`` -> (hit, first, slack), ``.critical_speed()`` -> ``[M]`` m/s).  Arguments and
        defaults as for :meth:`hidden_reach` (``v_cap`` / ``margin``: ``accelerator.occlusion_memory``'s values).  How many
        footprint cells are reached is not part of the result."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_clearance needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vehicle = _vehicle_tuple(self.vehicle_params)[:3]      # length, width, wb_rear_axle
        return self.sensor_model.hidden_clearance(arr["x"], arr["y"], arr["theta"], vehicle=vehicle,
                                                  v_cap=om["v_max"] if v_cap is None else v_cap,
                                                  margin=om["margin"] if margin is None else margin, dt=self.dt,
                                                  inflate=inflate, metric=metric, flow=flow)

    def hidden_witness(self, trajectories, v_max=None, margin=None, inflate=0.0, flow="any"):
        """EXTENSION, not part of the reference: :meth:`hidden_reach` with ``metric="road"`` and, per candidate, the route behind
        its finding -- the cell where hidden traffic first meets it, the hidden cell that traffic starts from and the cheapest
        route between them (:meth:`SensorModel.hidden_witness`; returns its :class:`~frenetix_occlusion.sensor_model.HiddenWitness`,
        whose ``reach`` is the forecast itself).  Arguments and defaults as for :meth:`hidden_reach`; ``flow="lanes"`` for hidden
        vehicles, ``flow="any"`` for pedestrians.  :meth:`add_witness_agents` turns selected witnesses into phantom agents."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_witness needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vehicle = _vehicle_tuple(self.vehicle_params)[:3]      # length, width, wb_rear_axle
        return self.sensor_model.hidden_witness(arr["x"], arr["y"], arr["theta"], vehicle=vehicle,
                                                v_max=om["v_max"] if v_max is None else v_max,
                                                margin=om["margin"] if margin is None else margin, dt=self.dt, inflate=inflate,
                                                flow=flow)

    def hidden_brake(self, trajectories, a_brake=None, v_max=None, margin=None, inflate=0.0, metric="euclid", flow="any"):
        """EXTENSION, not part of the reference: :meth:`hidden_reach` and, per candidate, the fail-safe question -- if the ego
        follows it until sample b and then brakes at ``a_brake``, does it come to rest before it enters road hidden traffic could
        have reached by then?  (:meth:`SensorModel.hidden_brake`; returns its :class:`~frenetix_occlusion.sensor_model.HiddenBrake`:
        ``commit [M]`` the first b from which it does not, -1 = never within the horizon; ``brake_first``, ``stop [M, T]``;
        ``reach`` the forecast itself.)  ``a_brake`` defaults to ``vehicle_params.a_max``; the speeds are the trajectories' own
        ``v``.  The other arguments and defaults as for :meth:`hidden_reach`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        return self.sensor_model.hidden_brake(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3],
                                              v_max=om["v_max"] if v_max is None else v_max,
                                              margin=om["margin"] if margin is None else margin, dt=self.dt,
                                              a_brake=vt[4] if a_brake is None else a_brake, inflate=inflate, metric=metric, flow=flow)

    def hidden_brake_ladder(self, trajectories, decelerations=None, starts=None, v_max=None, margin=None, inflate=0.0, metric="euclid",
                            flow="any"):
        """EXTENSION, not part of the reference: the fail-safe question of :meth:`hidden_brake` at a ladder of decelerations from one
        launch, and per candidate and brake start the gentlest level that keeps the moving ego clear of hidden traffic -- a brake
        threat number against hidden traffic (:meth:`SensorModel.hidden_brake_ladder`; returns its
        :class:`~frenetix_occlusion.sensor_model.HiddenBrakeLadder`: ``required``, ``last_unclear [M, B]``, ``commit [M, K]``,
        ``brake_first``, ``stop [M, B, K]``; ``.required_deceleration()``, ``.brake_threat_number(a_max)``, ``.monotone()``).
        ``decelerations`` defaults to 0.5, 1.0, ... up to ``vehicle_params.a_max``, with ``a_max`` itself appended if it is not on
        that grid (more than 64 levels are refused); ``starts`` (None = every sample) is the number of brake starts considered.
        The other arguments and defaults as for :meth:`hidden_brake`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake_ladder needs a previous evaluate_scenario")
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        if decelerations is None:
            decelerations = _default_brake_ladder(vt[4], "hidden_brake_ladder")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        return self.sensor_model.hidden_brake_ladder(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3],
                                                     v_max=om["v_max"] if v_max is None else v_max,
                                                     margin=om["margin"] if margin is None else margin, dt=self.dt,
                                                     decelerations=decelerations, starts=starts, inflate=inflate, metric=metric, flow=flow)

    def hidden_brake_classes(self, trajectories, speeds, a_brake=None, margin=None, inflate=0.0, metric="euclid", flow="any"):
        """EXTENSION, not part of the reference: the fail-safe question of :meth:`hidden_brake` for several hidden road users at
        once -- ``speeds`` (m/s, 1 .. 8 values: a pedestrian, a cyclist, a car) -- from one clearance and one walk over its key map
        (:meth:`SensorModel.hidden_brake_classes`; returns its :class:`~frenetix_occlusion.sensor_model.HiddenBrakeClasses`:
        ``commit [C, M]``, ``first [C, M]``, ``brake_first [C, M, T]``, ``stop [M, T]``, row c as ``hidden_brake(v_max=speeds[c])``
        gives them; ``.critical_speed()`` the slowest of them a candidate is not fail-safe against).  Defaults as for
        :meth:`hidden_brake`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake_classes needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        return self.sensor_model.hidden_brake_classes(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3], speeds=speeds,
                                                      margin=om["margin"] if margin is None else margin, dt=self.dt,
                                                      a_brake=vt[4] if a_brake is None else a_brake, inflate=inflate, metric=metric,
                                                      flow=flow)

    def hidden_brake_users(self, trajectories, users, a_brake=None, margin=None, inflate=0.0):
        """EXTENSION, not part of the reference: the fail-safe question of :meth:`hidden_brake_classes` for hidden road users that do
        not share a forecast -- ``users`` is 1 .. 8 triples ``(speed, metric, flow)``, say ``(2.0, "road", "any")`` for a pedestrian
        and ``(7.0, "road", "lanes")``, ``(13.9, "road", "lanes")`` for a cyclist and a car -- from one clearance per distinct
        ``(metric, flow)`` and ONE walk of every braking manoeuvre (:meth:`SensorModel.hidden_brake_users`; returns its
        :class:`~frenetix_occlusion.sensor_model.HiddenBrakeUsers`: ``commit [C, M]``, ``first [C, M]``, ``brake_first [C, M, T]``,
        ``stop [M, T]``, row c as ``hidden_brake(v_max=speed_c, metric=metric_c, flow=flow_c)`` gives them; ``.critical_user()`` the
        slowest user a candidate is not fail-safe against).  Defaults as for :meth:`hidden_brake_classes`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake_users needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        return self.sensor_model.hidden_brake_users(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3], users=users,
                                                    margin=om["margin"] if margin is None else margin, dt=self.dt,
                                                    a_brake=vt[4] if a_brake is None else a_brake, inflate=inflate)

    def hidden_brake_ladder_users(self, trajectories, users, decelerations=None, starts=None, detail=False, margin=None, inflate=0.0):
        """EXTENSION, not part of the reference: the brake threat number of :meth:`hidden_brake_ladder` against hidden road users that
        do not share a forecast -- ``users`` as for :meth:`hidden_brake_users` -- from one clearance per distinct ``(metric, flow)``
        and ONE walk of every braking manoeuvre at every deceleration (:meth:`SensorModel.hidden_brake_ladder_users`; returns its
        :class:`~frenetix_occlusion.sensor_model.HiddenBrakeLadderUsers`: ``required_all``, ``last_unclear_all``, ``blocking [M, B]``,
        per user ``required``, ``last_unclear [C, M, B]``, ``commit [C, M, L]``, ``first [C, M]``; ``.required_deceleration(user)``,
        ``.brake_threat_number(a_max, user)``, ``.monotone(user)``, ``.blocking_users()``; with ``detail`` also ``brake_first`` and
        ``stop``).  ``decelerations`` and ``starts`` default as for :meth:`hidden_brake_ladder`, the rest as for
        :meth:`hidden_brake_users`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake_ladder_users needs a previous evaluate_scenario")
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        if decelerations is None:
            decelerations = _default_brake_ladder(vt[4], "hidden_brake_ladder_users")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        return self.sensor_model.hidden_brake_ladder_users(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3], users=users,
                                                           margin=om["margin"] if margin is None else margin, dt=self.dt,
                                                           decelerations=decelerations, starts=starts, detail=detail, inflate=inflate)

    def hidden_brake_verdict(self, trajectories, users, commit_min, starts=None, a_brake=None, cost=None, safe=None, margin=None,
                             inflate=0.0):
        """EXTENSION, not part of the reference: the fail-safe VERDICT against the hidden road users of :meth:`hidden_brake_users` --
        for how many of the first ``starts`` brake starts (None: all) each candidate can still brake clear of every user, and which
        user ends them (:meth:`SensorModel.hidden_brake_verdict`; returns its
        :class:`~frenetix_occlusion.sensor_model.HiddenBrakeVerdict`: ``fail_safe [M]``, ``user [M]``, ``commit [C, M]``,
        ``first [C, M]``).  With ``cost [M, 16]`` / ``safe [M]`` of a sweep over the same candidates the verdict is folded into the
        two reserved columns, and candidates with ``fail_safe < commit_min`` lose their safety flag.  Defaults as for
        :meth:`hidden_brake_users`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake_verdict needs a previous evaluate_scenario")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        return self.sensor_model.hidden_brake_verdict(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3], users=users,
                                                      margin=om["margin"] if margin is None else margin, dt=self.dt,
                                                      a_brake=vt[4] if a_brake is None else a_brake, starts=starts,
                                                      commit_min=commit_min, cost=cost, safe=safe, inflate=inflate)

    def hidden_brake_ladder_verdict(self, trajectories, users, a_limit=None, starts=None, levels=None, cost=None, safe=None, margin=None,
                                    inflate=0.0):
        """EXTENSION, not part of the reference: the LADDER VERDICT against the hidden road users of :meth:`hidden_brake_users` -- the
        gentlest deceleration of the ladder ``levels`` (None: 0.5, 1.0, ... up to the vehicle's ``a_max``) that keeps each candidate
        clear of every user from the WORST of its first ``starts`` brake starts (None: all), and the user that blocks the level below
        (:meth:`SensorModel.hidden_brake_ladder_verdict`; returns its
        :class:`~frenetix_occlusion.sensor_model.HiddenBrakeLadderVerdict`: ``need``, ``at``, ``blocking``, ``user [M]``,
        ``decel [M]``, ``need_of``, ``first [C, M]``; ``.required_deceleration()``, ``.brake_threat_number(a_max)``,
        ``.critical_user()``).  With ``cost [M, 16]`` / ``safe [M]`` of a sweep over the same candidates the deceleration and the
        user are folded into the two reserved columns, and candidates that need more than ``a_limit`` (None: the vehicle's
        ``a_max``) or more than the ladder holds lose their safety flag.  The other defaults as for :meth:`hidden_brake_users`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake_ladder_verdict needs a previous evaluate_scenario")
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        if levels is None:
            levels = _default_brake_ladder(vt[4], "hidden_brake_ladder_verdict")
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        return self.sensor_model.hidden_brake_ladder_verdict(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3], users=users,
                                                             margin=om["margin"] if margin is None else margin, dt=self.dt,
                                                             levels=levels, starts=starts, a_limit=vt[4] if a_limit is None else a_limit,
                                                             cost=cost, safe=safe, inflate=inflate)

    def phantom_kind(self, type_name):
        """``(type_name, length, width)`` of the phantom :class:`FOAgentManager` makes of ``type_name``: the configuration's
        dimensions with the prediction's size factors (agent.py:402-405), so that the harm model's mass by size is the sweep's"""
        am = self.config["agent_manager"]
        key = str(type_name).lower()
        if not isinstance(am.get(key), dict) or "length" not in am[key] or "width" not in am[key]:
            raise ValueError(f"hidden_brake_impact: the configuration's agent_manager has no dimensions for the type {type_name!r}: "
                             "hand kinds over as (type_name, length, width)")
        pr = am["prediction"]
        big = key == "bicycle"
        fl = pr["size_factor_length_l"] if big else pr["size_factor_length_s"]
        fw = pr["size_factor_width_l"] if big else pr["size_factor_width_s"]
        return (str(type_name), float(am[key]["length"]) * float(fl), float(am[key]["width"]) * float(fw))

    def hidden_brake_impact(self, trajectories, users, kinds=None, harm_limit=None, starts=None, a_brake=None, cost=None, safe=None,
                            margin=None, inflate=0.0, approach="head_on", heading_slack=0.0):
        """EXTENSION, not part of the reference: the IMPACT VERDICT against the hidden road users of :meth:`hidden_brake_users` -- the
        worst harm that remains after braking at ``a_brake`` (None: the vehicle's ``a_max``) from one of the first ``starts`` brake
        starts (None: all): the reference's MAIS3+ probability at the speed the ego has left where it is hit, head-on and at the
        worst area of impact (:meth:`SensorModel.hidden_brake_impact`; returns its
        :class:`~frenetix_occlusion.hidden_traffic.HiddenBrakeImpact`: ``harm [M, 2]``, ``user [M]``, ``speed``, ``at``, ``commit``,
        ``first [C, M]``; ``.obstacle_harm()``, ``.ego_harm()``, ``.critical_user()``, ``.impact_speed()``, ``.harm_of(c)``).
        ``kinds``: one ``(type_name, length, width)`` or one type name per user -- a name alone takes the dimensions of the phantom
        the agent manager makes of that type (:meth:`phantom_kind`), so the numbers sit beside the sweep's ``max_obst_harm``; None:
        Pedestrian, Bicycle, Car by ascending speed, possible only with exactly three users.  With ``cost [M, 16]`` / ``safe [M]``
        of a sweep over the same candidates the obstacle's harm and the user are folded into the two reserved columns, and
        candidates whose harm exceeds ``harm_limit`` (None: the configuration's ``metric_thresholds.harm``; ``null`` there: inf)
        lose their safety flag.  ``approach="lanes"`` prices every user with flow ``"lanes"`` at the worst closing speed the lanes'
        driving directions allow where it meets the ego, within ``heading_slack`` radians of them, instead of head-on (``speed`` is
        then None; ``closing``, ``cosine``, ``.closing_speed()``, ``.approach_cosine()``).  The other defaults as for
        :meth:`hidden_brake_users`."""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError("hidden_brake_impact needs a previous evaluate_scenario")
        users = tuple(users)
        kinds = self._hidden_kinds(users, kinds, "hidden_brake_impact")
        harm_limit = self._hidden_harm_limit(harm_limit)
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        return self.sensor_model.hidden_brake_impact(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3], ego_mass=vt[3],
                                                     users=users, kinds=kinds, margin=om["margin"] if margin is None else margin,
                                                     dt=self.dt, a_brake=vt[4] if a_brake is None else a_brake, starts=starts,
                                                     harm_limit=harm_limit, cost=cost, safe=safe, inflate=inflate, approach=approach,
                                                     heading_slack=heading_slack)

    def _hidden_kinds(self, users, kinds, fn):
        """the ``kinds`` of ``fn`` (hidden_brake_impact, hidden_brake_harm_ladder) as ``(type_name, length, width)`` per user: a name
        alone takes the phantom's dimensions; None: Pedestrian, Bicycle, Car by ascending speed, with exactly three users"""
        if kinds is None:
            if len(users) != 3:
                raise ValueError(f"{fn}: kinds is required unless exactly three users are given "
                                 "(then: Pedestrian, Bicycle, Car by ascending speed)")
            order = sorted(range(3), key=lambda c: float(users[c][0]))
            kinds = [None] * 3
            for name, c in zip(("Pedestrian", "Bicycle", "Car"), order):
                kinds[c] = name
        return [self.phantom_kind(k) if isinstance(k, str) else tuple(k) for k in kinds]

    def _hidden_harm_limit(self, harm_limit):
        """``harm_limit``, None: the configuration's ``metric_thresholds.harm`` (``null`` there: inf)"""
        if harm_limit is None:
            harm_limit = ((self.config.get("metrics") or {}).get("metric_thresholds") or {}).get("harm")
            harm_limit = float("inf") if harm_limit is None else harm_limit
        return harm_limit

    def hidden_brake_harm_ladder(self, trajectories, users, kinds=None, harm_limit=None, levels=None, starts=None, a_limit=None, cost=None,
                                 safe=None, margin=None, inflate=0.0):
        """EXTENSION, not part of the reference: the HARM LADDER against the hidden road users of :meth:`hidden_brake_users` -- the
        gentlest deceleration of the ladder ``levels`` (None: 0.5, 1.0, ... up to the vehicle's ``a_max``) at which the harm of what
        still hits each candidate stays within ``harm_limit`` (None: the configuration's ``metric_thresholds.harm``; ``null`` there:
        inf) from the WORST of its first ``starts`` brake starts (None: all), and per level the greatest harm it leaves
        (:meth:`SensorModel.hidden_brake_harm_ladder`; returns its :class:`~frenetix_occlusion.hidden_traffic.HiddenBrakeHarmLadder`:
        the tensors of :meth:`hidden_brake_ladder_verdict`, ``harm_at``, ``user_at [M, L]``; ``.required_deceleration()``,
        ``.brake_threat_number(a_max)``, ``.critical_user()``, ``.harm_curve()``, ``.monotone()``).  ``kinds`` as for
        :meth:`hidden_brake_impact`.  With ``cost [M, 16]`` / ``safe [M]`` of a sweep over the same candidates the deceleration and
        the user are folded into the two reserved columns, and candidates that need more than ``a_limit`` (None: the vehicle's
        ``a_max``) or more than the ladder holds lose their safety flag.  Every user is priced head-on
        (:meth:`hidden_brake_harm_ladder_lanes` prices lane-bound users by their approach angle).  The other defaults as for
        :meth:`hidden_brake_users`."""
        return self._hidden_harm_ladder("hidden_brake_harm_ladder", trajectories, users, kinds, harm_limit, levels, starts, a_limit, cost,
                                        safe, margin, inflate)

    def hidden_brake_harm_ladder_lanes(self, trajectories, users, kinds=None, harm_limit=None, levels=None, starts=None, a_limit=None,
                                       cost=None, safe=None, margin=None, inflate=0.0, heading_slack=0.0):
        """EXTENSION, not part of the reference: the HARM LADDER BY APPROACH ANGLE -- :meth:`hidden_brake_harm_ladder` with every
        user with ``flow == "lanes"`` priced at the worst closing speed the lanes' driving directions allow where it meets the ego,
        within 22.5 degrees + ``heading_slack`` (radians) of a direction of the move table, instead of head-on
        (:meth:`SensorModel.hidden_brake_harm_ladder_lanes`; the same result class with ``approach == "lanes"``).  Never above the
        head-on call; the defaults are its sibling's."""
        return self._hidden_harm_ladder("hidden_brake_harm_ladder_lanes", trajectories, users, kinds, harm_limit, levels, starts, a_limit,
                                        cost, safe, margin, inflate, heading_slack=heading_slack)

    def _hidden_harm_ladder(self, fn, trajectories, users, kinds, harm_limit, levels, starts, a_limit, cost, safe, margin, inflate, **lanes):
        """the one body of :meth:`hidden_brake_harm_ladder` and :meth:`hidden_brake_harm_ladder_lanes` (``lanes``: its heading_slack)"""
        from .metrics.metric import trajectories_to_arrays
        from .sweep import _vehicle_tuple
        if self.timestep is None or self.sensor_model.window is None:
            raise RuntimeError(f"{fn} needs a previous evaluate_scenario")
        users = tuple(users)
        kinds = self._hidden_kinds(users, kinds, fn)
        harm_limit = self._hidden_harm_limit(harm_limit)
        vt = _vehicle_tuple(self.vehicle_params)               # length, width, wb_rear_axle, mass, a_max
        if levels is None:
            levels = _default_brake_ladder(vt[4], fn)
        arr = trajectories_to_arrays(trajectories)
        om = self.occlusion_memory
        return getattr(self.sensor_model, fn)(arr["x"], arr["y"], arr["theta"], arr["v"], vehicle=vt[:3], ego_mass=vt[3], users=users,
                                              kinds=kinds, margin=om["margin"] if margin is None else margin, dt=self.dt, levels=levels,
                                              starts=starts, harm_limit=harm_limit, a_limit=vt[4] if a_limit is None else a_limit,
                                              cost=cost, safe=safe, inflate=inflate, **lanes)

    def add_witness_agents(self, witness, max_agents=8, merge_cells=4, agent_type="Car"):
        """EXTENSION, not part of the reference: puts the hidden road users behind a :meth:`hidden_witness` result in front of the
        metric sweep.  ``witness.select(max_agents, merge_cells)`` picks the candidates whose witnesses differ (one per block of
        source cells, earliest first); each becomes a phantom of ``agent_type`` that drives its route at ``witness.speed(m)`` --
        it is at the conflict cell exactly at the sample the forecast named -- over the candidates' horizon
        (:meth:`FOAgentManager.add_route_agent`).  The next ``trajectory_safety_assessment_batch`` evaluates them after the device
        batch's slots, as it does manual agents; the next ``evaluate_scenario`` drops them with the step.  Returns the agents, in
        the order of ``select``.  The witness is the road user that is first by road distance, not the most harmful one, and
        its speed may exceed ``v_max`` by the bound :meth:`HiddenWitness.speed` states."""
        T = int(witness.reach.cells.shape[1])
        picked = witness.select(max_agents=max_agents, merge_cells=merge_cells)
        agents = [self.agent_manager.add_route_agent(route, witness.speed(m), agent_type=agent_type, horizon=(T - 0.5) * witness.dt)
                  for m, route in zip(picked, witness.routes(picked))]     # (T - 0.5: int(horizon / dt) + 1 == T whatever dt rounds to)
        self.metrics.invalidate()
        return agents

    def _update_time_step(self, timestep):
        self.timestep = timestep
        self.sensor_model.timestep = timestep
        self.agent_manager.timestep = timestep

    @staticmethod
    def _load_config(filepath=None):
        """interface.py:227-238 (there the default path is computed but not used; here it is)"""
        if not filepath:
            filepath = os.path.join(os.path.dirname(__file__), "config", "config.yaml")
        with open(filepath, "r") as f:
            return yaml.safe_load(f)
