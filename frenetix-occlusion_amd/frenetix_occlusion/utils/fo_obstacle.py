"""Per-timestep obstacle state cache (mirrors ref: utils/fo_obstacle.py:14-116, helper_functions.py:99-112).

Wraps each scenario obstacle -- a :class:`~frenetix_occlusion.scenario.Obstacle` or a duck-typed CommonRoad obstacle --
and caches pose / corner points / visibility for the current global time step.  ``arrays()`` packs what
``fo_scene_visibility`` consumes.  Pure host bookkeeping (a handful of obstacles); no polygons are built.
"""
import math

import numpy as np

from ..scenario import Obstacle, obstacle_from_commonroad, _CVX, _CVY


def _pyhost():
    from .. import _native
    return _native.pyhost()


# One step's obstacles travel as ONE byte buffer of O rows (csrc/fo_pyhost.c obstacle_rows writes the same layout):
# corners [O,4,2] f64 | centres [O,2] f64 | headings [O] f64 | dimensions [O,2] f64 | flags [O] u8 -- part k starts at byte O * k_AT
ROW_BYTES = 105
CENTRES_AT, HEADINGS_AT, DIMENSIONS_AT, FLAGS_AT = 64, 80, 88, 104
DYNAMIC_CANDIDATE_MASK, DYNAMIC_CANDIDATE_BITS = 13, 5      # flag bits 0 present, 2 dynamic role set; bit 3 bicycle / pedestrian clear


def _split(buf, f64):
    O = len(buf) // ROW_BYTES
    part = lambda a, b: buf[O * a:O * b].view(f64)
    return (part(0, CENTRES_AT).reshape(O, 4, 2), part(CENTRES_AT, HEADINGS_AT).reshape(O, 2), part(HEADINGS_AT, DIMENSIONS_AT),
            part(DIMENSIONS_AT, FLAGS_AT).reshape(O, 2), buf[O * FLAGS_AT:])


def split_rows(host):
    """(corners, centres, headings, dimensions, flags): the parts of a packed host buffer (numpy uint8 [O * ROW_BYTES]) as views"""
    return _split(host, np.float64)


def split_rows_device(d):
    """:func:`split_rows` for a packed buffer that is a torch uint8 tensor"""
    import torch
    return _split(d, torch.float64)


def n_dynamic_candidates(flags):
    """obstacles whose flags allow the dynamic-obstacle rule (present, dynamic role, no bicycle / pedestrian): a count the
    rule launch wants from the host (fo_spawn_rule_params_t::n_dynamic_plus1)"""
    return int(((flags & DYNAMIC_CANDIDATE_MASK) == DYNAMIC_CANDIDATE_BITS).sum())


def resolved_first(name):
    """property ``name`` over ``_name``: the visibility a one-call planning step left pending is applied
    (``resolve_visible_objects``, SensorModel.defer_visible_objects) before the attribute is read; assignable as before"""
    def get(self):
        self.resolve_visible_objects()
        return getattr(self, "_" + name)
    return property(get, lambda self, v: setattr(self, "_" + name, v))


class FOObstacle:
    def __init__(self, obst):
        self.cr_obstacle = obst
        self._o = obst if isinstance(obst, Obstacle) else obstacle_from_commonroad(obst)
        self.obstacle_id = self._o.obstacle_id
        self.obstacle_type = self._o.obstacle_type
        self.obstacle_role = self._o.role
        self.initial_timestep = self._o.initial_time_step
        self.global_timestep = None
        self.relative_time_step = None
        self.current_pos = None
        self.current_orientation = None
        self.current_corner_points = None
        self._owner = None               # the FOObstacles this one belongs to (pending visibility of a one-call step)
        self._current_visible = False
        self._last_visible_at_ts = None

    # visibility of the current step: after a one-call planning step these are read from the step's mirror when somebody looks
    current_visible = resolved_first("current_visible")
    last_visible_at_ts = resolved_first("last_visible_at_ts")

    def resolve_visible_objects(self):
        o = self._owner
        if o is not None and o._pending is not None:
            o._pending()

    @property
    def length(self):
        return self._o.length

    @property
    def width(self):
        return self._o.width

    def update_at_timestep(self, timestep):
        """fo_obstacle.py:79-116: rel = step - initial; 0 -> initial state, >= 1 -> state_list[rel-1], else absent"""
        if self._owner is not None:
            # the last step's visibility first (as FOObstacles.update does): a deferred one-call step must stamp
            # last_visible_at_ts with ITS time step before this obstacle moves on, not overwrite the moved state later
            if self._owner._pending is not None:
                self._owner._pending()
            self._owner._packed = None       # (a single obstacle moved by hand: the owner's packed rows are stale)
        self.global_timestep = timestep
        self.relative_time_step = timestep - self.initial_timestep
        self._current_visible = False
        pose = self._o.pose_at(timestep)
        if pose is None:
            self.current_pos = self.current_orientation = self.current_corner_points = None
            return
        self.current_pos = np.array(pose[:2], dtype=np.float64)
        self.current_orientation = float(pose[2])
        self.current_corner_points = self._o.corners(pose)

    @property
    def occludes(self):
        return str(self.obstacle_type).lower() != "bicycle"  # sensor_model.py:177 (Q10)


class FOObstacles:
    def __init__(self, cr_obstacles):
        self.cr_obstacles = list(cr_obstacles)
        self.fo_obstacles = [FOObstacle(o) for o in self.cr_obstacles]
        self._pending = None                        # SensorModel.resolve_visible_objects while a step's visibility is unread
        self._table = None                          # per-obstacle state table for update() (built on first use)
        self._packed = None                         # the current step's rows in the layout of packed()
        for o in self.fo_obstacles:
            o._owner = self
        self._visible_obstacle_multipolygon = None  # list of [4,2] corner arrays of the visible obstacles

    visible_obstacle_multipolygon = resolved_first("visible_obstacle_multipolygon")

    def resolve_visible_objects(self):
        if self._pending is not None:
            self._pending()

    def __iter__(self):
        return iter(self.fo_obstacles)

    def __len__(self):
        return len(self.fo_obstacles)

    def add(self, cr_obstacle):
        self.cr_obstacles.append(cr_obstacle)
        self.fo_obstacles.append(FOObstacle(cr_obstacle))
        self.fo_obstacles[-1]._owner = self
        self._table = self._packed = None

    def update(self, timestep):
        if self._pending is not None:     # the last step's visibility first: last_visible_at_ts outlives the step
            self._pending()
        O = len(self.fo_obstacles)
        if O == 0:
            return
        # All obstacles of the step in a handful of array expressions (the per-obstacle form -- FOObstacle.update_at_timestep,
        # kept for callers that move one obstacle -- costs ~10 us each): poses from a table [O, steps, 3] made once, corner
        # points by the formula of scenario.Obstacle.corners, written straight into the rows a one-call step uploads.
        H = _pyhost()
        if H is None and O < 4:          # (without the C helper the array form only pays from a handful of obstacles on)
            for o in self.fo_obstacles:
                o.update_at_timestep(timestep)
            return
        tb = self._table
        if tb is None:
            tb = self._table = self._build_table()
        host, corn, cen, yaw, dims, flags, present, ya = self._rows(tb, timestep, H)
        t0 = tb["t0_list"]
        for i, o in enumerate(self.fo_obstacles):
            o.global_timestep = timestep
            o.relative_time_step = timestep - t0[i]
            o._current_visible = False
            if present[i]:
                o.current_pos, o.current_orientation, o.current_corner_points = cen[i], float(ya[i]), corn[i]
            else:
                o.current_pos = o.current_orientation = o.current_corner_points = None
        self._packed = (host, corn, cen, flags, yaw, dims)

    def _rows(self, tb, timestep, H):
        """the rows of time step ``timestep`` in a fresh host buffer (layout of ``packed()``) -- what ``update`` writes"""
        O = len(self.fo_obstacles)
        host = np.empty(O * ROW_BYTES, dtype=np.uint8)                 # fresh per step: last step's views stay what they were
        corn = host[:O * CENTRES_AT].view(np.float64).reshape(O, 4, 2)
        cen = host[O * CENTRES_AT:O * HEADINGS_AT].view(np.float64).reshape(O, 2)
        yaw = host[O * HEADINGS_AT:O * DIMENSIONS_AT].view(np.float64)
        dims = host[O * DIMENSIONS_AT:O * FLAGS_AT].view(np.float64).reshape(O, 2)
        flags = host[O * FLAGS_AT:]
        if H is not None:
            # csrc/fo_pyhost.c obstacle_rows: the same operations in the same order, in C (the array expressions below cost
            # ~40 us of interpreter time whatever O is)
            present = np.empty(O, dtype=np.uint8)
            H.obstacle_rows(tb["P"], tb["L"], tb["t0"], tb["static_u8"], tb["vx"], tb["vy"], tb["dims"], tb["flags"], int(timestep),
                            host, present)
            ya = yaw
        else:
            rel = np.where(tb["static"], 0, timestep - tb["t0"])
            present = (rel >= 0) & (rel < tb["L"])
            pose = tb["P"][tb["ar"], np.clip(rel, 0, tb["L"] - 1)]          # [O, 3]
            ya = pose[:, 2]
            c = np.array([math.cos(v) for v in ya])[:, None]                # (math.cos, as Obstacle.corners: numpy's differs in the last bit)
            s = np.array([math.sin(v) for v in ya])[:, None]
            corn[:, :, 0] = pose[:, 0:1] + (c * tb["vx"] - s * tb["vy"])
            corn[:, :, 1] = pose[:, 1:2] + (s * tb["vx"] + c * tb["vy"])
            cen[:] = pose[:, :2]
            yaw[:] = ya
            dims[:] = tb["dims"]
            flags[:] = tb["flags"]
            if not present.all():
                gone = ~present
                corn[gone] = 0.0; cen[gone] = 0.0; yaw[gone] = 0.0; dims[gone] = 0.0; flags[gone] = 0
        return host, corn, cen, yaw, dims, flags, present, ya

    def rows_at(self, timesteps):
        """corner points [S, O, 4, 2] and flags [S, O] (uint8, as ``arrays_full``) of the obstacles at each of
        ``timesteps``: the rows ``update(t)`` would write, bit for bit, without moving any obstacle (occluder slices for
        ``SensorModel.future_visibility_ex``)"""
        O, S = len(self.fo_obstacles), len(timesteps)
        corn, flags = np.zeros((S, O, 4, 2)), np.zeros((S, O), dtype=np.uint8)
        if O == 0:
            return corn, flags
        tb = self._table
        if tb is None:
            tb = self._table = self._build_table()
        H = _pyhost()
        for i, t in enumerate(timesteps):
            _, c, _, _, _, f, _, _ = self._rows(tb, int(t), H)
            corn[i], flags[i] = c, f
        return corn, flags

    def predicted_rows(self, predictions, samples):
        """corner points [S, O, 4, 2] and flags [S, O] with every obstacle that has a prediction moved to it: slice s
        puts obstacle ``id`` at ``pos_list[j]`` / ``orientation_list[j]`` of ``predictions[id]`` with j = samples[s] held at
        the prediction's last entry (the corner formula of ``scenario.Obstacle.corners``, the obstacle's own dimensions);
        obstacles without a prediction keep the rows of the current step (``arrays_full``) in every slice"""
        corn0, _, flags0, _, _ = self.arrays_full()
        S = len(samples)
        corn = np.repeat(np.asarray(corn0, dtype=np.float64)[None], S, axis=0)
        flags = np.repeat(np.asarray(flags0, dtype=np.uint8)[None], S, axis=0)
        preds = predictions or {}
        if not preds:
            return corn, flags
        tb = self._table
        if tb is None:
            tb = self._table = self._build_table()
        for i, o in enumerate(self.fo_obstacles):
            p = preds.get(o.obstacle_id)
            if p is None:
                continue
            pos, ori = np.asarray(p["pos_list"], dtype=np.float64), np.asarray(p["orientation_list"], dtype=np.float64)
            n = min(len(pos), len(ori))
            if n == 0:
                continue
            for s, j in enumerate(samples):
                jj = min(int(j), n - 1)
                corn[s, i] = o._o.corners((float(pos[jj, 0]), float(pos[jj, 1]), float(ori[jj])))
                flags[s, i] = tb["flags"][i]      # a predicted obstacle is present
        return corn, flags

    def _build_table(self):
        obs = [o._o for o in self.fo_obstacles]
        O = len(obs)
        static = np.array([o.role == "static" for o in obs])
        L = np.array([1 if st else 1 + len(o.states) for o, st in zip(obs, static)])
        P = np.zeros((O, int(L.max()), 3))
        for i, o in enumerate(obs):
            P[i, 0] = o.initial[:3]
            if L[i] > 1:
                P[i, 1:L[i]] = np.asarray(o.states)[:, :3]
        l2 = np.array([o.length / 2.0 for o in obs])[:, None]
        w2 = np.array([o.width / 2.0 for o in obs])[:, None]
        flags = np.array([1 | (2 if f.occludes else 0) | (4 if f.obstacle_role == "dynamic" else 0)
                          | (8 if str(f.obstacle_type).lower() in ("bicycle", "pedestrian") else 0) for f in self.fo_obstacles],
                         dtype=np.uint8)
        return dict(static=static, static_u8=static.astype(np.uint8), t0=np.array([o.initial_time_step for o in obs], dtype=np.int64),
                    t0_list=[f.initial_timestep for f in self.fo_obstacles], L=L.astype(np.int64), P=np.ascontiguousarray(P),
                    ar=np.arange(O), vx=np.ascontiguousarray(_CVX[None, :] * l2), vy=np.ascontiguousarray(_CVY[None, :] * w2),
                    dims=np.array([(float(f.length), float(f.width)) for f in self.fo_obstacles]).reshape(O, 2), flags=flags)

    def update_multipolygon(self):
        self._visible_obstacle_multipolygon = [o.current_corner_points for o in self.fo_obstacles if o._current_visible]

    def _rows_of_state(self):
        """the tuple ``update`` leaves in ``_packed``, built from the obstacles' own state (they were moved one by one)"""
        host = np.zeros(len(self.fo_obstacles) * ROW_BYTES, dtype=np.uint8)
        corn, cen, yaw, dims, flags = split_rows(host)
        for i, o in enumerate(self.fo_obstacles):
            if o.current_pos is None:
                continue
            corn[i], cen[i], yaw[i], dims[i] = o.current_corner_points, o.current_pos, o.current_orientation, (o.length, o.width)
            flags[i] = (1 | (2 if o.occludes else 0) | (4 if o.obstacle_role == "dynamic" else 0)
                        | (8 if str(o.obstacle_type).lower() in ("bicycle", "pedestrian") else 0))
        return host, corn, cen, flags, yaw, dims

    def packed(self):
        """the rows ``SensorModel.stage_obstacles`` hands to a one-call step, one host buffer in the layout of
        ``SensorModel.upload_obstacles``: corners [O,4,2] | centres [O,2] | headings [O] | dimensions [O,2] | flags [O]"""
        return (self._packed or self._rows_of_state())[0]

    def arrays(self):
        """corner points [O,4,2], centres [O,2], flags uint8 [O] (bit0 present at this step, bit1 occludes)"""
        _, corn, cen, flags, _, _ = self._packed or self._rows_of_state()
        return corn, cen, flags & 3

    def arrays_full(self):
        """``arrays()`` plus what the spawn rule families read (fo_scene_spawn_rules): headings [O], dimensions [O,2]
        (length, width), and two more flag bits -- bit2 dynamic role, bit3 type bicycle or pedestrian
        (spawn_locator.py:209-210).  The visibility kernels test bits 0 and 1 only, so one flag array serves both."""
        return (self._packed or self._rows_of_state())[1:]
