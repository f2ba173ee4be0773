"""Hidden traffic (an extension): the reach forecast for one speed, the clearance that serves every speed up to
a cap, the witnesses, and the brake clearance with its siblings (by classes, by road users, at a ladder of decelerations, and the
ladder by road users), the device pose preparation and the fail-safe verdict that folds into a step's cost rows.  The functions
that take ``self`` are :class:`~frenetix_occlusion.sensor_model.SensorModel`'s methods."""
import ctypes as C
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .cell_window import CellWindow
from .occlusion_memory import occlusion_memory_r2


def hidden_reach_r2(v_max, dt, margin, cell_size, J):
    """the reach table of the hidden-traffic forecast: ``R2[j] = occlusion_memory_r2(v_max, j dt, margin,
    cell_size)`` for the J samples of a horizon -- what the occlusion memory uses for a step of j timesteps"""
    return np.array([occlusion_memory_r2(v_max, j * float(dt), margin, cell_size) for j in range(int(J))], dtype=np.int32)


def hidden_reach_road_units(r2):
    """the reach table of the forecast's road metric: ``L[j] = isqrt(169 R2[j])`` -- the Euclidean reach in the
    units of the road distance (12 per axis step, 17 per diagonal step, 13 per cell of Euclidean length), host int32 [J]"""
    return np.array([math.isqrt(169 * int(v)) for v in r2], dtype=np.int32)


HIDDEN_REACH_METRICS = ("euclid", "road")
HIDDEN_REACH_FLOWS = ("any", "lanes")      # "lanes": the road metric bound to the lanes' driving direction (DESIGN.md §5.10 "Lane flow")


def unit_headings(theta):
    """(cos, sin) of the sample headings as a float64 host array [..., 2]: the ONE place the forecast's footprints get their
    rotation from (the device takes no sine or cosine; a checker is handed these numbers as data)"""
    th = theta.detach().cpu().numpy() if torch.is_tensor(theta) else theta
    th = np.asarray(th, dtype=np.float64)
    return np.stack((np.cos(th), np.sin(th)), -1)


@dataclass
class HiddenReach:
    """what :meth:`SensorModel.hidden_reach` returns (device tensors): ``arrival [ny, nx]`` uint8 over ``window`` -- the
    first horizon sample at which a road user hidden now may be in the cell, 255 = not within the horizon or not road;
    ``cells [M, T]`` int32 -- cells of the ego rectangle at sample k that hidden traffic may have reached by then;
    ``first [M]`` int32 -- the first such sample, -1 = none; ``slack [M]`` int32 -- min over samples and footprint cells of
    (arrival - k), ``SLACK_NONE`` where the trajectory meets no reachable cell (``slack <= 0`` iff ``first >= 0``).
    ``r2`` (host int32 [J]) is the reach table, ``heading`` the (cos, sin) [M, T, 2] the footprints were turned by,
    ``from_memory`` whether the sources were the occlusion memory's hidden set of this step, ``from_vehicle_memory`` whether
    that set was the memory's vehicle layer V (``flow="lanes"`` with ``enable_occlusion_memory(vehicles="lanes")``).  ``metric``: "euclid" (reach as
    a disc around every hidden cell) or "road" (that, and no earlier than the distance along passable cells allows);
    ``reach`` (host int32 [J]) is the table in road-distance units (:func:`hidden_reach_road_units`), ``road_dist [ny, nx]``
    uint16 the road distance itself, 65535 = impassable or beyond ``reach[-1]`` (None for "euclid").  ``flow``: "any" (a hidden
    road user moves along the road in any direction) or "lanes" (a hidden vehicle obeys the driving direction of the lanes, DESIGN.md
    §5.10 "Lane flow"; ``road_dist`` then holds the distance over allowed steps, ``d_flow``)."""
    arrival: torch.Tensor
    cells: torch.Tensor
    first: torch.Tensor
    slack: torch.Tensor
    r2: np.ndarray
    window: CellWindow
    heading: Optional[torch.Tensor] = None
    from_memory: bool = False
    from_vehicle_memory: bool = False      # ... and that set was its vehicle layer V, not H (flow="lanes" only)
    metric: str = "euclid"
    reach: Optional[np.ndarray] = None
    road_dist: Optional[torch.Tensor] = None
    flow: str = "any"

    SLACK_NONE = 2 ** 31 - 1


@dataclass
class HiddenClearance:
    """what :meth:`SensorModel.hidden_clearance` returns (device tensors; DESIGN.md §5.10 "Clearance and critical speed"):
    ``key [ny, nx]`` int32 over ``window`` -- ``169 D2`` ("euclid") or ``max(169 D2, d^2)`` ("road") on road cells within the cap,
    ``NONE`` = INT32_MAX elsewhere; ``qmin [M, T]`` int32 -- the minimum of ``key`` over the ego rectangle at sample k, ``NONE``
    where the footprint holds no road cell within the cap and for ``k >= lengths[m]``; ``dist [ny, nx]`` uint16 the road
    distance (65535 = impassable or beyond ``isqrt(169 r2_cap)``; None for "euclid"); ``heading`` the (cos, sin) [M, T, 2] the
    footprints were turned by (hand it to a later call of the same candidates as ``heading=``); ``r2_cap`` the cap in squared
    cells: every reach table whose last entry is ``<= r2_cap`` is served.  ``dt``, ``margin``, ``cell_size`` are what the
    tables of :meth:`reach` are made of, ``from_memory`` whether the sources were the occlusion memory's hidden set
    (``from_vehicle_memory``: its vehicle layer V).  ``flow``:
    "any", or "lanes" -- ``d`` is the distance over the steps the lanes' driving direction allows (``d_flow``, which ``dist`` then holds).

    For any such table ``A(g) <= j`` iff ``key(g) <= 169 R2[j]``, so ``cells > 0``, ``first`` and ``slack`` of
    :meth:`SensorModel.hidden_reach` follow from ``qmin`` alone (:meth:`reach`).  The COUNT ``cells[m, k]`` itself does not:
    ``qmin`` keeps the nearest footprint cell, not how many there are."""
    key: torch.Tensor
    qmin: torch.Tensor
    dist: Optional[torch.Tensor]
    window: CellWindow
    heading: Optional[torch.Tensor]
    r2_cap: int
    metric: str = "euclid"
    dt: float = 0.1
    margin: float = 0.0
    cell_size: float = 0.5
    from_memory: bool = False
    from_vehicle_memory: bool = False      # ... and that set was its vehicle layer V, not H (flow="lanes" only)
    flow: str = "any"

    NONE = 2 ** 31 - 1
    SLACK_NONE = 2 ** 31 - 1

    def reach(self, v_max):
        """``(hit [M, T] bool, first [M] int32, slack [M] int32)`` for a hidden road user of up to ``v_max`` m/s: ``hit`` is
        ``cells > 0`` of ``hidden_reach(v_max=v_max)`` with the same metric, flow, margin and ``dt``, ``first`` and ``slack`` are its
        ``first`` and ``slack``, exactly.  Torch ops on the tensors' device, nothing is read back.  ValueError when the table
        of ``v_max`` ends beyond ``r2_cap``."""
        M, T = (int(v) for v in self.qmin.shape)
        v_max = float(v_max)
        if not v_max >= 0.0:
            raise ValueError("reach: v_max >= 0")
        r2 = hidden_reach_r2(v_max, self.dt, self.margin, self.cell_size, T)
        if T and int(r2[-1]) > int(self.r2_cap):
            raise ValueError(f"reach: the table of v_max = {v_max} m/s ends at R2 = {int(r2[-1])}, beyond r2_cap = {int(self.r2_cap)} "
                             "(ask hidden_clearance for a larger v_cap)")
        dev = self.qmin.device
        thr = torch.as_tensor(169 * r2.astype(np.int64), device=dev)            # non-decreasing, < 2^31
        q = self.qmin.to(torch.int64)
        k = torch.arange(T, device=dev, dtype=torch.int64)
        hit = q <= thr[None, :]
        first = torch.where(hit, k[None, :], T).amin(dim=1, keepdim=False) if T else torch.zeros(M, dtype=torch.int64, device=dev)
        first = torch.where(first >= T, -1, first).to(torch.int32)
        j = torch.searchsorted(thr, q.contiguous())                             # min { j : q <= 169 R2[j] }, T = none
        slack = torch.where(j < T, j - k[None, :], self.SLACK_NONE)
        slack = (slack.amin(dim=1) if T else torch.full((M,), self.SLACK_NONE, dtype=torch.int64, device=dev)).to(torch.int32)
        return hit, first, slack

    def critical_speed(self):
        """``v_crit [M]`` float64 (m/s): the slowest hidden road user that could meet the trajectory at all, ``+inf`` where nothing
        lies within the cap.  Per sample, with ``r = sqrt(qmin / 169) cs``: at ``k = 0`` the value is 0 if
        ``qmin <= 169 floor(margin^2 / cs^2)`` and ``+inf`` otherwise, at ``k >= 1`` it is ``max(0, r - margin) / (k dt)``;
        ``v_crit`` is the minimum over the samples.

        "euclid": exact -- ``D2 <= floor(X)`` iff ``D2 <= X``, so ``reach(v_crit (1 + 1e-9))`` hits and
        ``reach(v_crit (1 - 1e-9))`` does not (up to the rounding of this float64 formula, around 1e-15 relative).
        "road": the floor under ``169 R2`` makes it a LOWER bound -- no ``v_max < v_crit`` produces a hit, the smallest ``v_max``
        that does may be larger: the conservative side."""
        M, T = (int(v) for v in self.qmin.shape)
        dev = self.qmin.device
        inf = float("inf")
        if T == 0:
            return torch.full((M,), inf, dtype=torch.float64, device=dev)
        q = self.qmin.to(torch.int64)
        none = q == self.NONE
        r = torch.sqrt(q.to(torch.float64) / 169.0) * self.cell_size
        k = torch.arange(T, device=dev, dtype=torch.float64)
        kdt = k * self.dt
        kdt[0] = 1.0                                                             # (column 0 is replaced below)
        v = torch.clamp(r - self.margin, min=0.0) / kdt[None, :]
        r2_0 = int(hidden_reach_r2(0.0, self.dt, self.margin, self.cell_size, 1)[0])
        v[:, 0] = torch.where(q[:, 0] <= 169 * r2_0, 0.0, inf)
        v = torch.where(none, inf, v)
        return v.amin(dim=1)


def _prepare(self, entry, v_name, *, x, y, theta, vehicle, v, dt, margin, inflate, lengths, metric, flow="any", heading=None):
    """What ``hidden_reach`` and ``hidden_clearance`` (``entry``; ``v_name``: its name for the speed ``v``) do before they differ: the
    refusals in their one order (before the last one only ``window`` and ``cell_size`` of the model are read), the device inputs,
    the reach table of ``v``, this step's hidden set (None: the reset definition) and the ``fields`` both argument structures share."""
    if metric not in HIDDEN_REACH_METRICS:
        raise ValueError(f"{entry}: metric {metric!r}, one of {HIDDEN_REACH_METRICS} is possible")
    if flow not in HIDDEN_REACH_FLOWS:
        raise ValueError(f"{entry}: flow {flow!r}, one of {HIDDEN_REACH_FLOWS} is possible")
    if flow == "lanes" and metric != "road":
        raise ValueError(f"{entry}: flow 'lanes' follows the lanes along the road: it needs metric 'road', not {metric!r}")
    if self.window is None:
        raise RuntimeError(f"{entry} needs the cell classes of a previous launch()")
    length, width, wb = (float(a) for a in tuple(vehicle)[:3])
    v, dt, inflate = float(v), float(dt), float(inflate)
    margin = math.sqrt(2.0) * self.cell_size if margin is None else float(margin)
    if not (v >= 0.0 and margin >= 0.0 and dt > 0.0):
        raise ValueError(f"{entry}: {v_name} >= 0, margin >= 0 and dt > 0")
    hl, hw = 0.5 * length + inflate, 0.5 * width + inflate
    ext = N.HIDDEN_REACH_MAX_HALF_EXTENT * self.cell_size
    if not (0.0 <= hl <= ext and 0.0 <= hw <= ext and abs(wb) <= ext):
        raise ValueError(f"{entry}: the inflated half extents and |wb_rear_axle| must lie in [0, {ext} m]")
    M, T = (int(a) for a in x.shape)
    if tuple(y.shape) != (M, T) or (heading is None and (theta is None or tuple(theta.shape) != (M, T))):
        raise ValueError(f"{entry}: x, y and theta must be [M, T]")
    if heading is not None and tuple(heading.shape) != (M, T, 2):
        raise ValueError(f"{entry}: heading must be [M, T, 2]")
    if not 1 <= T <= N.HIDDEN_REACH_MAX_J:
        raise ValueError(f"{entry}: {T} samples per trajectory, 1 .. {N.HIDDEN_REACH_MAX_J} are possible")
    r2 = hidden_reach_r2(v, dt, margin, self.cell_size, T)
    if int(r2[-1]) >= (N.HIDDEN_REACH_MAX_HALO + 1) ** 2:
        raise ValueError(f"{entry}: a reach of {math.isqrt(int(r2[-1]))} cells at the end of the horizon, at most "
                         f"{N.HIDDEN_REACH_MAX_HALO} are possible (shorter horizon, lower {v_name} or larger cells)")
    if lengths is not None and tuple(np.shape(lengths)) != (M,):
        raise ValueError(f"{entry}: lengths must be [M]")
    if flow == "lanes" and getattr(self, "lane_moves", None) is None:
        raise RuntimeError(f"{entry}: flow 'lanes' needs the map's move table, and this model has none (it was built without lanelets)")
    dev = self.device
    tx, ty = N.on_device(x, dev), N.on_device(y, dev)
    heading = N.on_device(unit_headings(theta) if heading is None else heading, dev)
    tlen = None if lengths is None else N.on_device(lengths, dev, "int32")
    w = self.window
    # lane-abiding vehicles start from the occlusion memory's vehicle layer when it ran in this step's stage, every other
    # question from H, as before (flow="any" never reads V)
    vehicles = self._om.hidden_vehicles_on_device(w) if flow == "lanes" else None
    hidden = vehicles if vehicles is not None else self._om.hidden_on_device(w)
    fields = dict(M=M, T=T, d_x=N.ptr(tx), d_y=N.ptr(ty), d_heading=N.ptr(heading), d_len_or_null=N.ptr(tlen), hl=hl, hw=hw, wb=wb,
                  d_cls=self.cell_class.data_ptr(), d_hidden_or_null=N.ptr(hidden), win_ix0=w.ix0, win_iy0=w.iy0, win_nx=w.nx,
                  win_ny=w.ny)
    return SimpleNamespace(M=M, T=T, dt=dt, margin=margin, r2=r2, x=tx, y=ty, heading=heading, lengths=tlen, hidden=hidden, fields=fields,
                           from_vehicles=vehicles is not None)


def hidden_reach(self, x, y, theta, *, vehicle, v_max, dt, margin=None, inflate=0.0, lengths=None, metric="euclid", flow="any"):
    """Hidden-traffic reach forecast (``fo_scene_hidden_reach``, with ``metric="road"`` ``fo_scene_hidden_reach_road``:
    hidden traffic arrives along the road, not through what is not road; with ``flow="lanes"`` on top of it
    ``fo_scene_hidden_reach_flow``: hidden VEHICLES follow the driving direction of the lanes -- pedestrians do not, they keep
    ``flow="any"``); returns a :class:`HiddenReach`.  The kernels are queued
    on the current stream and nobody waits for them; ``theta`` is turned into (cos, sin) on the HOST (:func:`unit_headings`:
    the device takes no sine or cosine), so a ``theta`` that lives on the device is first copied back, which waits for the
    stream -- hand ``theta`` over as a host array, as a planner's trajectory objects give it, to avoid that.

    ``x, y, theta [M, T]``: candidate trajectories, sample k at ``k dt`` from now (M = 0: the arrival map alone).
    ``vehicle``: (length, width, wb_rear_axle) of the ego rectangle, ``inflate`` (m) is added to both half extents.
    A road user hidden now -- in the occlusion memory's hidden set when the memory ran this step, else anywhere on
    road that is not visible -- moves at up to ``v_max`` (m/s); ``margin`` (m, None = sqrt(2) cell sizes) as for the
    memory.  ``lengths [M]``: samples ``k >= lengths[m]`` of a ragged batch contribute nothing."""
    q = _prepare(self, "hidden_reach", "v_max", x=x, y=y, theta=theta, vehicle=vehicle, v=v_max, dt=dt, margin=margin, inflate=inflate,
                 lengths=lengths, metric=metric, flow=flow)
    dev, w, r2 = self.device, self.window, q.r2
    arrival = torch.empty((w.ny, w.nx), dtype=torch.uint8, device=dev)
    cells = torch.empty((q.M, q.T), dtype=torch.int32, device=dev)
    first = torch.empty(q.M, dtype=torch.int32, device=dev)
    slack = torch.empty(q.M, dtype=torch.int32, device=dev)
    args = N.HiddenReach(J=q.T, h_r2=r2.ctypes.data_as(C.POINTER(C.c_int32)), d_arrival=arrival.data_ptr(), d_cells=N.ptr(cells),
                         d_first=N.ptr(first), d_slack=N.ptr(slack), **q.fields)
    dist = torch.empty((w.ny, w.nx), dtype=torch.uint16, device=dev) if metric == "road" else None
    if dist is not None:
        args = N.HiddenReachRoad(base=args, d_dist_or_null=dist.data_ptr())
    entry = "fo_scene_hidden_reach" if dist is None else "fo_scene_hidden_reach_flow" if flow == "lanes" else "fo_scene_hidden_reach_road"
    self.ctx.call(entry, C.byref(args), N.current_stream(self._dev_index))
    self._hr_inputs = (q.x, q.y, q.heading, q.lengths)      # (stay referenced until the next call, as in future_visibility_ex)
    return HiddenReach(arrival, cells, first, slack, r2, w, q.heading, q.hidden is not None, q.from_vehicles, metric,
                       hidden_reach_road_units(r2), dist, flow)


def hidden_clearance(self, x, y, theta, *, vehicle, v_cap, dt, margin=None, inflate=0.0, lengths=None, metric="euclid",
                     heading=None, flow="any"):
    """Hidden-traffic clearance (``fo_scene_hidden_clearance``; DESIGN.md §5.10 "Clearance and critical speed"): ONE key
    map and one minimum per pose that answer :meth:`hidden_reach` for every ``v_max <= v_cap``
    (:meth:`HiddenClearance.reach`) and give the slowest hidden road user that could meet each trajectory
    (:meth:`HiddenClearance.critical_speed`); returns a :class:`HiddenClearance`.  Arguments as for :meth:`hidden_reach`;
    ``r2_cap`` is the last entry of the reach table of ``v_cap``.  ``heading``: the ``[M, T, 2]`` (cos, sin) tensor of an
    earlier :class:`HiddenReach` / :class:`HiddenClearance` of the SAME candidates -- the host-side ``unit_headings`` pass
    over ``theta`` is then skipped (``theta`` may be None).  The number of reached footprint cells (``cells`` of
    ``hidden_reach``) is not derivable from the result, only whether it is positive.  ``flow="lanes"`` (with ``metric="road"``):
    ``fo_scene_hidden_clearance_flow``, the key map of the lane flow."""
    q = _prepare(self, "hidden_clearance", "v_cap", x=x, y=y, theta=theta, vehicle=vehicle, v=v_cap, dt=dt, margin=margin, inflate=inflate,
                 lengths=lengths, metric=metric, flow=flow, heading=heading)
    dev, w, r2_cap = self.device, self.window, int(q.r2[-1])
    key = torch.empty((w.ny, w.nx), dtype=torch.int32, device=dev)
    qmin = torch.empty((q.M, q.T), dtype=torch.int32, device=dev)
    dist = torch.empty((w.ny, w.nx), dtype=torch.uint16, device=dev) if metric == "road" else None
    args = N.HiddenClearance(r2_cap=r2_cap, metric=N.HIDDEN_CLEARANCE_METRIC[metric], d_key=key.data_ptr(), d_qmin=N.ptr(qmin),
                             d_dist_or_null=N.ptr(dist), **q.fields)
    self.ctx.call("fo_scene_hidden_clearance_flow" if flow == "lanes" else "fo_scene_hidden_clearance", C.byref(args),
                  N.current_stream(self._dev_index))
    self._hc_inputs = (q.x, q.y, q.heading, q.lengths)      # (stay referenced until the next call, as in hidden_reach)
    return HiddenClearance(key, qmin, dist, w, q.heading, r2_cap, metric, q.dt, q.margin, self.cell_size, q.hidden is not None,
                           q.from_vehicles, flow)


# step k of the lattice points at k * 45 degrees: E, NE, N, NW, W, SW, S, SE (DESIGN.md §5.10 "Lane flow")
WITNESS_DIRS = np.array([(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)], dtype=np.int64)


def witness_path_cap(r2):
    """the shortest row of ``dirs`` that holds every walk of a forecast with the reach table ``r2``: ``isqrt(169 R2[J-1]) // 12``
    steps, rounded up to a multiple of 4 (at most ``_native.HIDDEN_WITNESS_MAX_STEPS`` at the halo cap)"""
    return (math.isqrt(169 * int(r2[-1])) // 12 + 3) // 4 * 4


@dataclass
class HiddenWitness:
    """what :meth:`SensorModel.hidden_witness` returns (DESIGN.md §5.10 "Witnesses"): ``reach`` is the :class:`HiddenReach` of the
    road / lane-flow forecast the witnesses belong to (``k* = reach.first``), and per candidate trajectory m (device tensors)
    ``cell [M, 2]`` int32 -- world-raster indices (gx, gy) of the conflict cell g*, the footprint cell of sample k* that hidden
    traffic reaches along the shortest road distance; ``source [M, 2]`` int32 -- the hidden cell that traffic starts from;
    ``steps [M]`` int32 -- lattice steps between them, -1 = the trajectory meets no hidden traffic (``cell`` and ``source`` then
    hold INT32_MIN), -2 = the maps are not a forecast's (never after :meth:`SensorModel.hidden_witness`); ``dist [M]`` int32 --
    the road distance ``d(g*)`` (12 per axis step, 17 per diagonal one), -1 = none; ``dirs [M, path_cap]`` uint8 -- the steps in
    walk order (from g* back to the source), 255 beyond ``steps``.  ``origin`` (x0, y0) and ``cell_size`` place the raster in the
    world, ``dt`` and ``v_max`` are the forecast's.

    The witness is the road user that is FIRST by road distance, not the most harmful one.  :meth:`routes`, :meth:`speed` and
    :meth:`select` read the tensors back once (the first call waits for the stream)."""
    reach: HiddenReach
    cell: torch.Tensor
    source: torch.Tensor
    steps: torch.Tensor
    dist: torch.Tensor
    dirs: torch.Tensor
    origin: tuple
    cell_size: float
    dt: float
    v_max: float
    path_cap: int

    def _host(self):
        h = self.__dict__.get("_host_copy")
        if h is None:
            h = SimpleNamespace(**{n: getattr(self, n).detach().cpu().numpy() for n in ("cell", "source", "steps", "dist", "dirs")},
                                first=self.reach.first.detach().cpu().numpy())
            self.__dict__["_host_copy"] = h
        return h

    def routes(self, indices):
        """per trajectory index a float64 ``[steps + 1, 2]`` polyline of cell centres (world coordinates) in TRAVEL order: the
        source first, the conflict cell last; ``None`` where ``steps < 0``"""
        h, out = self._host(), []
        for m in indices:
            n = int(h.steps[m])
            if n < 0:
                out.append(None)
                continue
            moves = WITNESS_DIRS[h.dirs[m, :n][::-1].astype(np.int64)]           # travel order: dir_{k_{n-1}}, .., dir_{k_0}
            cells = h.source[m].astype(np.int64)[None] + np.concatenate((np.zeros((1, 2), dtype=np.int64), np.cumsum(moves, axis=0)))
            out.append(np.asarray(self.origin, dtype=np.float64)[None] + (cells.astype(np.float64) + 0.5) * self.cell_size)
        return out

    def length(self, m):
        """length (m) of the route of trajectory m: ``cell_size`` per axis step, ``cell_size sqrt(2)`` per diagonal one"""
        h = self._host()
        n = max(int(h.steps[m]), 0)
        diag = int((h.dirs[m, :n] & 1).sum())
        return self.cell_size * ((n - diag) + diag * math.sqrt(2.0))

    def speed(self, m):
        """the speed (m/s) at which the witness of trajectory m is at the conflict cell exactly at sample k*: the route length
        divided by ``k* dt``; 0.0 when ``k* = 0`` (it is there now) and without a witness.

        Bound: ``speed <= 13/12 (v_max + margin / (k* dt))``.  A lattice path of road distance d has a length between ``d / 13``
        and ``d / 12`` cells (an axis step: 12 units for 1 cell; a diagonal one: 17 units for sqrt(2) cells, 17 / sqrt(2) > 12,
        and 12 dx + 5 dy <= 13 sqrt(dx^2 + dy^2)), and ``d(g*) <= L[k*] = isqrt(169 R2[k*]) <= 13 (v_max k* dt + margin) / cs``,
        so the length is at most ``13/12 (v_max k* dt + margin)``.  The speed can therefore exceed ``v_max``: the forecast's
        reach carries the margin, and the lattice measures an octagon, not a circle."""
        h = self._host()
        k = int(h.first[m])
        if k <= 0 or int(h.steps[m]) < 0:
            return 0.0
        return self.length(m) / (k * self.dt)

    def select(self, max_agents=8, merge_cells=4):
        """trajectory indices whose witnesses are worth an agent each: one per block of ``merge_cells`` x ``merge_cells`` source
        cells (``source // merge_cells``), within a block the smallest ``(k*, dist, m)``, the blocks ordered by that key, at most
        ``max_agents``"""
        h = self._host()
        merge = max(int(merge_cells), 1)
        best = {}
        for m in np.nonzero(h.steps >= 0)[0]:
            key = (int(h.first[m]), int(h.dist[m]), int(m))
            block = (int(h.source[m, 0]) // merge, int(h.source[m, 1]) // merge)
            if block not in best or key < best[block]:
                best[block] = key
        return [key[2] for key in sorted(best.values())[:max(int(max_agents), 0)]]


def hidden_witness(self, x, y, theta, *, vehicle, v_max, dt, margin=None, inflate=0.0, lengths=None, flow="any"):
    """Hidden-traffic witnesses (``fo_scene_hidden_witness``; DESIGN.md §5.10 "Witnesses"): runs
    ``hidden_reach(..., metric="road", flow=flow)`` and, on the very same device inputs, one more launch that gives per
    candidate the cell where hidden traffic first meets it, the hidden cell that traffic starts from and the cheapest route
    between them; returns a :class:`HiddenWitness`.  Arguments as for :meth:`hidden_reach`; the Euclidean metric has no route
    and is not offered.  Nothing is read back and nobody waits for the kernels."""
    reach = hidden_reach(self, x, y, theta, vehicle=vehicle, v_max=v_max, dt=dt, margin=margin, inflate=inflate, lengths=lengths,
                         metric="road", flow=flow)
    tx, ty, heading, tlen = self._hr_inputs
    M, T = (int(a) for a in tx.shape)
    dev, w = self.device, reach.window
    cap = witness_path_cap(reach.r2)
    cell = torch.empty((M, 2), dtype=torch.int32, device=dev)
    source = torch.empty((M, 2), dtype=torch.int32, device=dev)
    steps = torch.empty(M, dtype=torch.int32, device=dev)
    dist = torch.empty(M, dtype=torch.int32, device=dev)
    dirs = torch.empty((M, cap), dtype=torch.uint8, device=dev)
    length, width, wb = (float(a) for a in tuple(vehicle)[:3])
    inflate = float(inflate)
    base = N.HiddenReach(M=M, T=T, d_x=N.ptr(tx), d_y=N.ptr(ty), d_heading=N.ptr(heading), d_len_or_null=N.ptr(tlen),
                         hl=0.5 * length + inflate, hw=0.5 * width + inflate, wb=wb, J=T,
                         h_r2=reach.r2.ctypes.data_as(C.POINTER(C.c_int32)), win_ix0=w.ix0, win_iy0=w.iy0, win_nx=w.nx, win_ny=w.ny,
                         d_arrival=reach.arrival.data_ptr(), d_first=N.ptr(reach.first))
    args = N.HiddenWitness(base=base, d_dist=reach.road_dist.data_ptr(), flow=int(flow == "lanes"), path_cap=cap, d_cell=N.ptr(cell),
                           d_src=N.ptr(source), d_steps=N.ptr(steps), d_wdist=N.ptr(dist), d_dirs=N.ptr(dirs))
    self.ctx.call("fo_scene_hidden_witness", C.byref(args), N.current_stream(self._dev_index))
    return HiddenWitness(reach, cell, source, steps, dist, dirs, tuple(float(v) for v in self.raster_origin), self.cell_size,
                         float(dt), float(v_max), cap)


def travelled_arc(x, y):
    """the travelled chord length of trajectories ``x, y [M, T]`` -- be.py's ``insert(cumsum(sqrt(diff(x)^2 + diff(y)^2)), 0, 0)``
    per row, float64 ``[M, T]``.  Host arrays: that numpy formula.  Device tensors: the same with torch on the tensors' device,
    nothing is copied back.  The brake clearance takes the result as DATA (as it takes the headings): whichever form made it, the
    very numbers are kept in the :class:`HiddenBrake` and are what a checker is handed."""
    if torch.is_tensor(x) or torch.is_tensor(y):
        tx = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64), device=y.device)
        ty = y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y, dtype=np.float64), device=tx.device)
        tx, ty = tx.to(torch.float64), ty.to(torch.float64)
        seg = torch.sqrt(torch.diff(tx, dim=-1) ** 2 + torch.diff(ty, dim=-1) ** 2)
        return torch.cat((torch.zeros_like(tx[..., :1]), torch.cumsum(seg, dim=-1)), dim=-1)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    seg = np.sqrt(np.diff(x, axis=-1) ** 2 + np.diff(y, axis=-1) ** 2)
    return np.insert(np.cumsum(seg, axis=-1), 0, 0.0, axis=-1)


def _device_arc(x, y, dev):
    """:func:`travelled_arc` of a brake entry's candidates on ``dev``: made where ``x`` and ``y`` both live, host arrays' uploaded"""
    arc = travelled_arc(x, y) if torch.is_tensor(x) and torch.is_tensor(y) else travelled_arc(np.asarray(x), np.asarray(y))
    return N.on_device(arc, dev)


def _a_brake(a_brake, fn):
    """the deceleration of ``fn``'s manoeuvre as a float, or its refusal"""
    a_brake = float(a_brake)
    if not (a_brake >= 0.0 and math.isfinite(a_brake)):
        raise ValueError(f"{fn}: a_brake >= 0 and finite")
    return a_brake


def _decided_until(stop, lengths):
    """``decided_until`` of :class:`HiddenBrake` and :class:`HiddenBrakeClasses`: ``stop [M, T]`` does not depend on the hidden road
    user"""
    M, T = (int(v) for v in stop.shape)
    dev = stop.device
    Lm = torch.full((M,), T, dtype=torch.int64, device=dev)
    if lengths is not None:
        Lm = torch.clamp(lengths.to(torch.int64), 0, T)
    if T == 0:
        return Lm.to(torch.int32)
    b = torch.arange(T, device=dev, dtype=torch.int64)[None, :]
    open_end = (stop.to(torch.int64) == Lm[:, None]) & (b < Lm[:, None])
    return torch.where(open_end, b, Lm[:, None]).amin(dim=1).to(torch.int32)


@dataclass
class HiddenBrake:
    """what :meth:`SensorModel.hidden_brake` returns (DESIGN.md §5.10 "Brake clearance"): ``reach`` is the :class:`HiddenReach` of
    the forecast the manoeuvres were held against, and (device tensors, int32) ``brake_first [M, T]`` -- for "follow candidate m
    until sample b, then brake at ``a_brake``" the first sample ``i > b`` at which the braking ego's footprint holds a cell hidden
    traffic may have reached by then, -1 = none within the horizon (and for ``b >= lengths[m]``); ``stop [M, T]`` -- the first
    sample at which that manoeuvre stands, ``Lm`` = not within the horizon, -1 for ``b >= lengths[m]``; ``commit [M]`` -- the
    smallest b from which the candidate is no longer fail-safe: ``reach.first <= b`` (it is in reached road itself) or
    ``brake_first < stop`` (the braking ego meets reached road while it still moves), -1 = fail-safe from every sample of the
    horizon.  A LARGER ``commit`` is the safer candidate, -1 the safest.  ``arc [M, T]`` float64 is the travelled chord length the
    device was handed (:func:`travelled_arc`), ``a_brake`` (m/s^2) and ``dt`` the manoeuvre's, ``lengths [M]`` int32 the ragged
    batch's lengths on the device (None: every trajectory has T samples).

    Not claimed: the manoeuvre keeps to the candidate's own path and ends where it ends; one that still moves at the last sample
    is decided within the horizon only (:meth:`decided_until`); the heading is the nearer sample's; the hidden road user is the
    forecast's."""
    reach: HiddenReach
    brake_first: torch.Tensor
    stop: torch.Tensor
    commit: torch.Tensor
    arc: torch.Tensor
    a_brake: float
    dt: float
    lengths: Optional[torch.Tensor] = None

    def decided_until(self):
        """``[M]`` int32: the smallest brake start b with ``stop[m, b] == Lm`` -- from there on the horizon no longer sees the
        braking ego stand, so ``commit`` speaks only of the samples it has -- and ``Lm`` where every manoeuvre stands in time.
        Torch ops on the tensors' device, nothing is read back."""
        return _decided_until(self.stop, self.lengths)


def hidden_brake(self, x, y, theta, v, *, vehicle, v_max, dt, a_brake, margin=None, inflate=0.0, lengths=None, metric="euclid",
                 flow="any"):
    """Hidden-traffic brake clearance (``fo_scene_hidden_brake``; DESIGN.md §5.10 "Brake clearance"): runs
    ``hidden_reach(...)`` with these arguments and, on the very same device inputs, one more launch that holds the manoeuvre
    "follow the candidate until sample b, then brake at ``a_brake``" of every (candidate, b) against the forecast's arrival map;
    returns a :class:`HiddenBrake`.  ``v [M, T]``: the candidates' speed at each sample (m/s); the travelled chord length is
    :func:`travelled_arc` of ``x, y``.  The other arguments as for :meth:`hidden_reach`.  Nothing is read back and nobody waits
    for the kernels."""
    reach = hidden_reach(self, x, y, theta, vehicle=vehicle, v_max=v_max, dt=dt, margin=margin, inflate=inflate, lengths=lengths,
                         metric=metric, flow=flow)
    tx, ty, heading, tlen = self._hr_inputs
    M, T = (int(a) for a in tx.shape)
    if tuple(v.shape) != (M, T):
        raise ValueError("hidden_brake: v must be [M, T]")
    a_brake = _a_brake(a_brake, "hidden_brake")
    dev, w = self.device, reach.window
    tv = N.on_device(v, dev)
    arc = _device_arc(x, y, dev)
    brake_first = torch.empty((M, T), dtype=torch.int32, device=dev)
    stop = torch.empty((M, T), dtype=torch.int32, device=dev)
    commit = torch.empty(M, dtype=torch.int32, device=dev)
    length, width, wb = (float(a) for a in tuple(vehicle)[:3])
    inflate = float(inflate)
    base = N.HiddenReach(M=M, T=T, d_x=N.ptr(tx), d_y=N.ptr(ty), d_heading=N.ptr(heading), d_len_or_null=N.ptr(tlen),
                         hl=0.5 * length + inflate, hw=0.5 * width + inflate, wb=wb, J=T,
                         h_r2=reach.r2.ctypes.data_as(C.POINTER(C.c_int32)), win_ix0=w.ix0, win_iy0=w.iy0, win_nx=w.nx, win_ny=w.ny,
                         d_arrival=reach.arrival.data_ptr(), d_first=N.ptr(reach.first))
    args = N.HiddenBrake(base=base, d_v=N.ptr(tv), d_arc=N.ptr(arc), a_brake=a_brake, dt=float(dt), d_brake_first=N.ptr(brake_first),
                         d_stop=N.ptr(stop), d_commit=N.ptr(commit))
    self.ctx.call("fo_scene_hidden_brake", C.byref(args), N.current_stream(self._dev_index))
    self._hb_inputs = (tv, arc)                             # (stay referenced until the next call, as in hidden_reach)
    return HiddenBrake(reach, brake_first, stop, commit, arc, a_brake, float(dt), tlen)


def reference_deceleration_ladder(lo, hi):
    """the deceleration vector the reference's manoeuvre routine makes of ``deceleration=[lo, hi]``: ``np.arange(lo, hi, 0.1)``
    (metrics/be.py:106-107), float64 -- ``hi`` itself is not on it, and its entries are arange's ``lo + n * 0.1``, not decimals"""
    return np.arange(lo, hi, 0.1)


@dataclass
class HiddenBrakeLadder:
    """what :meth:`SensorModel.hidden_brake_ladder` returns (DESIGN.md §5.10 "Brake ladder"): ``reach`` is the :class:`HiddenReach` of
    the forecast the manoeuvres were held against, ``decelerations`` (host float64 ``[K]``, strictly ascending) the ladder, and (device
    tensors, int32) ``brake_first [M, B, K]`` and ``stop [M, B, K]`` -- slice k is, bit for bit, ``brake_first`` / ``stop`` of
    ``hidden_brake(a_brake=decelerations[k])`` at the brake starts ``b < B`` --, ``commit [M, K]`` -- that call's ``commit`` where it
    is ``< B``, else -1 --, ``required [M, B]`` -- the first level at which "follow candidate m until sample b, then brake" stays
    clear of hidden traffic while it moves, -1 = no level of the ladder does --, ``last_unclear [M, B]`` -- the last level at which
    it does not, -1 = every level is clear.  Both are -1 where there is no manoeuvre (``b >= lengths[m]``).  ``arc``, ``dt``,
    ``lengths`` as in :class:`HiddenBrake`.

    Not claimed: what :class:`HiddenBrake` does not claim; the answer is only as fine as the ladder; ``required`` is the first clear
    level, not a root -- harder braking is not always safer against an arrival map (:meth:`monotone`)."""
    reach: HiddenReach
    brake_first: torch.Tensor
    stop: torch.Tensor
    commit: torch.Tensor
    required: torch.Tensor
    last_unclear: torch.Tensor
    decelerations: np.ndarray
    arc: torch.Tensor
    dt: float
    lengths: Optional[torch.Tensor] = None

    def level(self, k):
        """``(brake_first [M, B], stop [M, B], commit [M])`` of level k: what ``hidden_brake(a_brake=decelerations[k])`` gives at the
        brake starts ``b < B`` (views, nothing is copied)"""
        return self.brake_first[:, :, k], self.stop[:, :, k], self.commit[:, k]

    def required_deceleration(self):
        """``[M, B]`` float64 (m/s^2): ``decelerations[required]``; ``+inf`` where a manoeuvre exists and no level of the ladder is
        clear; ``nan`` where there is no manoeuvre (``required == last_unclear == -1``).  Torch ops on the tensors' device, nothing
        is read back."""
        dev = self.required.device
        levels = torch.as_tensor(np.append(np.asarray(self.decelerations, dtype=np.float64), np.inf), device=dev)
        req = self.required.to(torch.int64)
        out = levels[torch.where(req >= 0, req, len(levels) - 1)]
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        return torch.where((req < 0) & (self.last_unclear < 0), nan, out)

    def brake_threat_number(self, a_max):
        """``[M, B]`` float64: :meth:`required_deceleration` divided by ``a_max`` -- the reference's ``break_threat_number``
        (metrics/be.py:56) against hidden traffic"""
        return self.required_deceleration() / float(a_max)

    def monotone(self):
        """``[M, B]`` bool: ``required == last_unclear + 1`` or ``required == -1`` -- below the first clear level everything is
        unclear and from it on everything is clear: where the reference's bisection would have been sound"""
        return (self.required == self.last_unclear + 1) | (self.required == -1)


def _ladder_levels(decelerations, fn):
    """the ladder of ``fn`` (hidden_brake_ladder and its sibling by road users) as float64 ``[L]``, or its refusal"""
    levels = np.zeros(0)                                   # (what is no 1-D sequence of numbers is refused as an empty ladder is)
    if not isinstance(decelerations, (str, bytes)) and np.ndim(decelerations) == 1:
        try:
            levels = np.array([float(a) for a in decelerations], dtype=np.float64)
        except (TypeError, ValueError):
            pass
    if not 1 <= len(levels) <= N.HIDDEN_BRAKE_MAX_LEVELS or not (np.isfinite(levels) & (levels >= 0.0)).all():
        raise ValueError(f"{fn}: decelerations must hold 1 .. {N.HIDDEN_BRAKE_MAX_LEVELS} finite values >= 0")
    if not (np.diff(levels) > 0.0).all():
        raise ValueError(f"{fn}: decelerations must be strictly ascending (required is then the gentlest clear one)")
    return levels


def default_brake_ladder(a_max, fn):
    """the default ladder of ``fn`` (hidden_brake_ladder and hidden_brake_ladder_users): 0.5, 1.0, ... up to ``a_max``, with ``a_max``
    itself appended if it is not on that grid"""
    a_max = float(a_max)
    n = int(a_max // 0.5) if 0.5 <= a_max < float("inf") else 0      # levels on the 0.5 grid
    on_grid = n > 0 and 0.5 * n == a_max
    if n + (not on_grid) > N.HIDDEN_BRAKE_MAX_LEVELS:
        raise ValueError(f"{fn}: the default ladder 0.5, 1.0, ... up to a_max = {a_max} m/s^2 has more than "
                         f"{N.HIDDEN_BRAKE_MAX_LEVELS} levels (hand decelerations over)")
    return [0.5 * (k + 1) for k in range(n)] + ([] if on_grid else [a_max])


def _ladder_starts(starts, T, fn):
    """the number of brake starts of ``fn``: ``starts``, an integer in ``[1, T]``, None = T"""
    if starts is None:
        starts = T
    if isinstance(starts, bool) or not isinstance(starts, (int, np.integer)) or not 1 <= int(starts) <= T:
        raise ValueError(f"{fn}: starts = {starts!r}, an integer in [1, T = {T}] or None")
    return int(starts)


def hidden_brake_ladder(self, x, y, theta, v, *, vehicle, v_max, dt, decelerations, starts=None, margin=None, inflate=0.0, lengths=None,
                        metric="euclid", flow="any"):
    """Hidden-traffic brake ladder (``fo_scene_hidden_brake_ladder``; DESIGN.md §5.10 "Brake ladder"): runs ``hidden_reach(...)``
    with these arguments and, on the very same device inputs, ONE more launch that holds the manoeuvre "follow the candidate until
    sample b, then brake" of every (candidate, b) against the forecast's arrival map at every deceleration of ``decelerations``
    (1 .. 64 finite values >= 0, strictly ascending, m/s^2) for the brake starts ``b < starts`` (an integer in ``[1, T]``, None =
    T); returns a :class:`HiddenBrakeLadder`, whose ``required`` is the gentlest deceleration of the ladder that keeps the moving ego
    clear.  The other arguments as for :meth:`hidden_brake`.  Nothing is read back and nobody waits for the kernels."""
    reach = hidden_reach(self, x, y, theta, vehicle=vehicle, v_max=v_max, dt=dt, margin=margin, inflate=inflate, lengths=lengths,
                         metric=metric, flow=flow)
    tx, ty, heading, tlen = self._hr_inputs
    M, T = (int(a) for a in tx.shape)
    if tuple(v.shape) != (M, T):
        raise ValueError("hidden_brake_ladder: v must be [M, T]")
    levels = _ladder_levels(decelerations, "hidden_brake_ladder")
    B, K = _ladder_starts(starts, T, "hidden_brake_ladder"), len(levels)
    dev, w = self.device, reach.window
    tv = N.on_device(v, dev)
    arc = _device_arc(x, y, dev)
    brake_first = torch.empty((M, B, K), dtype=torch.int32, device=dev)
    stop = torch.empty((M, B, K), dtype=torch.int32, device=dev)
    required = torch.empty((M, B), dtype=torch.int32, device=dev)
    last_unclear = torch.empty((M, B), dtype=torch.int32, device=dev)
    commit = torch.empty((M, K), dtype=torch.int32, device=dev)
    length, width, wb = (float(a) for a in tuple(vehicle)[:3])
    inflate = float(inflate)
    base = N.HiddenReach(M=M, T=T, d_x=N.ptr(tx), d_y=N.ptr(ty), d_heading=N.ptr(heading), d_len_or_null=N.ptr(tlen),
                         hl=0.5 * length + inflate, hw=0.5 * width + inflate, wb=wb, J=T,
                         h_r2=reach.r2.ctypes.data_as(C.POINTER(C.c_int32)), win_ix0=w.ix0, win_iy0=w.iy0, win_nx=w.nx, win_ny=w.ny,
                         d_arrival=reach.arrival.data_ptr(), d_first=N.ptr(reach.first))
    args = N.HiddenBrakeLadder(base=base, d_v=N.ptr(tv), d_arc=N.ptr(arc), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), K=K, B=B,
                               dt=float(dt), d_brake_first=N.ptr(brake_first), d_stop=N.ptr(stop), d_required=N.ptr(required),
                               d_last_unclear=N.ptr(last_unclear), d_commit=N.ptr(commit))
    self.ctx.call("fo_scene_hidden_brake_ladder", C.byref(args), N.current_stream(self._dev_index))
    self._hbl_inputs = (tv, arc)                            # (stay referenced until the next call, as in hidden_brake)
    return HiddenBrakeLadder(reach, brake_first, stop, commit, required, last_unclear, levels, arc, float(dt), tlen)


def hidden_brake_thresholds(speeds, dt, margin, cell_size, T):
    """the threshold table of :meth:`SensorModel.hidden_brake_classes` (DESIGN.md §5.10 "Brake clearance by classes"): host int32
    ``[C, T]``, row c = ``169 * hidden_reach_r2(speeds[c], dt, margin, cell_size, T)`` -- a cell's key is at most ``thr[c, j]`` iff a
    road user of up to ``speeds[c]`` m/s may be in it at sample j"""
    rows = [169 * hidden_reach_r2(float(v), dt, margin, cell_size, T).astype(np.int64) for v in speeds]
    return np.ascontiguousarray(np.stack(rows).astype(np.int32)) if rows else np.zeros((0, int(T)), dtype=np.int32)


@dataclass
class HiddenBrakeClasses:
    """what :meth:`SensorModel.hidden_brake_classes` returns (DESIGN.md §5.10 "Brake clearance by classes"): ``clearance`` is the
    :class:`HiddenClearance` the manoeuvres were held against (``v_cap = max(speeds)``), ``speeds`` the C hidden-user speeds (m/s) in
    the order given, ``thr`` (host int32 ``[C, T]``) their threshold table (:func:`hidden_brake_thresholds`), and (device tensors,
    int32) ``brake_first [C, M, T]``, ``stop [M, T]``, ``commit [C, M]``, ``first [C, M]``: row c of each is, bit for bit,
    ``brake_first`` / ``stop`` / ``commit`` of ``hidden_brake(v_max=speeds[c])`` and ``first`` of its forecast, with the same metric,
    flow, margin and hidden set (see :class:`HiddenBrake` for their meaning).  ``arc``, ``a_brake``, ``dt``, ``lengths`` as there."""
    clearance: HiddenClearance
    speeds: tuple
    thr: np.ndarray
    brake_first: torch.Tensor
    stop: torch.Tensor
    commit: torch.Tensor
    first: torch.Tensor
    arc: torch.Tensor
    a_brake: float
    dt: float
    lengths: Optional[torch.Tensor] = None

    def decided_until(self):
        """``[M]`` int32, as :meth:`HiddenBrake.decided_until`: ``stop`` is the same for every class"""
        return _decided_until(self.stop, self.lengths)

    def critical_speed(self):
        """``[M]`` float64 (m/s): the smallest ``speeds[c]`` with ``commit[c, m] >= 0`` -- the slowest of the given hidden road users
        against which candidate m is not fail-safe over the whole horizon --, ``+inf`` if there is none.  Torch ops on the
        tensors' device, nothing is read back."""
        dev = self.commit.device
        sp = torch.as_tensor(np.asarray(self.speeds, dtype=np.float64).reshape(-1, 1), device=dev)
        inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
        return torch.where(self.commit >= 0, sp, inf).amin(dim=0)


def hidden_brake_classes(self, x, y, theta, v, *, vehicle, speeds, dt, a_brake, margin=None, inflate=0.0, lengths=None,
                         metric="euclid", flow="any", heading=None):
    """Hidden-traffic brake clearance for several hidden-user speeds in one pass (``fo_scene_hidden_brake_classes``; DESIGN.md
    §5.10 "Brake clearance by classes"): runs ``hidden_clearance(..., v_cap=max(speeds), heading=heading)`` and, on the very same
    device inputs, ONE more launch that walks the manoeuvre "follow the candidate until sample b, then brake at ``a_brake``" of
    every (candidate, b) over the key map and decides it for every speed of ``speeds`` (1 .. 8 values, m/s, any order) at once;
    returns a :class:`HiddenBrakeClasses`.  Row c of its outputs is what ``hidden_brake(v_max=speeds[c])`` gives, bit for bit.
    ``len(speeds) * T`` may not exceed ``_native.HIDDEN_BRAKE_MAX_TABLE``: the thresholds travel as a kernel argument.  The other
    arguments as for :meth:`hidden_brake` and :meth:`hidden_clearance`.  Nothing is read back and nobody waits for the kernels."""
    try:
        speeds = tuple(float(s) for s in speeds)
    except TypeError:
        speeds = ()
    if not 1 <= len(speeds) <= N.HIDDEN_BRAKE_MAX_CLASSES or not all(math.isfinite(s) and s >= 0.0 for s in speeds):
        raise ValueError(f"hidden_brake_classes: speeds must hold 1 .. {N.HIDDEN_BRAKE_MAX_CLASSES} finite values >= 0")
    T = int(x.shape[1]) if len(getattr(x, "shape", ())) == 2 else 0
    if len(speeds) * T > N.HIDDEN_BRAKE_MAX_TABLE:
        raise ValueError(f"hidden_brake_classes: {len(speeds)} speeds x {T} samples = {len(speeds) * T} thresholds, at most "
                         f"{N.HIDDEN_BRAKE_MAX_TABLE} are possible (they travel as a kernel argument)")
    clearance = hidden_clearance(self, x, y, theta, vehicle=vehicle, v_cap=max(speeds), dt=dt, margin=margin, inflate=inflate,
                                 lengths=lengths, metric=metric, heading=heading, flow=flow)
    tx, ty, thead, tlen = self._hc_inputs
    M, T = (int(a) for a in tx.shape)
    if tuple(v.shape) != (M, T):
        raise ValueError("hidden_brake_classes: v must be [M, T]")
    a_brake = _a_brake(a_brake, "hidden_brake_classes")
    dev, w, C_ = self.device, clearance.window, len(speeds)
    thr = hidden_brake_thresholds(speeds, clearance.dt, clearance.margin, clearance.cell_size, T)
    tv = N.on_device(v, dev)
    arc = _device_arc(x, y, dev)
    brake_first = torch.empty((C_, M, T), dtype=torch.int32, device=dev)
    stop = torch.empty((M, T), dtype=torch.int32, device=dev)
    commit = torch.empty((C_, M), dtype=torch.int32, device=dev)
    first = torch.empty((C_, M), dtype=torch.int32, device=dev)
    length, width, wb = (float(a) for a in tuple(vehicle)[:3])
    inflate = float(inflate)
    args = N.HiddenBrakeClasses(M=M, T=T, d_x=N.ptr(tx), d_y=N.ptr(ty), d_heading=N.ptr(thead), d_len_or_null=N.ptr(tlen),
                                hl=0.5 * length + inflate, hw=0.5 * width + inflate, wb=wb, win_ix0=w.ix0, win_iy0=w.iy0, win_nx=w.nx,
                                win_ny=w.ny, r2_cap=int(clearance.r2_cap), C=C_, d_key=clearance.key.data_ptr(), d_qmin=N.ptr(clearance.qmin),
                                d_v=N.ptr(tv), d_arc=N.ptr(arc), a_brake=a_brake, dt=float(dt), h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)),
                                d_brake_first=N.ptr(brake_first), d_stop=N.ptr(stop), d_commit=N.ptr(commit), d_first=N.ptr(first))
    self.ctx.call("fo_scene_hidden_brake_classes", C.byref(args), N.current_stream(self._dev_index))
    self._hbc_inputs = (tv, arc)                            # (stay referenced until the next call, as in hidden_brake)
    return HiddenBrakeClasses(clearance, speeds, thr, brake_first, stop, commit, first, arc, a_brake, float(dt), tlen)


@dataclass
class HiddenBrakeUsers:
    """what :meth:`SensorModel.hidden_brake_users` returns (DESIGN.md §5.10 "Brake clearance by road users"): ``users`` the C hidden
    road users ``(speed, metric, flow)`` in the order given, ``clearances`` one :class:`HiddenClearance` per distinct
    ``(metric, flow)`` in order of first appearance (``v_cap`` = the fastest of its users), ``map_of`` (tuple of C ints) the
    clearance each user is held against, ``thr`` (host int32 ``[C, T]``) the threshold table (:func:`hidden_brake_thresholds` of the
    users' speeds), and (device tensors, int32) ``brake_first [C, M, T]``, ``stop [M, T]``, ``commit [C, M]``, ``first [C, M]``: row c
    of each is, bit for bit, what ``hidden_brake_classes(speeds=(speed_c,), metric=metric_c, flow=flow_c)`` and
    ``hidden_brake(v_max=speed_c, metric=metric_c, flow=flow_c)`` give.  ``arc``, ``a_brake``, ``dt``, ``lengths`` as in
    :class:`HiddenBrake`."""
    clearances: tuple
    users: tuple
    map_of: tuple
    thr: np.ndarray
    brake_first: torch.Tensor
    stop: torch.Tensor
    commit: torch.Tensor
    first: torch.Tensor
    arc: torch.Tensor
    a_brake: float
    dt: float
    lengths: Optional[torch.Tensor] = None

    def decided_until(self):
        """``[M]`` int32, as :meth:`HiddenBrake.decided_until`: ``stop`` is the same for every user"""
        return _decided_until(self.stop, self.lengths)

    def critical_user(self):
        """``[M]`` int64: the index of the slowest user with ``commit[c, m] >= 0`` -- the lowest index among equal speeds --, -1 if
        the candidate is fail-safe against every user.  Torch ops on the tensors' device, nothing is read back."""
        dev = self.commit.device
        speeds = [u[0] for u in self.users]
        order = sorted(range(len(speeds)), key=lambda c: (speeds[c], c))        # a stable ranking: rank r is user order[r]
        rank = torch.as_tensor(np.argsort(np.asarray(order, dtype=np.int64)).reshape(-1, 1), device=dev)
        best = torch.where(self.commit >= 0, rank, len(speeds)).amin(dim=0)
        users = torch.as_tensor(np.asarray(order + [-1], dtype=np.int64), device=dev)
        return users[best]

    def critical_speed(self):
        """``[M]`` float64 (m/s): the speed of :meth:`critical_user`, ``+inf`` if there is none"""
        dev = self.commit.device
        sp = torch.as_tensor(np.asarray([u[0] for u in self.users] + [float("inf")], dtype=np.float64), device=dev)
        return sp[self.critical_user()]


def _road_users(users, x, fn):
    """the users of ``fn`` (hidden_brake_users and its ladder) as a tuple of ``(float speed, metric, flow)``, or its refusal"""
    try:
        users = tuple(users)
    except TypeError:
        users = ()
    if not 1 <= len(users) <= N.HIDDEN_BRAKE_MAX_CLASSES:
        raise ValueError(f"{fn}: users must hold 1 .. {N.HIDDEN_BRAKE_MAX_CLASSES} triples (speed, metric, flow)")
    for c, u in enumerate(users):
        try:
            s, m, f = u
            s = float(s)
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: users[{c}] = {u!r} is no triple (speed, metric, flow) with a number for the speed") from None
    users = tuple((float(s), m, f) for s, m, f in users)
    for c, (s, m, f) in enumerate(users):
        if m not in HIDDEN_REACH_METRICS:
            raise ValueError(f"{fn}: users[{c}]: metric {m!r}, one of {HIDDEN_REACH_METRICS} is possible")
        if f not in HIDDEN_REACH_FLOWS:
            raise ValueError(f"{fn}: users[{c}]: flow {f!r}, one of {HIDDEN_REACH_FLOWS} is possible")
        if f == "lanes" and m != "road":
            raise ValueError(f"{fn}: users[{c}]: flow 'lanes' follows the lanes along the road: it needs metric 'road', "
                             f"not {m!r}")
    if not all(math.isfinite(s) and s >= 0.0 for s, _, _ in users):
        raise ValueError(f"{fn}: the users' speeds must be finite and >= 0")
    T = int(x.shape[1]) if len(getattr(x, "shape", ())) == 2 else 0
    if len(users) * T > N.HIDDEN_BRAKE_MAX_TABLE:
        raise ValueError(f"{fn}: {len(users)} users x {T} samples = {len(users) * T} thresholds, at most "
                         f"{N.HIDDEN_BRAKE_MAX_TABLE} are possible (they travel as a kernel argument)")
    return users


def _users_clearances(self, users, x, y, theta, *, vehicle, dt, margin, inflate, lengths, heading):
    """``(maps, map_of, clearances)``: one ``hidden_clearance`` per distinct ``(metric, flow)`` of ``users`` in order of first
    appearance, each at the fastest of its users; the first call's device inputs and heading tensor go to the later ones"""
    maps = []                                               # the distinct (metric, flow) in order of first appearance: at most three
    for _, m, f in users:
        if (m, f) not in maps:
            maps.append((m, f))
    map_of = tuple(maps.index((m, f)) for _, m, f in users)
    clearances = []
    cx, cy, clen = x, y, lengths
    for k, (m, f) in enumerate(maps):
        v_cap = max(s for c, (s, _, _) in enumerate(users) if map_of[c] == k)
        clearances.append(hidden_clearance(self, cx, cy, theta, vehicle=vehicle, v_cap=v_cap, dt=dt, margin=margin, inflate=inflate,
                                           lengths=clen, metric=m, heading=heading, flow=f))
        cx, cy, heading, clen = self._hc_inputs             # the later clearances take the first one's device inputs and headings
    return maps, map_of, clearances


@dataclass
class _UsersCall:
    """what the callers of the users family (hidden_brake_users, its ladder and the two verdicts) prepare alike: the ``clearances``
    and ``map_of`` of :func:`_users_clearances`, the device inputs ``x, y, heading, lengths`` of the first of them, ``M, T``,
    the threshold table ``thr`` of the users' speeds, and the half extents ``hl, hw`` and ``wb`` of the ego rectangle"""
    clearances: tuple
    map_of: tuple
    x: torch.Tensor
    y: torch.Tensor
    heading: torch.Tensor
    lengths: Optional[torch.Tensor]
    M: int
    T: int
    thr: np.ndarray
    hl: float
    hw: float
    wb: float

    def fields(self, tv, arc, dt):
        """the members every structure of the family begins with (``M`` .. ``d_arc``; _native._HIDDEN_USERS_HEAD), ``dt`` and
        ``h_thr``, as keyword arguments"""
        cl, w = self.clearances, self.clearances[0].window
        maps_t, caps_t, classes_t = (C.c_void_p * N.HIDDEN_BRAKE_MAX_MAPS, C.c_int32 * N.HIDDEN_BRAKE_MAX_MAPS,
                                     C.c_int32 * N.HIDDEN_BRAKE_MAX_CLASSES)
        pad = lambda vals: list(vals) + [None] * (N.HIDDEN_BRAKE_MAX_MAPS - len(vals))
        return dict(M=self.M, T=self.T, d_x=N.ptr(self.x), d_y=N.ptr(self.y), d_heading=N.ptr(self.heading),
                    d_len_or_null=N.ptr(self.lengths), hl=self.hl, hw=self.hw, wb=self.wb, win_ix0=w.ix0, win_iy0=w.iy0,
                    win_nx=w.nx, win_ny=w.ny, K=len(cl), C=len(self.map_of),
                    d_key=maps_t(*pad([c.key.data_ptr() for c in cl])), d_qmin=maps_t(*pad([N.ptr(c.qmin) for c in cl])),
                    r2_cap=caps_t(*[int(c.r2_cap) for c in cl]), map_of=classes_t(*self.map_of), d_v=N.ptr(tv), d_arc=N.ptr(arc),
                    dt=float(dt), h_thr=self.thr.ctypes.data_as(C.POINTER(C.c_int32)))


def _users_call(self, fn, users, x, y, theta, v, *, vehicle, dt, margin, inflate, lengths, heading=None, poses=None):
    """the :class:`_UsersCall` of ``fn`` for the ``users`` that :func:`_road_users` let through: runs the clearances, then refuses a
    ``v`` of another shape.  ``poses``: the :class:`HiddenPoses` a verdict walks on -- the clearances take its heading (no ``theta``),
    and its arc and finite flag are held to the shape too"""
    if poses is not None:
        theta, heading = None, poses.heading
    _, map_of, clearances = _users_clearances(self, users, x, y, theta, vehicle=vehicle, dt=dt, margin=margin, inflate=inflate,
                                              lengths=lengths, heading=heading)
    M, T = (int(a) for a in self._hc_inputs[0].shape)
    if poses is None and tuple(v.shape) != (M, T):
        raise ValueError(f"{fn}: v must be [M, T]")
    if poses is not None and (tuple(v.shape) != (M, T) or tuple(poses.arc.shape) != (M, T) or tuple(poses.finite.shape) != (M,)):
        raise ValueError(f"{fn}: v and poses.arc must be [M, T], poses.finite [M]")
    first_c = clearances[0]
    thr = hidden_brake_thresholds([s for s, _, _ in users], first_c.dt, first_c.margin, first_c.cell_size, T)
    length, width, wb = (float(a) for a in tuple(vehicle)[:3])
    inflate = float(inflate)
    return _UsersCall(tuple(clearances), map_of, *self._hc_inputs, M, T, thr, 0.5 * length + inflate, 0.5 * width + inflate, wb)


def _arg_bytes(users, x, levels, noun, fn):
    """refuses thresholds and ``levels`` (``noun``: what ``fn`` calls them) that together overflow the kernel argument they travel as"""
    T = int(x.shape[1]) if len(getattr(x, "shape", ())) == 2 else 0
    if 4 * len(users) * T + 8 * len(levels) > N.HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES:
        raise ValueError(f"{fn}: {len(users)} users x {T} samples = {len(users) * T} thresholds of 4 bytes and {len(levels)} {noun} "
                         f"of 8 bytes are {4 * len(users) * T + 8 * len(levels)} bytes, at most "
                         f"{N.HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES} are possible (they travel as a kernel argument)")


def _cost_safe(cost, safe, M, device, fn):
    """refuses a verdict's ``cost`` / ``safe`` that do not come as a pair or are not the ``M`` rows of a sweep on ``device``"""
    if (cost is None) != (safe is None):
        raise ValueError(f"{fn}: cost and safe go together: give both or neither")
    if cost is not None:
        ok = (torch.is_tensor(cost) and torch.is_tensor(safe) and cost.device == device == safe.device and cost.dtype == torch.float64
              and safe.dtype == torch.uint8 and tuple(cost.shape) == (M, N.NC) and tuple(safe.shape) == (M,) and cost.is_contiguous()
              and safe.is_contiguous())
        if not ok:
            raise ValueError(f"{fn}: cost must be a contiguous float64 [M, {N.NC}] and safe a uint8 [M] tensor on the model's device "
                             "(they are written in place)")


def hidden_brake_users(self, x, y, theta, v, *, vehicle, users, dt, a_brake, margin=None, inflate=0.0, lengths=None, heading=None):
    """Hidden-traffic brake clearance for mixed road users in one walk (``fo_scene_hidden_brake_users``; DESIGN.md §5.10 "Brake
    clearance by road users"): ``users`` is a sequence of 1 .. 8 ``(speed, metric, flow)`` -- say ``(2.0, "road", "any")`` for a
    pedestrian, ``(7.0, "road", "lanes")`` for a cyclist and ``(13.9, "road", "lanes")`` for a car.  Runs one
    ``hidden_clearance`` per distinct ``(metric, flow)`` (``v_cap`` = the fastest of its users; the first call's heading tensor and
    device inputs go to the later ones, so there is one host-side heading pass) and then ONE launch that walks the manoeuvre of every
    (candidate, b) once and decides it for every user on that user's key map; returns a :class:`HiddenBrakeUsers`.
    ``len(users) * T`` may not exceed ``_native.HIDDEN_BRAKE_MAX_TABLE``.  The other arguments as for :meth:`hidden_brake_classes`.
    Nothing is read back and nobody waits for the kernels."""
    fn = "hidden_brake_users"
    users = _road_users(users, x, fn)
    p = _users_call(self, fn, users, x, y, theta, v, vehicle=vehicle, dt=dt, margin=margin, inflate=inflate, lengths=lengths,
                    heading=heading)
    a_brake = _a_brake(a_brake, fn)
    dev, M, T, C_ = self.device, p.M, p.T, len(users)
    tv = N.on_device(v, dev)
    arc = _device_arc(x, y, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    brake_first, stop, commit, first = new(C_, M, T), new(M, T), new(C_, M), new(C_, M)
    args = N.HiddenBrakeUsers(**p.fields(tv, arc, dt), a_brake=a_brake, d_brake_first=N.ptr(brake_first), d_stop=N.ptr(stop),
                              d_commit=N.ptr(commit), d_first=N.ptr(first))
    self.ctx.call("fo_scene_hidden_brake_users", C.byref(args), N.current_stream(self._dev_index))
    # (stay referenced until the next call, as in hidden_brake_classes -- the clearances' maps too: the caller may drop the result)
    self._hbu_inputs = (tv, arc, p.clearances)
    return HiddenBrakeUsers(p.clearances, users, p.map_of, p.thr, brake_first, stop, commit, first, arc, a_brake, float(dt), p.lengths)


@dataclass
class HiddenBrakeLadderUsers:
    """what :meth:`SensorModel.hidden_brake_ladder_users` returns (DESIGN.md §5.10 "Brake ladder by road users"): ``clearances``,
    ``users``, ``map_of`` and ``thr`` as in :class:`HiddenBrakeUsers`, ``decelerations`` (host float64 ``[L]``, strictly ascending) the
    ladder, and (device tensors, int32) per user ``required [C, M, B]``, ``last_unclear [C, M, B]``, ``commit [C, M, L]`` -- row c is
    what :class:`HiddenBrakeLadder` holds against that user's forecast -- and ``first [C, M]``; over the users ``required_all [M, B]``
    -- the first level at which "follow candidate m until sample b, then brake" stays clear of EVERY user while it moves, -1 = no
    level of the ladder does --, ``last_unclear_all [M, B]`` -- the last level at which some user is not clear, -1 = none -- and
    ``blocking [M, B]``, a bit mask: bit c is set iff user c is unclear at level ``required_all - 1`` (at the last level where
    ``required_all`` is -1; 0 where it is 0) -- the users that keep the ego from the next gentler level.  All four are -1 (``blocking``
    0) where there is no manoeuvre (``b >= lengths[m]``).  With ``detail``: ``brake_first [C, M, B, L]`` and ``stop [M, B, L]`` -- slice
    l is ``hidden_brake_users(a_brake=decelerations[l])`` at the brake starts ``b < B``, bit for bit --, else both None.  ``arc``,
    ``dt``, ``lengths`` as in :class:`HiddenBrake`.

    Not claimed: what :class:`HiddenBrakeUsers` and :class:`HiddenBrakeLadder` do not claim.  ``required_all`` is NOT the maximum of
    the users' ``required``: harder braking is not always safer against a map, so the first level clear of every user can lie above
    every single user's own."""
    clearances: tuple
    users: tuple
    map_of: tuple
    thr: np.ndarray
    decelerations: np.ndarray
    required: torch.Tensor
    last_unclear: torch.Tensor
    commit: torch.Tensor
    first: torch.Tensor
    required_all: torch.Tensor
    last_unclear_all: torch.Tensor
    blocking: torch.Tensor
    brake_first: Optional[torch.Tensor]
    stop: Optional[torch.Tensor]
    arc: torch.Tensor
    dt: float
    lengths: Optional[torch.Tensor] = None

    def _pair(self, user):
        if user is None:
            return self.required_all, self.last_unclear_all
        return self.required[user], self.last_unclear[user]

    def required_deceleration(self, user=None):
        """``[M, B]`` float64 (m/s^2): ``decelerations[required_all]`` -- of ``required[user]`` with ``user`` --; ``+inf`` where a
        manoeuvre exists and no level of the ladder is clear; ``nan`` where there is no manoeuvre.  Torch ops on the tensors' device,
        nothing is read back."""
        required, last_unclear = self._pair(user)
        dev = required.device
        levels = torch.as_tensor(np.append(np.asarray(self.decelerations, dtype=np.float64), np.inf), device=dev)
        req = required.to(torch.int64)
        out = levels[torch.where(req >= 0, req, len(levels) - 1)]
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        return torch.where((req < 0) & (last_unclear < 0), nan, out)

    def brake_threat_number(self, a_max, user=None):
        """``[M, B]`` float64: :meth:`required_deceleration` divided by ``a_max`` -- the reference's ``break_threat_number``
        (metrics/be.py:56) against the hidden road users, or one of them"""
        return self.required_deceleration(user) / float(a_max)

    def monotone(self, user=None):
        """``[M, B]`` bool, as :meth:`HiddenBrakeLadder.monotone`, over all users or for one"""
        required, last_unclear = self._pair(user)
        return (required == last_unclear + 1) | (required == -1)

    def blocking_users(self):
        """``[C, M, B]`` bool: bit c of ``blocking``"""
        bits = torch.arange(len(self.users), dtype=torch.int32, device=self.blocking.device).reshape(-1, 1, 1)
        return (self.blocking.unsqueeze(0) >> bits & 1) != 0

    def level(self, l):
        """``(brake_first [C, M, B], stop [M, B], commit [C, M])`` of level l: what ``hidden_brake_users(a_brake=decelerations[l])``
        gives at the brake starts ``b < B`` (views, nothing is copied); needs ``detail``"""
        if self.brake_first is None:
            raise ValueError("HiddenBrakeLadderUsers.level: brake_first and stop were not asked for (detail=True)")
        return self.brake_first[..., l], self.stop[..., l], self.commit[..., l]


def hidden_brake_ladder_users(self, x, y, theta, v, *, vehicle, users, dt, decelerations, starts=None, detail=False, margin=None,
                              inflate=0.0, lengths=None, heading=None):
    """Hidden-traffic brake ladder for mixed road users in one walk (``fo_scene_hidden_brake_ladder_users``; DESIGN.md §5.10 "Brake
    ladder by road users"): ``users`` as for :meth:`hidden_brake_users`, ``decelerations`` and ``starts`` as for
    :meth:`hidden_brake_ladder`.  Runs one ``hidden_clearance`` per distinct ``(metric, flow)`` as :meth:`hidden_brake_users` does and
    then ONE launch that walks the manoeuvre of every (candidate, b, deceleration) once and decides it for every user on that user's
    key map; returns a :class:`HiddenBrakeLadderUsers`, whose ``required_all`` is the gentlest deceleration of the ladder that keeps
    the moving ego clear of every user.  ``detail``: also ``brake_first [C, M, B, L]`` and ``stop [M, B, L]`` (4 (C + 1) M B L bytes).
    ``4 * len(users) * T + 8 * len(decelerations)`` may not exceed ``_native.HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES``.  Nothing is read
    back and nobody waits for the kernels."""
    fn = "hidden_brake_ladder_users"
    users = _road_users(users, x, fn)
    levels = _ladder_levels(decelerations, fn)
    _arg_bytes(users, x, levels, "decelerations", fn)
    p = _users_call(self, fn, users, x, y, theta, v, vehicle=vehicle, dt=dt, margin=margin, inflate=inflate, lengths=lengths,
                    heading=heading)
    B = _ladder_starts(starts, p.T, fn)
    dev, M, C_, L_ = self.device, p.M, len(users), len(levels)
    tv = N.on_device(v, dev)
    arc = _device_arc(x, y, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    required, last_unclear, commit, first = new(C_, M, B), new(C_, M, B), new(C_, M, L_), new(C_, M)
    required_all, last_unclear_all, blocking = new(M, B), new(M, B), new(M, B)
    brake_first, stop = (new(C_, M, B, L_), new(M, B, L_)) if detail else (None, None)
    args = N.HiddenBrakeLadderUsers(**p.fields(tv, arc, dt), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), L=L_, B=B,
                                    d_required=N.ptr(required), d_last_unclear=N.ptr(last_unclear), d_commit=N.ptr(commit),
                                    d_first=N.ptr(first), d_required_all=N.ptr(required_all), d_last_unclear_all=N.ptr(last_unclear_all),
                                    d_blocking=N.ptr(blocking), d_brake_first_or_null=N.ptr(brake_first), d_stop_or_null=N.ptr(stop))
    self.ctx.call("fo_scene_hidden_brake_ladder_users", C.byref(args), N.current_stream(self._dev_index))
    # (stay referenced until the next call, as in hidden_brake_users)
    self._hblu_inputs = (tv, arc, p.clearances)
    return HiddenBrakeLadderUsers(p.clearances, users, p.map_of, p.thr, levels, required, last_unclear, commit, first, required_all,
                                  last_unclear_all, blocking, brake_first, stop, arc, float(dt), p.lengths)


@dataclass
class HiddenPoses:
    """what :meth:`SensorModel.hidden_poses` returns (device tensors; DESIGN.md §5.10 "Fail-safe verdict"): ``heading [M, T, 2]``
    float64 -- (cos, sin) of the sample headings from one ``sincos`` per sample, the bits the sweep rotates the ego rectangle by;
    ``arc [M, T]`` float64 -- the travelled chord length as numpy's :func:`travelled_arc` sums it on host arrays (sequentially);
    ``finite [M]`` uint8 -- 1 iff every x, y, theta, v of the samples ``k < lengths[m]`` is finite.  Hand it to a later call of the
    SAME candidates as ``poses=``."""
    heading: torch.Tensor
    arc: torch.Tensor
    finite: torch.Tensor


def hidden_poses(self, x, y, theta, v, lengths=None):
    """Device pose preparation (``fo_scene_hidden_poses``): (cos, sin), travelled arc and finite flag of the candidates
    ``x, y, theta, v [M, T]`` in one launch on the current stream; returns a :class:`HiddenPoses`.  Candidates that live on the device
    stay there: nothing is copied back and nobody waits (host arrays are uploaded first).  Needs no previous ``launch()``."""
    fn = "hidden_poses"
    shape = tuple(x.shape)
    if len(shape) != 2 or any(tuple(q.shape) != shape for q in (y, theta, v)):
        raise ValueError(f"{fn}: x, y, theta and v must be [M, T]")
    M, T = (int(a) for a in shape)
    if M and not 1 <= T <= N.HIDDEN_REACH_MAX_J:
        raise ValueError(f"{fn}: {T} samples per trajectory, 1 .. {N.HIDDEN_REACH_MAX_J} are possible")
    if lengths is not None and tuple(np.shape(lengths)) != (M,):
        raise ValueError(f"{fn}: lengths must be [M]")
    dev = self.device
    tx, ty, tth, tv = (N.on_device(q, dev) for q in (x, y, theta, v))
    tlen = None if lengths is None else N.on_device(lengths, dev, "int32")
    heading = torch.empty((M, T, 2), dtype=torch.float64, device=dev)
    arc = torch.empty((M, T), dtype=torch.float64, device=dev)
    finite = torch.empty((M,), dtype=torch.uint8, device=dev)
    args = N.HiddenPoses(M=M, T=T, d_x=N.ptr(tx), d_y=N.ptr(ty), d_theta=N.ptr(tth), d_v=N.ptr(tv), d_len_or_null=N.ptr(tlen),
                         d_heading=N.ptr(heading), d_arc=N.ptr(arc), d_finite=N.ptr(finite))
    self.ctx.call("fo_scene_hidden_poses", C.byref(args), N.current_stream(self._dev_index))
    self._hp_inputs = (tx, ty, tth, tv, tlen)               # (stay referenced until the next call, as in hidden_reach)
    return HiddenPoses(heading, arc, finite)


@dataclass
class HiddenBrakeVerdict:
    """what :meth:`SensorModel.hidden_brake_verdict` returns (DESIGN.md §5.10 "Fail-safe verdict"; device tensors, int32):
    ``fail_safe [M]`` -- the number of leading brake starts, of the ``starts`` that were walked, from which braking keeps the moving
    ego clear of every user (0: not even now; ``starts``: throughout); ``user [M]`` -- the lowest user that ends them, -1 = none,
    -2 = the candidate has a non-finite pose and fails closed (``fail_safe`` 0); ``commit [C, M]`` -- ``hidden_brake_users``' commit
    where it is below ``starts``, else -1; ``first [C, M]`` -- that call's ``first``.  ``poses`` the :class:`HiddenPoses` it walked
    on, ``commit_min`` the bound below which a candidate lost its safety flag, ``users``, ``map_of``, ``thr``, ``clearances`` as in
    :class:`HiddenBrakeUsers`."""
    fail_safe: torch.Tensor
    user: torch.Tensor
    commit: torch.Tensor
    first: torch.Tensor
    poses: HiddenPoses
    starts: int
    commit_min: int
    users: tuple = ()
    map_of: tuple = ()
    thr: Optional[np.ndarray] = None
    clearances: tuple = ()

    def critical_user(self):
        """``[M]`` int64: the user that ends a candidate's fail-safe brake starts (the lowest index among those that do so at the
        same start), -1 where the candidate is fail-safe throughout ``starts``, -2 where it has a non-finite pose.  Nothing is read
        back."""
        return self.user.to(torch.int64)


def hidden_brake_verdict(self, x, y, theta, v, *, vehicle, users, dt, a_brake, starts, commit_min, cost=None, safe=None, margin=None,
                         inflate=0.0, lengths=None, poses=None):
    """Hidden-traffic fail-safe verdict (``fo_scene_hidden_brake_verdict``; DESIGN.md §5.10 "Fail-safe verdict"): for the hidden road
    ``users`` of :meth:`hidden_brake_users`, over the first ``starts`` brake starts alone (an integer in ``[1, T]``, None = T: what a
    planner executes before it replans), how long each candidate stays fail-safe -- and, with ``cost [M, 16]`` float64 / ``safe [M]``
    uint8 of a sweep or planning step over the SAME candidates (both or neither), that answer in the two reserved cost columns, and
    ``safe = 0`` where ``fail_safe < commit_min`` (``0 <= commit_min <= starts``).  The stage only ever takes safety away.

    Everything runs on the device and on the current stream: the pose preparation (:meth:`hidden_poses`; ``poses=`` an earlier
    :class:`HiddenPoses` of the same candidates skips it, ``theta`` may then be None), one ``hidden_clearance`` per distinct
    ``(metric, flow)`` on the device headings, and ONE launch for the walk and the fold.  Nothing is read back and nobody waits;
    returns a :class:`HiddenBrakeVerdict`.  The other arguments as for :meth:`hidden_brake_users`."""
    fn = "hidden_brake_verdict"
    users = _road_users(users, x, fn)
    if poses is None:
        poses = hidden_poses(self, x, y, theta, v, lengths)
    p = _users_call(self, fn, users, x, y, None, v, vehicle=vehicle, dt=dt, margin=margin, inflate=inflate, lengths=lengths, poses=poses)
    a_brake = _a_brake(a_brake, fn)
    B = _ladder_starts(starts, p.T, fn)
    if isinstance(commit_min, bool) or not isinstance(commit_min, (int, np.integer)) or not 0 <= int(commit_min) <= B:
        raise ValueError(f"{fn}: commit_min = {commit_min!r}, an integer in [0, starts = {B}]")
    commit_min = int(commit_min)
    dev, M, C_ = self.device, p.M, len(users)
    _cost_safe(cost, safe, M, p.x.device, fn)
    tv = N.on_device(v, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    fail_safe, user, commit, first = new(M), new(M), new(C_, M), new(C_, M)
    args = N.HiddenBrakeVerdict(**p.fields(tv, poses.arc, dt), a_brake=a_brake, B=B, commit_min=commit_min,
                                d_finite_or_null=N.ptr(poses.finite), d_cost_or_null=N.ptr(cost), d_safe_or_null=N.ptr(safe),
                                d_fail_safe=N.ptr(fail_safe), d_user=N.ptr(user), d_commit=N.ptr(commit), d_first=N.ptr(first))
    self.ctx.call("fo_scene_hidden_brake_verdict", C.byref(args), N.current_stream(self._dev_index))
    # (stay referenced until the next call, as in hidden_brake_users)
    self._hbv_inputs = (tv, poses, p.clearances, cost, safe)
    self._hbv_args = args                                   # (the structure of the last call: tools/hidden_reach_bench.py replays the launch alone)
    return HiddenBrakeVerdict(fail_safe, user, commit, first, poses, B, commit_min, users, p.map_of, p.thr, p.clearances)


@dataclass
class HiddenBrakeLadderVerdict:
    """what :meth:`SensorModel.hidden_brake_ladder_verdict` returns (DESIGN.md §5.10 "Ladder verdict"; device tensors): with ``ra``,
    ``blk``, ``req`` for ``required_all``, ``blocking``, ``required`` of :class:`HiddenBrakeLadderUsers` on the same inputs and
    ``ends = min(starts, lengths[m])`` -- ``need [M]`` int32, the largest ``ra[m, b]`` over ``b < ends`` with -1 ("no level") counted
    as ``L = len(levels)``: the level the worst brake start needs, -1 where ``ends`` is 0; ``at [M]`` the first such start, -1 =
    none; ``blocking [M]`` = ``blk[m, at[m]]``, the users that keep that start from the next gentler level; ``user [M]`` its lowest
    set bit, -1 = none, -2 = the candidate has a non-finite pose and fails closed (``need`` L, ``decel`` inf); ``decel [M]`` float64
    = ``levels[need]``, ``+inf`` for ``need == L``, 0.0 for ``need == -1``; per user ``need_of [C, M]`` -- the same maximum over
    ``req[c]`` -- and ``first [C, M]``.  ``poses`` the :class:`HiddenPoses` it walked on, ``levels`` (host float64 ``[L]``, strictly
    ascending), ``starts``, ``a_limit`` (above it a candidate lost its safety flag), ``users``, ``map_of``, ``thr``, ``clearances``
    as in :class:`HiddenBrakeUsers`.

    Not claimed: what :class:`HiddenBrakeLadderUsers` does not claim; the answer is only as fine as the ladder."""
    need: torch.Tensor
    at: torch.Tensor
    blocking: torch.Tensor
    user: torch.Tensor
    decel: torch.Tensor
    need_of: torch.Tensor
    first: torch.Tensor
    levels: np.ndarray
    starts: int
    a_limit: float
    users: tuple = ()
    poses: Optional[HiddenPoses] = None
    map_of: tuple = ()
    thr: Optional[np.ndarray] = None
    clearances: tuple = ()

    def required_deceleration(self):
        """``[M]`` float64 (m/s^2): ``decel`` -- what the cost row holds in its first reserved column"""
        return self.decel

    def brake_threat_number(self, a_max):
        """``[M]`` float64: ``decel / a_max`` -- the reference's ``break_threat_number`` (metrics/be.py:56) against the hidden road
        users, from the worst of the brake starts walked.  Nothing is read back."""
        return self.decel / float(a_max)

    def critical_user(self):
        """``[M]`` int64: the lowest user that keeps the worst brake start from the next gentler level, -1 = none, -2 where the
        candidate has a non-finite pose.  Nothing is read back."""
        return self.user.to(torch.int64)


def hidden_brake_ladder_verdict(self, x, y, theta, v, *, vehicle, users, dt, levels=None, starts, a_limit, cost=None, safe=None,
                                margin=None, inflate=0.0, lengths=None, poses=None):
    """Hidden-traffic ladder verdict (``fo_scene_hidden_brake_ladder_verdict``; DESIGN.md §5.10 "Ladder verdict"): for the hidden
    road ``users`` of :meth:`hidden_brake_users` and the ladder ``levels`` of :meth:`hidden_brake_ladder_users` (None: 0.5, 1.0, ...
    up to ``a_limit``, which must then be finite), over the first ``starts`` brake starts alone (an integer in ``[1, T]``, None = T:
    what a planner executes before it replans), the gentlest deceleration of the ladder that keeps the moving ego clear of every user
    from the WORST of those starts -- and, with ``cost [M, 16]`` float64 / ``safe [M]`` uint8 of a sweep or planning step over the
    SAME candidates (both or neither), that deceleration and the blocking user in the two reserved cost columns, and ``safe = 0``
    where no level suffices or the deceleration exceeds ``a_limit`` (``>= 0``, ``inf`` allowed).  The stage only ever takes safety
    away.  It owns the same two columns as :meth:`hidden_brake_verdict`: fold one or the other into a row.

    Everything runs on the device and on the current stream: the pose preparation (:meth:`hidden_poses`; ``poses=`` an earlier
    :class:`HiddenPoses` of the same candidates skips it, ``theta`` may then be None), one ``hidden_clearance`` per distinct
    ``(metric, flow)`` on the device headings, and ONE launch for the walk, the reduction over the brake starts and the fold.
    Nothing is read back and nobody waits; returns a :class:`HiddenBrakeLadderVerdict`."""
    fn = "hidden_brake_ladder_verdict"
    users = _road_users(users, x, fn)
    try:
        a_limit = float(a_limit)
    except (TypeError, ValueError):
        a_limit = float("nan")
    if not a_limit >= 0.0:
        raise ValueError(f"{fn}: a_limit >= 0 (inf is possible, nan is not)")
    if levels is None:
        if not math.isfinite(a_limit):
            raise ValueError(f"{fn}: the default levels run up to a_limit, which is not finite: hand levels over")
        levels = default_brake_ladder(a_limit, fn)
    levels = _ladder_levels(levels, fn)
    _arg_bytes(users, x, levels, "levels", fn)
    if poses is None:
        poses = hidden_poses(self, x, y, theta, v, lengths)
    p = _users_call(self, fn, users, x, y, None, v, vehicle=vehicle, dt=dt, margin=margin, inflate=inflate, lengths=lengths, poses=poses)
    B = _ladder_starts(starts, p.T, fn)
    dev, M, C_, L_ = self.device, p.M, len(users), len(levels)
    _cost_safe(cost, safe, M, p.x.device, fn)
    tv = N.on_device(v, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    need, at, blocking, user, need_of, first = new(M), new(M), new(M), new(M), new(C_, M), new(C_, M)
    decel = torch.empty((M,), dtype=torch.float64, device=dev)
    args = N.HiddenBrakeLadderVerdict(**p.fields(tv, poses.arc, dt), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), L=L_, B=B,
                                      a_limit=a_limit, d_finite_or_null=N.ptr(poses.finite), d_cost_or_null=N.ptr(cost),
                                      d_safe_or_null=N.ptr(safe), d_need=N.ptr(need), d_at=N.ptr(at), d_blocking=N.ptr(blocking),
                                      d_user=N.ptr(user), d_decel=N.ptr(decel), d_need_of=N.ptr(need_of), d_first=N.ptr(first))
    self.ctx.call("fo_scene_hidden_brake_ladder_verdict", C.byref(args), N.current_stream(self._dev_index))
    # (stay referenced until the next call, as in hidden_brake_users)
    self._hblv_inputs = (tv, poses, p.clearances, cost, safe)
    self._hblv_args = args                                  # (the structure of the last call: tools/hidden_reach_bench.py replays the launch alone)
    return HiddenBrakeLadderVerdict(need, at, blocking, user, decel, need_of, first, levels, B, a_limit, users, poses, p.map_of, p.thr,
                                    p.clearances)


def hidden_impact_rows(kinds, ego_mass, coeff=None, fn="hidden_impact_rows"):
    """The harm rows ``[C, 4]`` (host float64) of the road users ``kinds`` -- one ``(type_name, length, width)`` each -- against an
    ego of ``ego_mass`` kg, from the library's own ``fo_hidden_impact_row`` (csrc/fo_hidden_impact.hpp, where what a row means
    stands); ``coeff``: the entries of harm_params.json as :func:`metrics.metric.load_harm_coeff` returns them (None: the package's).
    A type the reference has no protection entry for is refused."""
    from .metrics.metric import load_harm_coeff
    coeff = load_harm_coeff() if coeff is None else dict(coeff)
    try:
        if set(coeff) != {n for n, _ in N.HarmCoeff._fields_}:
            raise TypeError
        hc = N.HarmCoeff(**{k: float(v) for k, v in coeff.items()})
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: coeff must hold the eight entries of harm_params.json (metrics.metric.load_harm_coeff)") from None
    try:
        ego_mass = float(ego_mass)
    except (TypeError, ValueError):
        ego_mass = float("nan")
    if not (ego_mass > 0.0 and math.isfinite(ego_mass)):
        raise ValueError(f"{fn}: ego_mass must be positive and finite")
    rows = np.empty((len(kinds), 4), dtype=np.float64)
    lib = N.load()
    for c, kind in enumerate(kinds):
        try:
            name, length, width = kind
            code = N.TYPE_CODES.get(str(name).lower(), -1)
            size = float(length) * float(width)
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: kinds[{c}] = {kind!r}, a (type_name, length, width) is needed") from None
        if code < 0:
            raise ValueError(f"{fn}: kinds[{c}]: the harm model has no protection entry for the type {name!r}")
        if not (size > 0.0 and math.isfinite(size)):
            raise ValueError(f"{fn}: kinds[{c}]: length and width must be positive and finite")
        row = (C.c_double * 4)()
        if lib.fo_hidden_impact_row(code, size, ego_mass, C.byref(hc), row) != N.FO_OK:
            raise ValueError(f"{fn}: kinds[{c}] = {kind!r} has no harm row")
        rows[c] = row[:]
    return rows


@dataclass
class HiddenBrakeImpact:
    """what :meth:`SensorModel.hidden_brake_impact` returns (DESIGN.md §5.10 "Impact verdict"; device tensors): ``harm [M, 2]`` float64
    -- (obstacle harm, ego harm), the reference's MAIS3+ probabilities head-on and at the worst area of impact, of the user whose
    obstacle harm is greatest at the speed the ego has left where it is hit; (0, 0) where no user hits a brake start, (1, 1) where the
    candidate has a non-finite pose and fails closed; ``user [M]`` int32 that user (the lowest on a tie), -1 = none, -2 = fails
    closed; per user ``speed [C, M]`` float64 -- the greatest ego speed at a hit over the brake starts walked, 0.0 without a hit --,
    ``at [C, M]`` int32 the first brake start that attains it, -1 = none, and ``commit``, ``first [C, M]`` int32 as in
    :class:`HiddenBrakeVerdict`.  ``rows`` (host float64 ``[C, 4]``) and ``speed_of`` (host ``[C]``) the harm rows and speeds of the
    users, ``kinds`` their ``(type_name, length, width)``, ``harm_limit`` the bound above which a candidate lost its safety flag;
    ``poses``, ``starts``, ``users``, ``map_of``, ``thr``, ``clearances`` as in :class:`HiddenBrakeVerdict`.

    With ``approach="lanes"`` (DESIGN.md §5.10 "Impact verdict by approach angle") ``speed`` is None and the per-user pair is
    ``closing [C, M]`` float64 -- the greatest closing speed over the brake starts walked, every lane-bound user at the worst angle
    the lanes allow where it meets the ego, 0.0 without a hit -- and ``cosine [C, M]`` float64, the approach cosine at ``at``
    (1.0 = head-on, and without a hit); ``at`` is then the first start that attains ``closing``.  ``approach`` and
    ``heading_slack`` are the call's; with ``"head_on"`` ``closing`` and ``cosine`` are None.

    Not claimed: the bound is worst-area for every user and head-on for every user that is not lane-bound (with ``"head_on"``: for
    every user; ``approach="lanes"`` prices lane-bound users by their approach angle); a standing ego that is reached carries no
    harm; brake starts beyond ``starts`` are not looked at; this is harm, not risk -- there is no collision probability in it."""
    harm: torch.Tensor
    user: torch.Tensor
    speed: torch.Tensor
    at: torch.Tensor
    commit: torch.Tensor
    first: torch.Tensor
    rows: np.ndarray
    speed_of: np.ndarray
    kinds: tuple
    harm_limit: float
    poses: Optional[HiddenPoses] = None
    starts: int = 0
    users: tuple = ()
    map_of: tuple = ()
    thr: Optional[np.ndarray] = None
    clearances: tuple = ()
    closing: Optional[torch.Tensor] = None
    cosine: Optional[torch.Tensor] = None
    approach: str = "head_on"
    heading_slack: float = 0.0

    def obstacle_harm(self):
        """``[M]`` float64: what the cost row holds in its first reserved column"""
        return self.harm[:, 0]

    def ego_harm(self):
        """``[M]`` float64: the ego's harm against the same user at the same speed"""
        return self.harm[:, 1]

    def critical_user(self):
        """``[M]`` int64: the user whose obstacle harm is greatest, -1 = no user hits, -2 where the candidate has a non-finite pose"""
        return self.user.to(torch.int64)

    def impact_speed(self, user=None):
        """``[M]`` float64 (m/s): the ego speed at the hit against ``user`` -- against the chosen user by default, 0.0 where there is
        none.  Torch ops on the tensors' device, nothing is read back.  With ``approach="lanes"`` the ego speed at the hit is no
        output: :meth:`closing_speed` is what is priced."""
        if self.speed is None:
            raise ValueError("impact_speed: with approach=\"lanes\" the ego speed at the hit is not an output; .closing_speed() is "
                             "the speed that is priced and .approach_cosine() its angle")
        return self._picked(self.speed, user, 0.0)

    def _picked(self, per_user, user, none):
        if user is not None:
            return per_user[user]
        u = self.user.to(torch.int64)
        picked = per_user.gather(0, u.clamp(min=0).unsqueeze(0))[0]
        return torch.where(u >= 0, picked, torch.full_like(picked, none))

    def closing_speed(self, user=None):
        """``[M]`` float64 (m/s): the closing speed that is priced against ``user`` -- against the chosen user by default, 0.0 where
        there is none.  With ``approach="head_on"`` it is ``speed + speed_of``."""
        if self.closing is not None:
            return self._picked(self.closing, user, 0.0)
        w = torch.where(self.at >= 0, self.speed + torch.as_tensor(self.speed_of, device=self.speed.device).unsqueeze(1),
                        torch.zeros_like(self.speed))
        return self._picked(w, user, 0.0)

    def approach_cosine(self, user=None):
        """``[M]`` float64: the cosine of the reference's principal direction of force the closing speed was formed with, 1.0 =
        head-on (and where there is no hit)"""
        return self._picked(torch.ones_like(self.speed) if self.cosine is None else self.cosine, user, 1.0)

    def harm_of(self, c):
        """``[M, 2]`` float64: (obstacle harm, ego harm) of user ``c`` from ``speed[c]`` by the same row, (0, 0) where it has no hit;
        elementwise torch ops on the device (not a hot path; ``exp`` is torch's, the last bits may differ from ``harm``)"""
        p = self.rows[c]
        w = self.closing[c] if self.closing is not None else self.speed[c] + float(self.speed_of[c])
        both = torch.stack((1.0 / (1.0 + torch.exp(p[0] + p[1] * w)), 1.0 / (1.0 + torch.exp(p[2] + p[3] * w))), dim=1)
        return torch.where((self.at[c] >= 0).unsqueeze(1), both, torch.zeros_like(both))


def _harm_limit(harm_limit, fn):
    try:
        harm_limit = float(harm_limit)
    except (TypeError, ValueError):
        harm_limit = float("nan")
    if not harm_limit >= 0.0:
        raise ValueError(f"{fn}: harm_limit >= 0 (inf is possible, nan is not)")
    return harm_limit


def _impact_kinds(kinds, users, fn):
    """``kinds`` as a tuple of ``(type_name, length, width)``, one per user, or its refusal"""
    try:
        kinds = tuple((str(k[0]), float(k[1]), float(k[2])) for k in kinds)
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"{fn}: kinds must hold one (type_name, length, width) per user") from None
    if len(kinds) != len(users):
        raise ValueError(f"{fn}: {len(kinds)} kinds for {len(users)} users: one (type_name, length, width) per user")
    return kinds


def _impact_rows(self, users, kinds, ego_mass, coeff, fn):
    """``(rows, speed_of, d_rows, d_speed_of)``: the harm rows of :func:`hidden_impact_rows` and the users' speeds, on the host and
    on the model's device -- built once per distinct ``(users, kinds, ego_mass, coeff)`` and kept: after the first call nothing is
    uploaded"""
    from .metrics.metric import load_harm_coeff
    coeff = load_harm_coeff() if coeff is None else dict(coeff)
    try:
        key = (tuple(s for s, _, _ in users), kinds, float(ego_mass), tuple(sorted((str(k), float(q)) for k, q in coeff.items())))
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: ego_mass and the entries of coeff must be numbers") from None
    cache = self.__dict__.setdefault("_hbi_rows", {})
    if key not in cache:
        rows = hidden_impact_rows(kinds, ego_mass, coeff, fn)
        speed_of = np.array(key[0], dtype=np.float64)
        if len(cache) >= 16:
            cache.clear()
        cache[key] = (rows, speed_of, N.on_device(rows, self.device), N.on_device(speed_of, self.device))
    return cache[key]


def hidden_brake_impact(self, x, y, theta, v, *, vehicle, ego_mass, users, kinds, dt, a_brake, starts, harm_limit, coeff=None, cost=None,
                        safe=None, margin=None, inflate=0.0, lengths=None, poses=None, approach="head_on", heading_slack=0.0):
    """Hidden-traffic impact verdict (``fo_scene_hidden_brake_impact``; DESIGN.md §5.10 "Impact verdict"): for the hidden road
    ``users`` of :meth:`hidden_brake_users`, of the ``kinds`` ``(type_name, length, width)`` -- one per user --, over the first
    ``starts`` brake starts alone (an integer in ``[1, T]``, None = T: what a planner executes before it replans), the worst harm
    that remains after braking at ``a_brake``: the reference's MAIS3+ probability at the speed the ego of ``ego_mass`` kg has left
    where a manoeuvre is hit, head-on and at the worst area of impact -- and, with ``cost [M, 16]`` float64 / ``safe [M]`` uint8 of a
    sweep or planning step over the SAME candidates (both or neither), the obstacle's harm and the user in the two reserved cost
    columns, and ``safe = 0`` where that harm exceeds ``harm_limit`` (``>= 0``, ``inf`` allowed).  The stage only ever takes safety
    away.  It owns the same two columns as :meth:`hidden_brake_verdict` and :meth:`hidden_brake_ladder_verdict`: fold one of the
    three into a row.  ``coeff``: the entries of harm_params.json (None: the package's).

    ``approach="lanes"`` (``fo_scene_hidden_brake_impact_lanes``; DESIGN.md §5.10 "Impact verdict by approach angle") prices every
    user with ``flow == "lanes"`` at the worst closing speed the lanes' driving directions allow at the cells where it meets the
    ego -- ``dv = sqrt(v_ego^2 + v_user^2 + 2 v_ego v_user cos(pdof))`` at the greatest ``cos(pdof)`` over the headings within
    22.5 degrees + ``heading_slack`` (radians, ``>= 0``; what a lane change or a swerve may add) of a direction the move table
    leaves -- and every other user head-on as before; the result is never above the default's.  It needs the map's move table
    (``lane_moves``) where a user is lane-bound.  ``"head_on"``, the default, is the call as it always was.

    Everything runs on the device and on the current stream: the pose preparation (:meth:`hidden_poses`; ``poses=`` an earlier
    :class:`HiddenPoses` of the same candidates skips it, ``theta`` may then be None), one ``hidden_clearance`` per distinct
    ``(metric, flow)`` on the device headings, and ONE launch for the walk, the harm and the fold.  The harm rows are built once per
    distinct ``(users, kinds, ego_mass, coeff)`` and kept on the device: after the first call nothing is uploaded.  Nothing is read
    back and nobody waits; returns a :class:`HiddenBrakeImpact`."""
    fn = "hidden_brake_impact"
    users = _road_users(users, x, fn)
    if approach not in ("head_on", "lanes"):
        raise ValueError(f"{fn}: approach = {approach!r}: 'head_on' or 'lanes'")
    try:
        heading_slack = float(heading_slack)
    except (TypeError, ValueError):
        heading_slack = float("nan")
    if not (heading_slack >= 0.0 and math.isfinite(heading_slack)):
        raise ValueError(f"{fn}: heading_slack must be a finite angle >= 0 in radians")
    dir_mask = sum(1 << c for c, u in enumerate(users) if u[2] == "lanes") if approach == "lanes" else 0
    if dir_mask and getattr(self, "lane_moves", None) is None:
        raise ValueError(f"{fn}: approach='lanes' with a lane-bound user needs the map's move table (lane_moves is None)")
    kinds = _impact_kinds(kinds, users, fn)
    harm_limit = _harm_limit(harm_limit, fn)
    rows, speed_of, d_rows, d_speed_of = _impact_rows(self, users, kinds, ego_mass, coeff, fn)
    if poses is None:
        poses = hidden_poses(self, x, y, theta, v, lengths)
    p = _users_call(self, fn, users, x, y, None, v, vehicle=vehicle, dt=dt, margin=margin, inflate=inflate, lengths=lengths, poses=poses)
    a_brake = _a_brake(a_brake, fn)
    B = _ladder_starts(starts, p.T, fn)
    dev, M, C_ = self.device, p.M, len(users)
    _cost_safe(cost, safe, M, p.x.device, fn)
    tv = N.on_device(v, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    user, at, commit, first = new(M), new(C_, M), new(C_, M), new(C_, M)
    harm = torch.empty((M, 2), dtype=torch.float64, device=dev)
    speed = torch.empty((C_, M), dtype=torch.float64, device=dev)
    common = dict(**p.fields(tv, poses.arc, dt), a_brake=a_brake, B=B, d_speed_of=N.ptr(d_speed_of), d_harm_rows=N.ptr(d_rows),
                  harm_limit=harm_limit, d_finite_or_null=N.ptr(poses.finite), d_cost_or_null=N.ptr(cost), d_safe_or_null=N.ptr(safe),
                  d_harm=N.ptr(harm), d_user=N.ptr(user), d_at=N.ptr(at), d_commit=N.ptr(commit), d_first=N.ptr(first))
    closing = cosine = None
    if approach == "lanes":
        closing, cosine, speed = speed, torch.empty((C_, M), dtype=torch.float64, device=dev), None
        h = math.pi / 8.0 + heading_slack
        cos_h, sin_h = (math.cos(h), math.sin(h)) if h < math.pi else (-1.0, 0.0)      # (cos_h = -1: every user is head-on)
        args = N.HiddenBrakeImpactLanes(**common, d_closing=N.ptr(closing), d_cosine=N.ptr(cosine), dir_mask=dir_mask, cos_h=cos_h,
                                        sin_h=sin_h)
        self.ctx.call("fo_scene_hidden_brake_impact_lanes", C.byref(args), N.current_stream(self._dev_index))
    else:
        args = N.HiddenBrakeImpact(**common, d_speed=N.ptr(speed))
        self.ctx.call("fo_scene_hidden_brake_impact", C.byref(args), N.current_stream(self._dev_index))
    # (stay referenced until the next call, as in hidden_brake_users)
    self._hbi_inputs = (tv, poses, p.clearances, cost, safe)
    self._hbi_args = args                                   # (the structure of the last call: tools/hidden_reach_bench.py replays the launch alone)
    return HiddenBrakeImpact(harm, user, speed, at, commit, first, rows, speed_of, kinds, harm_limit, poses, B, users, p.map_of, p.thr,
                             p.clearances, closing, cosine, approach, heading_slack)


@dataclass
class HiddenBrakeHarmLadder:
    """what :meth:`SensorModel.hidden_brake_harm_ladder` returns (DESIGN.md §5.10 "Harm ladder"; device tensors): the seven tensors
    of :class:`HiddenBrakeLadderVerdict` -- ``need``, ``at``, ``blocking``, ``user [M]`` int32, ``decel [M]`` float64, ``need_of``,
    ``first [C, M]`` int32 -- with "unclear" read as "hit at an obstacle harm above ``harm_limit``": ``decel`` is the gentlest
    deceleration of ``levels`` that keeps the harm of every hit within the limit from the WORST of the first ``starts`` brake starts,
    ``+inf`` where no level does (``need == L``), 0.0 where nothing was asked; ``user`` the lowest user that keeps the worst start
    from the next gentler level, -2 = the candidate has a non-finite pose and fails closed.  And the curve: ``harm_at [M, L]``
    float64, the greatest obstacle harm (the reference's MAIS3+ probability, head-on and at the worst area of impact) that is left
    at level ``l`` over the starts and users, 0.0 without a hit, 1.0 where the candidate fails closed; ``user_at [M, L]`` int32 the
    lowest user that attains it, -1 = none, -2 = fails closed.  ``rows``, ``speed_of``, ``kinds``, ``harm_limit`` as in
    :class:`HiddenBrakeImpact`; ``levels``, ``starts``, ``a_limit``, ``poses``, ``users``, ``map_of``, ``thr``, ``clearances`` as in
    :class:`HiddenBrakeLadderVerdict`.

    What :meth:`SensorModel.hidden_brake_harm_ladder_lanes` returns has ``approach == "lanes"`` and its ``heading_slack``: every
    user with ``flow == "lanes"`` is priced at the approach angle the lanes allow, and nothing is above the head-on call's.

    Not claimed: what the two siblings do not claim; with ``approach == "head_on"`` every user is priced head-on
    (:meth:`SensorModel.hidden_brake_harm_ladder_lanes` prices lane-bound users by their approach angle); the answer is only as
    fine as the ladder; harder braking is not always safer, so ``harm_at`` need not fall along ``l``."""
    need: torch.Tensor
    at: torch.Tensor
    blocking: torch.Tensor
    user: torch.Tensor
    decel: torch.Tensor
    need_of: torch.Tensor
    first: torch.Tensor
    harm_at: torch.Tensor
    user_at: torch.Tensor
    levels: np.ndarray
    starts: int
    harm_limit: float
    a_limit: float
    rows: np.ndarray
    speed_of: np.ndarray
    kinds: tuple = ()
    users: tuple = ()
    poses: Optional[HiddenPoses] = None
    map_of: tuple = ()
    thr: Optional[np.ndarray] = None
    clearances: tuple = ()
    approach: str = "head_on"
    heading_slack: float = 0.0

    def required_deceleration(self):
        """``[M]`` float64 (m/s^2): ``decel`` -- what the cost row holds in its first reserved column"""
        return self.decel

    def brake_threat_number(self, a_max):
        """``[M]`` float64: ``decel / a_max`` -- the reference's ``break_threat_number`` (metrics/be.py:56) against the hidden road
        users, with "no collision" relaxed to "harm within ``harm_limit``".  Nothing is read back."""
        return self.decel / float(a_max)

    def critical_user(self):
        """``[M]`` int64: the lowest user that keeps the worst brake start from the next gentler level, -1 = none, -2 where the
        candidate has a non-finite pose.  Nothing is read back."""
        return self.user.to(torch.int64)

    def harm_curve(self):
        """``(levels, harm_at, user_at)``: the ladder (host float64 ``[L]``) and what each of its levels leaves, ``[M, L]`` each"""
        return self.levels, self.harm_at, self.user_at

    def monotone(self):
        """``[M]`` bool: ``harm_at`` never rises from a level to the next harder one -- where harder braking is never worse, and a
        bisection over the deceleration would have been sound.  Nothing is read back."""
        if self.harm_at.shape[1] < 2:
            return torch.ones((self.harm_at.shape[0],), dtype=torch.bool, device=self.harm_at.device)
        return (self.harm_at[:, 1:] <= self.harm_at[:, :-1]).all(dim=1)


def hidden_brake_harm_ladder(self, x, y, theta, v, *, vehicle, ego_mass, users, kinds, dt, levels=None, starts, harm_limit,
                             a_limit=float("inf"), coeff=None, cost=None, safe=None, margin=None, inflate=0.0, lengths=None, poses=None):
    """Hidden-traffic harm ladder (``fo_scene_hidden_brake_harm_ladder``; DESIGN.md §5.10 "Harm ladder"): for the hidden road
    ``users`` of :meth:`hidden_brake_users`, of the ``kinds`` of :meth:`hidden_brake_impact`, and the ladder ``levels`` of
    :meth:`hidden_brake_ladder_verdict` (None: 0.5, 1.0, ... up to ``a_limit``, which must then be finite), over the first ``starts``
    brake starts alone, the gentlest deceleration of the ladder at which the obstacle harm of every hit that remains -- the
    reference's MAIS3+ probability at the speed the ego of ``ego_mass`` kg has left where it is hit, head-on and at the worst area of
    impact -- stays within ``harm_limit`` (``>= 0``, ``inf`` allowed) from the WORST of those starts; and per level the greatest
    harm it leaves.  ``harm_limit = 0`` is the ladder verdict.  With ``cost [M, 16]`` float64 / ``safe [M]`` uint8 of a sweep or
    planning step over the SAME candidates (both or neither) that deceleration and the blocking user go into the two reserved cost
    columns, and ``safe = 0`` where no level suffices or the deceleration exceeds ``a_limit``.  The stage only ever takes safety
    away.  It owns the same two columns as :meth:`hidden_brake_verdict`, :meth:`hidden_brake_ladder_verdict` and
    :meth:`hidden_brake_impact`: fold one of the four into a row.

    Everything runs on the device and on the current stream: the pose preparation (``poses=`` skips it), one ``hidden_clearance``
    per distinct ``(metric, flow)``, and ONE launch for the walk, the harms, the reduction and the fold.  The harm rows are the
    impact verdict's, built once and kept on the device.  Nothing is read back and nobody waits; returns a
    :class:`HiddenBrakeHarmLadder`."""
    return _harm_ladder_call(self, "hidden_brake_harm_ladder", None, x, y, theta, v, vehicle=vehicle, ego_mass=ego_mass, users=users,
                             kinds=kinds, dt=dt, levels=levels, starts=starts, harm_limit=harm_limit, a_limit=a_limit, coeff=coeff,
                             cost=cost, safe=safe, margin=margin, inflate=inflate, lengths=lengths, poses=poses)


def hidden_brake_harm_ladder_lanes(self, x, y, theta, v, *, vehicle, ego_mass, users, kinds, dt, levels=None, starts, harm_limit,
                                   a_limit=float("inf"), coeff=None, cost=None, safe=None, margin=None, inflate=0.0, lengths=None,
                                   poses=None, heading_slack=0.0):
    """Hidden-traffic harm ladder by approach angle (``fo_scene_hidden_brake_harm_ladder_lanes``; DESIGN.md §5.10 "Harm ladder by
    approach angle"): :meth:`hidden_brake_harm_ladder` with every user with ``flow == "lanes"`` priced at the worst closing speed the
    lanes' driving directions allow at the cells where it meets the ego -- ``dv = sqrt(v_ego^2 + v_user^2 + 2 v_ego v_user
    cos(pdof))`` at the greatest ``cos(pdof)`` over the headings within 22.5 degrees + ``heading_slack`` (radians, ``>= 0``) of a
    direction the move table leaves, as ``hidden_brake_impact(approach="lanes")`` prices it -- and every other user head-on as
    before.  ``decel`` and ``harm_at`` are never above the head-on call's; without a lane-bound user, or with ``heading_slack`` at
    or above 7 pi / 8, every output is that call's bit for bit.  It needs the map's move table (``lane_moves``) where a user is
    lane-bound.  One launch, the same arguments, the same two reserved columns: fold one of the five stages into a row.  Returns a
    :class:`HiddenBrakeHarmLadder` with ``approach == "lanes"``."""
    return _harm_ladder_call(self, "hidden_brake_harm_ladder_lanes", heading_slack, x, y, theta, v, vehicle=vehicle, ego_mass=ego_mass,
                             users=users, kinds=kinds, dt=dt, levels=levels, starts=starts, harm_limit=harm_limit, a_limit=a_limit,
                             coeff=coeff, cost=cost, safe=safe, margin=margin, inflate=inflate, lengths=lengths, poses=poses)


def _harm_ladder_call(self, fn, heading_slack, x, y, theta, v, *, vehicle, ego_mass, users, kinds, dt, levels, starts, harm_limit, a_limit,
                      coeff, cost, safe, margin, inflate, lengths, poses):
    """the ONE body of :func:`hidden_brake_harm_ladder` (``heading_slack is None``: head-on) and
    :func:`hidden_brake_harm_ladder_lanes`: one set of checks, one set of buffers, the entry by the form"""
    lanes = heading_slack is not None
    users = _road_users(users, x, fn)
    dir_mask = 0
    if lanes:
        try:
            heading_slack = float(heading_slack)
        except (TypeError, ValueError):
            heading_slack = float("nan")
        if not (heading_slack >= 0.0 and math.isfinite(heading_slack)):
            raise ValueError(f"{fn}: heading_slack must be a finite angle >= 0 in radians")
        dir_mask = sum(1 << c for c, u in enumerate(users) if u[2] == "lanes")
        if dir_mask and getattr(self, "lane_moves", None) is None:
            raise ValueError(f"{fn}: a lane-bound user needs the map's move table (lane_moves is None)")
    try:
        a_limit = float(a_limit)
    except (TypeError, ValueError):
        a_limit = float("nan")
    if not a_limit >= 0.0:
        raise ValueError(f"{fn}: a_limit >= 0 (inf is possible, nan is not)")
    if levels is None:
        if not math.isfinite(a_limit):
            raise ValueError(f"{fn}: the default levels run up to a_limit, which is not finite: hand levels over")
        levels = default_brake_ladder(a_limit, fn)
    levels = _ladder_levels(levels, fn)
    _arg_bytes(users, x, levels, "levels", fn)
    kinds = _impact_kinds(kinds, users, fn)
    harm_limit = _harm_limit(harm_limit, fn)
    rows, speed_of, d_rows, d_speed_of = _impact_rows(self, users, kinds, ego_mass, coeff, fn)
    if poses is None:
        poses = hidden_poses(self, x, y, theta, v, lengths)
    p = _users_call(self, fn, users, x, y, None, v, vehicle=vehicle, dt=dt, margin=margin, inflate=inflate, lengths=lengths, poses=poses)
    B = _ladder_starts(starts, p.T, fn)
    dev, M, C_, L_ = self.device, p.M, len(users), len(levels)
    _cost_safe(cost, safe, M, p.x.device, fn)
    tv = N.on_device(v, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    need, at, blocking, user, need_of, first, user_at = new(M), new(M), new(M), new(M), new(C_, M), new(C_, M), new(M, L_)
    decel = torch.empty((M,), dtype=torch.float64, device=dev)
    harm_at = torch.empty((M, L_), dtype=torch.float64, device=dev)
    common = dict(**p.fields(tv, poses.arc, dt), h_levels=levels.ctypes.data_as(C.POINTER(C.c_double)), L=L_, B=B, a_limit=a_limit,
                  d_finite_or_null=N.ptr(poses.finite), d_cost_or_null=N.ptr(cost), d_safe_or_null=N.ptr(safe), d_need=N.ptr(need),
                  d_at=N.ptr(at), d_blocking=N.ptr(blocking), d_user=N.ptr(user), d_decel=N.ptr(decel), d_need_of=N.ptr(need_of),
                  d_first=N.ptr(first), d_speed_of=N.ptr(d_speed_of), d_harm_rows=N.ptr(d_rows), harm_limit=harm_limit,
                  d_harm_at=N.ptr(harm_at), d_user_at=N.ptr(user_at))
    if lanes:
        h = math.pi / 8.0 + heading_slack
        cos_h, sin_h = (math.cos(h), math.sin(h)) if h < math.pi else (-1.0, 0.0)      # (cos_h = -1: every user is head-on)
        args = N.HiddenBrakeHarmLadderLanes(**common, dir_mask=dir_mask, cos_h=cos_h, sin_h=sin_h)
        self.ctx.call("fo_scene_hidden_brake_harm_ladder_lanes", C.byref(args), N.current_stream(self._dev_index))
    else:
        args = N.HiddenBrakeHarmLadder(**common)
        self.ctx.call("fo_scene_hidden_brake_harm_ladder", C.byref(args), N.current_stream(self._dev_index))
    # (stay referenced until the next call, as in hidden_brake_users)
    self._hbhl_inputs = (tv, poses, p.clearances, cost, safe)
    self._hbhl_args = args                                  # (the structure of the last call: tools/hidden_reach_bench.py replays the launch alone)
    return HiddenBrakeHarmLadder(need, at, blocking, user, decel, need_of, first, harm_at, user_at, levels, B, harm_limit, a_limit, rows,
                                 speed_of, kinds, users, poses, p.map_of, p.thr, p.clearances, "lanes" if lanes else "head_on",
                                 heading_slack if lanes else 0.0)
