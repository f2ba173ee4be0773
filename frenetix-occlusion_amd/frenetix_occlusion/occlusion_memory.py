"""Occlusion memory (an extension): the host plan of a step, and the device state of one sensor model."""
import ctypes as C
import math

import torch

from . import _native as N

OCCLUSION_MEMORY_METRICS = ("euclid", "road")
OCCLUSION_MEMORY_VEHICLES = ("off", "lanes")     # "lanes": the vehicle layer V next to H (DESIGN.md §5.9 "Vehicle layer")


def occlusion_memory_r2(v_max, dt_s, margin, cell_size):
    """R2 = floor(rho^2 / cs^2), rho = v_max * dt_s + margin, in float64: the reach of the occlusion memory as a squared
    cell count, so that device and host model decide membership in D = {dx^2 + dy^2 <= R2} in integers"""
    rho = float(v_max) * float(dt_s) + float(margin)
    return int(math.floor((rho * rho) / (float(cell_size) * float(cell_size))))


class OcclusionMemoryPlan:
    """Host side of the occlusion memory, without device state: what the next step hands the device.

    :meth:`next_step` returns ``(r2, reason)``: ``reason`` None = a memory step with reach ``r2``; otherwise the step is a
    reset (the previous step's hidden set is replaced by the road raster) and ``reason`` says why -- ``"first"`` (no
    previous step), ``"explicit"`` (:meth:`reset`), ``"time"`` (the timestep did not increase, or no timestep was given) or
    ``"reach"`` (``sqrt(R2)`` beyond the kernel's halo, ``OCCLUSION_MEMORY_MAX_HALO`` cells).  :meth:`commit` records a step
    that ran; a step given no timestep leaves the recorded timestep as it was (the next step's Δt counts from the last one
    that had a timestep, a longer reach, never a shorter one)."""

    def __init__(self, v_max=13.9, margin=None, cell_size=0.5, dt=0.1, max_halo=None):
        self.v_max, self.cell_size, self.dt = float(v_max), float(cell_size), float(dt)
        self.margin = math.sqrt(2.0) * self.cell_size if margin is None else float(margin)
        if not (self.v_max >= 0.0 and self.margin >= 0.0 and self.cell_size > 0.0 and self.dt > 0.0):
            raise ValueError("occlusion memory: v_max >= 0, margin >= 0, cell_size > 0 and dt > 0")
        self.max_halo = N.OCCLUSION_MEMORY_MAX_HALO if max_halo is None else int(max_halo)
        self.timestep = None          # timestep of the last committed step that had one
        self.has_prev = False         # a previous step's hidden set exists
        self._explicit = False

    def reset(self):
        self._explicit = True

    def next_step(self, timestep):
        if self._explicit:
            return 0, "explicit"
        if not self.has_prev:
            return 0, "first"
        if timestep is None or self.timestep is None or int(timestep) <= int(self.timestep):
            return 0, "time"
        r2 = occlusion_memory_r2(self.v_max, (int(timestep) - int(self.timestep)) * self.dt, self.margin, self.cell_size)
        if r2 > self.max_halo * self.max_halo:
            return 0, "reach"
        return r2, None

    def commit(self, timestep):
        self._explicit = False
        self.has_prev = True
        if timestep is not None:
            self.timestep = int(timestep)


class OcclusionMemory:
    """Device state of one :class:`~frenetix_occlusion.sensor_model.SensorModel`'s occlusion memory: the host plan (None
    while the memory is off) and the ping-pong buffers of the hidden set H; with ``vehicles == "lanes"`` a second pair for the
    vehicle layer V (DESIGN.md §5.9 "Vehicle layer"), armed and committed with H under the one plan: the same ``r2``, the same
    reset reasons."""

    def __init__(self, ctx, device):
        self.ctx, self.device = ctx, device
        self.buf, self.cur = None, 0       # the two buffers, index of the one the next step writes
        self.vbuf = None                   # the vehicle layer's pair (the same index), allocated only when it is on
        self.reset_reason = None
        self.configure(None, "euclid")

    def configure(self, plan, metric, vehicles="off"):
        """switch the memory on (a fresh :class:`OcclusionMemoryPlan`: the next step is a reset) or off (None)"""
        self.plan, self.metric = plan, metric
        self.vehicles = vehicles if plan is not None else "off"
        self.prev_window, self.host = None, None      # window of the other buffer's H, its host copy
        self.vprev_window, self.vhost = None, None    # the same for V
        if plan is None:
            self.buf = self.reset_reason = None
        if self.vehicles == "off":
            self.vbuf = None

    def hidden(self):
        """H of the last step (numpy uint8 [ny, nx] over its window: 1 = a hidden road user may be in the cell), read
        from the device when first looked at; None while the memory is off or before its first step"""
        if self.plan is None or self.prev_window is None:
            return None
        if self.host is None:
            w = self.prev_window
            self.host = self.buf[1 - self.cur][:w.nx * w.ny].view(w.ny, w.nx).cpu().numpy()
        return self.host

    def hidden_on_device(self, w):
        """this step's H_k on the device when the memory ran in the stage that produced the classes of window ``w``, else None"""
        return self.buf[1 - self.cur] if self.plan is not None and self.prev_window is w else None

    def hidden_vehicles(self):
        """V of the last step (numpy uint8 [ny, nx] over its window: 1 = a hidden lane-abiding vehicle may be in the cell), read
        from the device when first looked at; None while the vehicle layer is off or before its first step"""
        if self.plan is None or self.vehicles == "off" or self.vprev_window is None:
            return None
        if self.vhost is None:
            w = self.vprev_window
            self.vhost = self.vbuf[1 - self.cur][:w.nx * w.ny].view(w.ny, w.nx).cpu().numpy()
        return self.vhost

    def hidden_vehicles_on_device(self, w):
        """this step's V_k on the device when the vehicle layer ran in the stage that produced the classes of window ``w``, else None"""
        return self.vbuf[1 - self.cur] if self.plan is not None and self.vehicles != "off" and self.vprev_window is w else None

    def arm(self, w, timestep):
        """arm the context's next visibility stage (fo_scene_set_occlusion_memory, or its _road form); returns the commit to call once the
        stage has been queued, or None while the memory is off"""
        plan = self.plan
        if plan is None:
            return None
        cells = w.nx * w.ny
        if self.buf is None or self.buf[0].numel() < cells:
            if self.buf is not None:
                torch.cuda.current_stream(self.device).synchronize()   # (a step in flight may still read the old pair)
            self.buf = [torch.zeros(cells, dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.prev_window = self.vprev_window = None
            plan.has_prev = False
        lanes = self.vehicles == "lanes"
        if lanes and (self.vbuf is None or self.vbuf[0].numel() < self.buf[0].numel()):
            if self.vbuf is not None:
                torch.cuda.current_stream(self.device).synchronize()
            self.vbuf = [torch.zeros(self.buf[0].numel(), dtype=torch.uint8, device=self.device) for _ in range(2)]
            self.prev_window = self.vprev_window = None     # (both sets start over: one plan, one reason)
            plan.has_prev = False
        r2, reason = plan.next_step(timestep)

        def armed(pair, pw):      # the structure of one set: the buffer this step writes, the other one with its window
            cur, prev = pair[self.cur], pair[1 - self.cur]
            m = N.OcclusionMemory(r2=r2, reset=1 if reason else 0, d_cur=cur.data_ptr(), cur_bytes=cur.numel())
            if reason is None:
                m.prev_ix0, m.prev_iy0, m.prev_nx, m.prev_ny = pw.ix0, pw.iy0, pw.nx, pw.ny
                m.d_prev, m.prev_bytes = prev.data_ptr(), prev.numel()
            return C.byref(m)
        arm = (self.ctx._lib.fo_scene_set_occlusion_memory_road if self.metric == "road"
               else self.ctx._lib.fo_scene_set_occlusion_memory)
        self.ctx._check(arm(self.ctx._h, armed(self.buf, self.prev_window)))
        if lanes:                 # (after the main call: it rides on the main memory of the same stage)
            self.ctx._check(self.ctx._lib.fo_scene_set_occlusion_memory_vehicles(self.ctx._h, armed(self.vbuf, self.vprev_window)))

        def commit():
            plan.commit(timestep)
            self.prev_window, self.cur, self.host = w, 1 - self.cur, None
            self.vprev_window, self.vhost = (w if lanes else None), None
            self.reset_reason = reason
        return commit
