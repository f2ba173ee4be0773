"""Occlusion memory (an extension): the host plan of a step, and the device state of one sensor model."""
import ctypes as C
import math

import torch

from . import _native as N

OCCLUSION_MEMORY_METRICS = ("euclid", "road")


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
    while the memory is off) and the ping-pong buffers of the hidden set H."""

    def __init__(self, ctx, device):
        self.ctx, self.device = ctx, device
        self.buf, self.cur = None, 0       # the two buffers, index of the one the next step writes
        self.reset_reason = None
        self.configure(None, "euclid")

    def configure(self, plan, metric):
        """switch the memory on (a fresh :class:`OcclusionMemoryPlan`: the next step is a reset) or off (None)"""
        self.plan, self.metric = plan, metric
        self.prev_window, self.host = None, None      # window of the other buffer's H, its host copy
        if plan is None:
            self.buf = self.reset_reason = None

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
            self.prev_window = None
            plan.has_prev = False
        r2, reason = plan.next_step(timestep)
        cur, prev = self.buf[self.cur], self.buf[1 - self.cur]
        pw = self.prev_window
        m = N.OcclusionMemory(r2=r2, reset=1 if reason else 0, d_cur=cur.data_ptr(), cur_bytes=cur.numel())
        if reason is None:
            m.prev_ix0, m.prev_iy0, m.prev_nx, m.prev_ny = pw.ix0, pw.iy0, pw.nx, pw.ny
            m.d_prev, m.prev_bytes = prev.data_ptr(), prev.numel()
        arm = (self.ctx._lib.fo_scene_set_occlusion_memory_road if self.metric == "road"
               else self.ctx._lib.fo_scene_set_occlusion_memory)
        self.ctx._check(arm(self.ctx._h, C.byref(m)))

        def commit():
            plan.commit(timestep)
            self.prev_window, self.cur, self.host = w, 1 - self.cur, None
            self.reset_reason = reason
        return commit
