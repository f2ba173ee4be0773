"""Future visibility (an extension): how much of the currently occluded area each candidate trajectory will come to
see.  The two entries are :class:`~frenetix_occlusion.sensor_model.SensorModel`'s methods of the same names (``self``)."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native as N


@dataclass
class FutureVisibility:
    """what :meth:`SensorModel.future_visibility_ex` returns (device tensors, K = ceil(T / t_stride) poses):
    ``revealed [M, K]`` int32 and ``area [M, K]`` float64 as for ``future_visibility``; ``revealed_new [M, K]`` int32
    (cells a pose sees that no earlier pose of its trajectory saw) and ``revealed_any [M]`` int32 (their row sum: distinct
    cells the trajectory reveals), None unless asked for; ``slice_timesteps``: the time step each occluder slice stands
    for (None when the caller handed in slices of its own)."""
    revealed: torch.Tensor
    area: torch.Tensor
    revealed_new: Optional[torch.Tensor] = None
    revealed_any: Optional[torch.Tensor] = None
    slice_timesteps: Optional[list] = None


def _fan_table(self, name, key, n_rays, fov_deg, r):
    """the world-aligned fan directions [n_rays, 2] on the device, kept on the model as ``name`` for as long as ``key`` stays"""
    if getattr(self, name + "_key", None) != key:
        dirs = torch.empty((n_rays, 2), dtype=torch.float64, device=self.device)
        self.ctx.call("fo_scene_fan", n_rays, 0.0, fov_deg, r, 0, dirs.data_ptr(), None, None, N.current_stream(self._dev_index))
        setattr(self, name, dirs)
        setattr(self, name + "_key", key)
    return getattr(self, name)


def future_visibility(self, x, y, t_stride=5, n_rays=192, radius=None):
    """How much of the currently occluded area each candidate trajectory will come to see.

    x, y: [M, T] trajectory samples (numpy or device tensors).  From every ``t_stride``-th sample a world-aligned
    full fan of ``n_rays`` rays (<= 768) of length ``radius`` (default: the sensor radius) is cast against the
    static map and the obstacles of the last ``upload_obstacles``; returns device tensors
    ``revealed [M, K]`` (int32: cells of the occluded set of the last ``launch`` that lie inside that fan) and
    ``area [M, K]`` (float64: area of the polygon of hit points), K = ceil(T / t_stride).  Queued on the current
    stream, no host synchronisation.  Uses the plain chord rule of the ray fan (no exact settlement, no
    enclosed-hole or footprint-polygon refinements): it is a cost term, not a reproduction of reference output."""
    if self.window is None:
        raise RuntimeError("future_visibility needs the occluded set of a previous launch()")
    dev = self.device
    tx, ty = N.on_device(x, dev), N.on_device(y, dev)
    M, T = tx.shape
    K = (T + t_stride - 1) // t_stride
    r = float(self.sensor_radius if radius is None else radius)
    key = int(n_rays)
    dirs = _fan_table(self, "_fv_dirs", key, key, 360.0, r)
    revealed = torch.empty((M, K), dtype=torch.int32, device=dev)
    area = torch.empty((M, K), dtype=torch.float64, device=dev)
    d_corn, _, d_flags, O = getattr(self, "_obst", (None, None, None, 0))
    w = self.window
    self.ctx.call("fo_scene_future_visibility", M, T, tx.data_ptr(), ty.data_ptr(), int(t_stride), key,
                  dirs.data_ptr(), r, O, N.ptr(d_corn), N.ptr(d_flags), self.occluded_idx_buffer.data_ptr(),
                  self.n_occluded.data_ptr(), w.ix0, w.iy0, w.nx, revealed.data_ptr(), area.data_ptr(),
                  N.current_stream(self._dev_index))
    return revealed, area


def future_visibility_ex(self, x, y, theta=None, *, t_stride=5, n_rays=192, radius=None, fov="full", occluders=None,
                         first_seen=False):
    """Extended :meth:`future_visibility` (``fo_scene_future_visibility_ex``); returns a :class:`FutureVisibility`.
    Queued on the current stream, no host synchronisation.

    ``theta [M, T]``: headings of the samples; the fan of pose k is rotated by (cos, sin) of ``theta[:, k t_stride]``
    (numpy's for host arrays, torch's on the device for device tensors; None: world-aligned).  ``fov``: ``"full"`` or degrees; below 359.9 an open fan of ``n_rays`` rays from -fov/2 to
    +fov/2 about the pose heading, which needs ``theta``.  ``occluders``: None = the obstacles of the last
    ``upload_obstacles`` (one slice, what ``future_visibility`` casts against), or ``(corners [S, O, 4, 2], flags [S, O])``
    -- pose k casts against slice min(k, S - 1) (flags bit 0 present, bit 1 occludes).  ``first_seen``: also the
    first-seen counts (a workgroup per trajectory; the window may hold at most
    ``_native.FUTURE_VISIBILITY_MAX_CELLS`` cells)."""
    if self.window is None:
        raise RuntimeError("future_visibility_ex needs the occluded set of a previous launch()")
    dev = self.device
    tx, ty = N.on_device(x, dev), N.on_device(y, dev)
    M, T = tx.shape
    K = (T + t_stride - 1) // t_stride
    r = float(self.sensor_radius if radius is None else radius)
    fov_deg = 360.0 if isinstance(fov, str) and fov == "full" else float(fov)
    if fov_deg >= 359.9:
        fov_deg = 360.0     # the full fan of future_visibility
    key = (int(n_rays), fov_deg)
    dirs = _fan_table(self, "_fvx_dirs", key, key[0], fov_deg, r)
    heading = None
    if theta is not None:     # [M, K, 2], computed once: on the host for host samples (a checker can redo them), else here
        if torch.is_tensor(theta):
            th = theta.to(dev, torch.float64)[:, ::t_stride]
            heading = torch.stack((torch.cos(th), torch.sin(th)), -1).contiguous()
        else:
            th = np.asarray(theta, dtype=np.float64)[:, ::t_stride]
            heading = N.on_device(np.stack((np.cos(th), np.sin(th)), -1), dev)
    if occluders is None:
        d_corn, _, d_flags, O = getattr(self, "_obst", (None, None, None, 0))
        S, slice_ts = 1, [getattr(self, "timestep", None)]
    else:
        corn, flags = occluders
        d_corn = N.on_device(corn, dev)
        d_flags = N.on_device(flags, dev, "uint8")
        if d_corn.dim() != 4 or d_corn.shape[2:] != (4, 2) or tuple(d_flags.shape) != tuple(d_corn.shape[:2]):
            raise ValueError("occluders: corners [S, O, 4, 2] and flags [S, O]")
        S, O, slice_ts = int(d_corn.shape[0]), int(d_corn.shape[1]), None
    revealed = torch.empty((M, K), dtype=torch.int32, device=dev)
    area = torch.empty((M, K), dtype=torch.float64, device=dev)
    new = torch.empty((M, K), dtype=torch.int32, device=dev) if first_seen else None
    any_ = torch.empty(M, dtype=torch.int32, device=dev) if first_seen else None
    w, p = self.window, N.ptr
    args = N.FutureVisibility(M=M, T=T, t_stride=int(t_stride), n_rays=key[0], d_x=tx.data_ptr(), d_y=ty.data_ptr(),
                              d_dirs=dirs.data_ptr(), r=r, fov_deg=fov_deg, d_heading=p(heading), O=O,
                              n_slices=S, d_ocorn=p(d_corn), d_oflags=p(d_flags),
                              d_occ_idx=self.occluded_idx_buffer.data_ptr(), d_n_occ=self.n_occluded.data_ptr(),
                              win_ix0=w.ix0, win_iy0=w.iy0, win_nx=w.nx, win_ny=w.ny, d_revealed=revealed.data_ptr(),
                              d_area=area.data_ptr(), d_revealed_new=p(new), d_revealed_any=p(any_))
    self.ctx.call("fo_scene_future_visibility_ex", C.byref(args), N.current_stream(self._dev_index))
    # (inputs made here stay referenced until the next call: the caching allocator may not hand them out earlier anyway,
    # they are freed in stream order)
    self._fvx_inputs = (tx, ty, heading, d_corn, d_flags)
    return FutureVisibility(revealed, area, new, any_, slice_ts)
