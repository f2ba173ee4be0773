"""Throughput of the future-visibility extension at the BASELINE configs[2] size (10 000 trajectories, city grid):
HIP-event time of fo_scene_future_visibility for a few (stride, rays) settings, or with --ex of the extended entry
fo_scene_future_visibility_ex in the configuration the flags ask for.  Run on the GPU box.

    future_visibility_bench.py [M]                                     the old entry, (stride, rays) table
    future_visibility_bench.py [M] --ex [--slices S] [--fov DEG] [--first-seen] [--rays N] [--stride K] [--calls C]
        --slices S   S moving occluder slices (the parked cars shifted per pose); 1 = the obstacles of the step
        --fov DEG    an open fan of DEG degrees about each pose's heading (360 = world-aligned full circle)
        --first-seen the first-seen outputs (a workgroup per trajectory)
    prints the median of C calls (HIP events around each) and, with --old, the old entry measured the same way."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "frenetix-occlusion_amd"))
from frenetix_occlusion import scenario as SC, synthetic as SY  # noqa: E402
from frenetix_occlusion.sensor_model import SensorModel  # noqa: E402


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
    ap.add_argument("--ex", action="store_true")
    ap.add_argument("--old", action="store_true", help="also time the old entry at the same rays / stride")
    ap.add_argument("--slices", type=int, default=1)
    ap.add_argument("--fov", type=float, default=360.0)
    ap.add_argument("--first-seen", action="store_true")
    ap.add_argument("--rays", type=int, default=720)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--calls", type=int, default=25)
    a = ap.parse_args()
    sc = SC.synthetic_urban_grid()
    ego = sc.ego_initial
    sm = SensorModel(sc.lanelets, None, sensor_radius=50.0, sensor_angle=360.0)
    corn0, cen0, flags0 = sc.obstacle_arrays(0)[:3]
    sm.upload_obstacles((corn0, cen0, flags0))
    sm.launch(ego[:2], float(ego[2]))
    M = a.M
    traj = SY.make_trajectories(M, 31, 0.1, seed=20240134, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    dev = sm.device
    tx, ty = torch.as_tensor(traj["x"]).to(dev), torch.as_tensor(traj["y"]).to(dev)
    n_occ = int(sm.n_occluded.item())
    if not a.ex:
        for stride, rays in ((5, 192), (5, 720), (10, 192), (5, 96), (5, 256), (5, 384), (1, 192)):
            ms = _median_ms(lambda: sm.future_visibility(tx, ty, t_stride=stride, n_rays=rays), 5)
            rev, _ = sm.future_visibility(tx, ty, t_stride=stride, n_rays=rays)
            K = (31 + stride - 1) // stride
            print(f"M={M} stride={stride} (K={K}) rays={rays}: {ms:8.3f} ms  = {M * K * rays / ms / 1e6:6.2f} Grays/s, "
                  f"{M * K / ms / 1e3:6.2f} Mposes/s; occluded cells {n_occ}; mean revealed at last pose "
                  f"{float(rev[:, -1].double().mean()):.1f}")
        return
    K = (31 + a.stride - 1) // a.stride
    occ = None
    if a.slices > 1:
        rng = np.random.default_rng(3)
        shift = rng.uniform(-2.0, 2.0, size=(a.slices, len(flags0), 1, 2))
        shift[0] = 0.0
        corn = corn0[None] + np.cumsum(shift, axis=0)
        occ = (torch.as_tensor(corn).to(dev), torch.as_tensor(np.repeat(flags0[None], a.slices, axis=0)).to(dev))
    theta = torch.as_tensor(traj["theta"]).to(dev) if a.fov < 359.9 else None
    run = lambda: sm.future_visibility_ex(tx, ty, theta, t_stride=a.stride, n_rays=a.rays, fov=a.fov, occluders=occ,
                                          first_seen=a.first_seen)
    ms = _median_ms(run, a.calls)
    out = run()
    torch.cuda.synchronize()
    tag = f"ex slices={a.slices} fov={a.fov:g} first_seen={int(a.first_seen)}"
    extra = f"; mean revealed_any {float(out.revealed_any.double().mean()):.1f}" if a.first_seen else ""
    print(f"M={M} K={K} rays={a.rays} {tag}: median {ms:8.3f} ms over {a.calls} calls{extra}; occluded cells {n_occ}")
    if a.old:
        ms0 = _median_ms(lambda: sm.future_visibility(tx, ty, t_stride=a.stride, n_rays=a.rays), a.calls)
        print(f"M={M} K={K} rays={a.rays} old entry: median {ms0:8.3f} ms over {a.calls} calls")


if __name__ == "__main__":
    main()
