"""Writes tests/golden/brake_manoeuvre.npz: what the reference's own, unmodified ``BE._calc_deceleration_trajectory(traj,
break_time_step=b, deceleration=[a])`` (metrics/be.py:84-146) makes of straight trajectories -- the pin of the brake clearance's
re-sampling rule (DESIGN.md §5.10 "Brake clearance", tests/test_hidden_brake_cpu.py).

Run where the reference is present only (see gen_golden.py, whose loading of be.py -- ``gen_be`` -- and whose duck-typed harness
objects this script uses).  be.py runs as it stands: its speed profile, its running sum of ``v dt``, scipy's interp1d.

The inputs are DYADIC: ``dt = 0.25``, speeds that are multiples of 0.5 and constant over stretches, straight paths along an axis that
start on a multiple of 0.125, decelerations that are dyadic too.  Every ``v dt``, every partial sum of them and every chord length is
then exact in binary, ``cumsum(v dt)`` IS the travelled chord length, and the reference's running sum from 0 coincides exactly with
the sum the brake clearance starts at ``arc[b]``.  Speeds never fall along a trajectory, so no manoeuvre runs past the end of its
path (where the reference raises).  Cases that stop inside the horizon and cases that do not are both there."""
import os
import sys

import numpy as np

import gen_golden as G


def main():
    G._install_aliases()
    sys.path.insert(0, G.REF)
    sys.path.insert(0, os.path.dirname(os.path.dirname(G.OUT)))
    from oracle import fo_oracle as O
    O.build()
    G._install_rectangle_stub(O)
    from frenetix_occlusion.metrics.be import BE          # the reference's own class, unmodified

    dt, T = 0.25, 12
    profiles = [np.full(T, 8.0), np.full(T, 2.5), np.repeat([4.0, 6.0, 8.0], 4), np.repeat([1.0, 1.5, 9.0, 9.5], 3),
                np.repeat([0.5, 5.0], [3, T - 3])]
    starts = [(0.0, 0.0), (-3.125, 7.5), (12.0, -0.375), (100.25, 64.0), (-8.0, -8.5)]
    axes = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (1.0, 0.0)]
    trajs = []
    for v, (x0, y0), (ax, ay) in zip(profiles, starts, axes):
        s = np.concatenate(([0.0], np.cumsum(v[:-1] * dt)))
        x, y = x0 + ax * s, y0 + ay * s
        chord = np.insert(np.cumsum(np.sqrt(np.diff(x) ** 2 + np.diff(y) ** 2)), 0, 0)
        assert np.array_equal(chord, s) and np.array_equal(np.insert(np.cumsum(v * dt), 0, 0)[:-1], chord)
        trajs.append(G.Traj(x, y, np.full(T, np.arctan2(ay, ax)), v, np.zeros(T)))
    be = BE(G.VehicleParams(), G.AgentManager(dt))
    rows = []
    for n, tr in enumerate(trajs):
        for b in range(1, 6):
            for a in (0.0, 0.5, 2.0, 3.0, 8.0):
                (out,), _ = be._calc_deceleration_trajectory(tr, break_time_step=b, deceleration=[a])
                c = out.cartesian
                rows.append((n, b, a, np.array(c.x), np.array(c.y), np.array(c.v)))
    v_new = np.stack([r[5] for r in rows])
    stops = (v_new[:, -1] == 0.0)
    assert stops.any() and (~stops).any()
    np.savez_compressed(os.path.join(G.OUT, "brake_manoeuvre.npz"), dt=np.float64(dt),
                        x=np.stack([t.cartesian.x for t in trajs]), y=np.stack([t.cartesian.y for t in trajs]),
                        v=np.stack([t.cartesian.v for t in trajs]), theta=np.stack([t.cartesian.theta for t in trajs]),
                        case_traj=np.array([r[0] for r in rows], dtype=np.int32), case_b=np.array([r[1] for r in rows], dtype=np.int32),
                        case_a=np.array([r[2] for r in rows], dtype=np.float64), x_new=np.stack([r[3] for r in rows]),
                        y_new=np.stack([r[4] for r in rows]), v_new=v_new)
    print(f"brake_manoeuvre.npz: {len(rows)} manoeuvres of {len(trajs)} trajectories, {int(stops.sum())} stop inside the horizon")


if __name__ == "__main__":
    main()
