"""Writes tests/golden/brake_ladder.npz: what the reference's own, unmodified ``BE._calc_deceleration_trajectory(traj,
break_time_step=b, deceleration=[lo, hi])`` (metrics/be.py:84-146) makes of a two-entry ``deceleration`` -- the ladder
``np.arange(lo, hi, 0.1)`` of be.py:106-107 -- and the speed row ``v`` of every level: the pin of
``hidden_traffic.reference_deceleration_ladder`` and of the speed profile of the brake ladder's checker (DESIGN.md §5.10 "Brake
ladder", tests/test_hidden_brake_ladder_cpu.py).  Arrays only, a few KB.

Run where the reference is present only (see gen_golden.py, whose loading of be.py -- ``gen_be`` -- and whose duck-typed harness
objects this script uses, as gen_brake_manoeuvre.py does).  be.py runs as it stands.

Positions are NOT recorded: tests/golden/brake_manoeuvre.npz pins the re-sampling rule on dyadic inputs, and at the non-dyadic
levels of an ``arange`` ladder the reference's running sum from 0 and the brake clearance's sum from ``arc[b]`` may differ in the last
bits (DESIGN.md §5.10 "Brake clearance").  The speed row has no such freedom: ``maximum(v[b] - decel * (n * dt), 0)`` is one
expression.  The trajectories are gen_brake_manoeuvre.py's kind -- straight, speeds that rise, so no manoeuvre runs past the
end of its path (where the reference raises) -- with a ``dt`` of 0.1 and speeds that are not dyadic on purpose."""
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

    dt, T = 0.1, 8
    profiles = [np.linspace(8.3, 8.9, T), np.linspace(2.7, 9.1, T), np.repeat([0.3, 4.4, 13.9, 14.2], 2)]
    trajs = []
    for n, v in enumerate(profiles):
        s = np.concatenate(([0.0], np.cumsum(v[:-1] * dt)))
        trajs.append(G.Traj(3.0 * n + s, np.full(T, -1.5 * n), np.zeros(T), v, np.zeros(T)))
    be = BE(G.VehicleParams(), G.AgentManager(dt))
    ladders = [(0.5, 11.6), (0.0, 3.0), (2.0, 2.05)]
    rows = []
    for lo, hi in ladders:
        for n, tr in enumerate(trajs):
            if hi - lo > 1.0 and n != (1 if hi > 10.0 else 2):   # a long ladder on one trajectory each: the file stays small
                continue
            for b in ((1,) if hi > 10.0 else (1, 3, 6)):
                outs, decel = be._calc_deceleration_trajectory(tr, break_time_step=b, deceleration=[lo, hi])
                decel = np.asarray(decel, dtype=np.float64)
                assert len(outs) == len(decel)
                rows.append((lo, hi, n, b, decel, np.stack([np.array(o.cartesian.v, dtype=np.float64) for o in outs])))
    out = dict(dt=np.float64(dt), v=np.stack([t.cartesian.v for t in trajs]),
               case_lo=np.array([r[0] for r in rows]), case_hi=np.array([r[1] for r in rows]),
               case_traj=np.array([r[2] for r in rows], dtype=np.int32), case_b=np.array([r[3] for r in rows], dtype=np.int32))
    # one array per kind, the calls one after the other (a zip member per call would cost more than its numbers)
    out["levels"] = np.array([len(r[4]) for r in rows], dtype=np.int32)
    out["decel"] = np.concatenate([r[4] for r in rows])
    out["v_new"] = np.concatenate([r[5] for r in rows])          # [sum(levels), T]
    np.savez_compressed(os.path.join(G.OUT, "brake_ladder.npz"), **out)
    print(f"brake_ladder.npz: {len(rows)} calls, ladders of {sorted({len(r[4]) for r in rows})} levels")


if __name__ == "__main__":
    main()
