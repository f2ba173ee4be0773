#!/usr/bin/env python3
"""Writes tests/golden/dce_rounding.npz and tests/golden/cp_exact.npz: the sweep inputs built by tests/ref_sweep_exact.py
and the outputs its exact references give for them (no reference code is run; see that module's docstring).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_sweep_exact.py

tests/test_sweep_exact_cpu.py rebuilds both files' contents and checks them bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_sweep_exact as R  # noqa: E402

TTC_THR = 100.0     # every finite TTC is below it: `safe` is False exactly where some pair's rounded DCE is 0.0


def _inputs(traj, agents, veh, dt):
    out = {"traj_" + k: traj[k] for k in ("x", "y", "theta", "v", "a")}
    out.update({"agent_" + k: agents[k] for k in ("pos", "yaw", "v", "cov", "shape", "raw_dims", "type", "len")})
    out.update({"vehicle": np.array(veh), "dt": dt})
    return out


def dce_contents():
    traj, agents, labels, pair_agent = R.build_dce_inputs()
    dce, tdce, ttc, ttce, safe, recs = R.expected_dce(traj, agents, R.DCE_VEH, R.DCE_DT, TTC_THR)
    out = _inputs(traj, agents, R.DCE_VEH, R.DCE_DT)
    out.update({"label": np.array(labels), "pair_agent": pair_agent, "ttc_thr": TTC_THR, "ref_dce": dce,
                "ref_time_dce": tdce, "ref_ttc": ttc, "ref_ttce": ttce, "ref_safe": safe,
                "rec_m": recs["m"], "rec_a": recs["a"], "rec_t": recs["t"], "rec_mm": recs["mm"], "rec_tie": recs["tie"],
                "rec_gap_mm": recs["gap_mm"]})
    return out


def cp_contents(erf_args=None):
    """(erf_args: a list that receives the diagonal erf arguments, in units of sigma sqrt 2)"""
    traj, agents, pair_agent = R.build_cp_inputs()
    cp, us = R.expected_cp(traj, agents, R.CP_VEH)
    if erf_args is not None:
        erf_args.append(us)
    out = _inputs(traj, agents, R.CP_VEH, R.CP_DT)
    out.update({"pair_agent": pair_agent, "n_diag": len(R.DIAG_SIG), "ref_cp": cp})
    return out


if __name__ == "__main__":
    for name, fn in (("dce_rounding", dce_contents), ("cp_exact", cp_contents)):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **fn())
        print("wrote", path, os.path.getsize(path), "bytes")
