"""Writes tests/golden/hidden_impact_harm.npz: what the reference's own, unmodified ``get_harm`` (metrics/utils/harm_model.py:35-107,
with logistic_regression.py:11-75) answers for one-sample pairs of an ego pose and a road user -- the pin of the harm rows of the
hidden-traffic impact verdict (DESIGN.md §5.10 "Impact verdict", csrc/fo_hidden_impact.hpp, tests/test_hidden_impact_cpu.py).  Numbers
only, a few KB.

Run where the reference is present only (see gen_golden.py, whose aliases for the absent third-party names and whose duck-typed harness
objects this script uses, as gen_brake_ladder.py does).  harm_model.py runs as it stands, with the reference's own harm_params.json and
risk_params.json.

Two blocks.  ``bound_*``: pairs built to ATTAIN the bound a row states -- the road user drives against the ego's heading (yaw = theta +
pi, so cos(pdof) = 1 and dv = v_ego + v_obs) and stands where both angles of impact fall into the area whose LR4S term is greatest
under the reference's coefficients -- for Car, Bicycle, Pedestrian and Truck x ego speeds {0, 0.5, 3, 8, 15} x the README's user speeds
{2.0, 7.0, 13.9}.  ``rand_*``: 256 pairs per type at random yaws, positions and speeds: no reference harm may exceed the row's."""
import os
import sys
import types

import numpy as np

import gen_golden as G

KINDS = ("Car", "Bicycle", "Pedestrian", "Truck")
EGO_SPEEDS = (0.0, 0.5, 3.0, 8.0, 15.0)
USER_SPEEDS = (2.0, 7.0, 13.9)
N_RANDOM = 256


def dims(kind):
    raw_l, raw_w = G.RAW_DIMS[kind]
    fl, fw = (1.4, 2.5) if kind == "Bicycle" else (1.2, 1.3)       # the prediction's size factors, as gen_golden.make_prediction
    return raw_l * fl, raw_w * fw


def main():
    G._install_aliases()
    sys.path.insert(0, G.REF)
    for modname, cls_name, cls in (("frenetix_occlusion.metrics.dce", "DCE", G._OracleDCE), ("frenetix_occlusion.metrics.be", "BE", G._NoBE)):
        mod = types.ModuleType(modname)
        setattr(mod, cls_name, cls)
        sys.modules[modname] = mod
    from frenetix_occlusion.metrics.hr import HR                     # (its _load_param: the reference's own parameter files)
    from frenetix_occlusion.metrics.utils.harm_model import get_harm  # the reference's own function, unmodified
    vp = G.VehicleParams()
    modes, coeffs = HR._load_param("risk_params"), HR._load_param("harm_params")
    area = coeffs["log_reg"]["reduced_sym_angle_areas"]
    # the angle of impact of the worst area: front 0, side pi / 2, rear pi
    worst = max((0.0, 0.0), (area["side"], np.pi / 2), (area["rear"], np.pi))[1]

    def one(kind, theta, v_ego, yaw, pos, v_obs):
        am = G.AgentManager(0.1)
        am.phantom_agents.append(G.Agent(10000, kind))
        length, width = dims(kind)
        pred = {"pos_list": np.array([pos], dtype=np.float64), "v_list": np.array([v_obs]), "orientation_list": np.array([yaw]),
                "shape": {"length": length, "width": width}}
        traj = G.Traj([0.0, 0.1 * v_ego * np.cos(theta)], [0.0, 0.1 * v_ego * np.sin(theta)], [theta, theta], [v_ego, v_ego], [0.0, 0.0])
        ego, obst = get_harm(am, traj, {100000: pred}, vp, modes, coeffs)
        return float(np.ravel(ego[100000])[0]), float(np.ravel(obst[100000])[0])

    bound, rand = [], []
    for k, kind in enumerate(KINDS):
        for n, v_ego in enumerate(EGO_SPEEDS):
            for v_obs in USER_SPEEDS:
                theta = 0.3 * n - 0.5
                rel = theta + worst                                  # both angles of impact are `worst`
                ego, obst = one(kind, theta, v_ego, theta + np.pi, (3.0 * np.cos(rel), 3.0 * np.sin(rel)), v_obs)
                bound.append((k, v_ego, v_obs, ego, obst))
    rng = np.random.default_rng(20240607)
    for k, kind in enumerate(KINDS):
        for _ in range(N_RANDOM):
            theta, yaw = rng.uniform(-np.pi, np.pi, size=2)
            v_ego, v_obs = rng.uniform(0.0, 16.0), rng.uniform(0.0, 15.0)
            ego, obst = one(kind, theta, v_ego, yaw, rng.uniform(-6.0, 6.0, size=2), v_obs)
            rand.append((k, v_ego, v_obs, ego, obst))
    bound, rand = np.array(bound), np.array(rand)
    out = dict(kinds=np.array(KINDS), dims=np.array([dims(k) for k in KINDS]), ego_mass=np.float64(vp.mass),
               coeff=np.array([area["const"], area["speed"], area["side"], area["rear"], coeffs["log_reg"]["ignore_angle"]["const"],
                               coeffs["log_reg"]["ignore_angle"]["speed"], coeffs["pedestrian"]["const"], coeffs["pedestrian"]["speed"]]))
    for name, rows in (("bound", bound), ("rand", rand)):
        out.update({f"{name}_kind": rows[:, 0].astype(np.int32), f"{name}_v_ego": rows[:, 1], f"{name}_v_obs": rows[:, 2],
                    f"{name}_ego_harm": rows[:, 3], f"{name}_obst_harm": rows[:, 4]})
    np.savez_compressed(os.path.join(G.OUT, "hidden_impact_harm.npz"), **out)
    print(f"hidden_impact_harm.npz: {len(bound)} pairs at the bound, {len(rand)} random pairs")


if __name__ == "__main__":
    main()
