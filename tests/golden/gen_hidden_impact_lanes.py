"""Writes tests/golden/hidden_impact_lanes.npz: what the reference's own, unmodified ``get_harm`` (metrics/utils/harm_model.py:35-107,
with logistic_regression.py:11-75) answers for one-sample pairs of an ego pose and a road user whose heading obeys a move byte -- the pin
of the approach cosine and the closing speed of the hidden-traffic impact verdict by approach angle (DESIGN.md §5.10 "Impact verdict by
approach angle", csrc/fo_hidden_approach.hpp, tests/test_hidden_impact_lanes_cpu.py).  Numbers only, a few KB.

Run where the reference is present only (see gen_golden.py and gen_hidden_impact.py, whose harness this script uses).  harm_model.py
runs as it stands, with the reference's own harm_params.json and risk_params.json.

The headings a move byte leaves are H = the union over its central directions k (bits k - 1, k, k + 1 all set) of
[k 45 deg - h, k 45 deg + h], h = 22.5 deg + heading_slack.

Two blocks.  ``bound_*``: pairs built to ATTAIN the bound -- the road user's yaw is the maximiser of cos(pdof) over H: theta + pi if it
lies inside H, else the sector edge nearest to it; the user stands where both angles of impact fall into the area whose LR4S term is
greatest -- for Car, Bicycle, Pedestrian and Truck x ego speeds {0.5, 3, 8, 15} x user speeds {2.0, 7.0, 13.9} x the (ego heading,
byte, slack) combinations of COMBOS: a side approach, a same-direction approach, a sector that holds theta + pi, a two-sector union,
non-lattice ego headings, a slack.  ``rand_*``: 256 pairs per type with the yaw uniform inside H at random headings, bytes, slacks,
positions and speeds: no reference harm may exceed the stage's."""
import math
import os
import sys
import types

import numpy as np

import gen_golden as G
import gen_hidden_impact as GI

KINDS = GI.KINDS
EGO_SPEEDS = (0.5, 3.0, 8.0, 15.0)
USER_SPEEDS = GI.USER_SPEEDS
N_RANDOM = 256
BASE = math.pi / 8.0
# (ego heading in degrees, move byte, heading_slack in radians)
COMBOS = (
    (0.0, 0b00001110, 0.0),        # the ego heads east, the lane north (bits 1, 2, 3; central 2): a side approach, sector centre 90 deg off
    (0.0, 0b10000011, 0.0),        # the lane heads east like the ego (bits 7, 0, 1; central 0): the same direction, the user from behind
    (10.0, 0b00111000, 0.0),       # the lane heads west (central 4): the sector holds theta + pi, head-on
    (0.0, 0b00011111, 0.0),        # an east, a north and a west lanelet over one cell: bits 0 .. 4, central 1, 2, 3 -- a union of three sectors
    (45.0, 0b10001111, 0.0),       # an east and a north lanelet: bits 7, 0, 1 | 1, 2, 3 -- central 0, 1, 2: a two-sector union and more
    (33.3, 0b11100000, 0.0),       # a non-lattice ego heading against a south-bound lane (central 6)
    (-141.7, 0b00001110, 0.2),     # a non-lattice heading, slack 0.2 rad
    (200.0, 0b11000001, 0.2),      # central 7, slack
)


def central(byte):
    return [k for k in range(8) if all(byte >> ((k + d) % 8) & 1 for d in (-1, 0, 1))]


def wrap(a):
    return (a + math.pi) % (2.0 * math.pi) - math.pi


def maximiser(theta, byte, slack):
    """the yaw in H whose cos(yaw - theta + pi) is greatest: theta + pi inside H, else the nearest sector edge"""
    h = BASE + slack
    target = theta + math.pi
    best = None
    for k in central(byte):
        d = wrap(target - k * math.pi / 4.0)
        yaw = target if abs(d) <= h else k * math.pi / 4.0 + math.copysign(h, d)
        c = math.cos(yaw - theta + math.pi)
        if best is None or c > best[0]:
            best = (c, yaw)
    return best[1]


def in_side(a):
    return math.pi / 4.0 <= a < 3.0 * math.pi / 4.0 or -math.pi / 4.0 >= a > -3.0 * math.pi / 4.0


def placed(theta, yaw, worst, rng=None):
    """(theta', yaw', position): the same headings written so that, as harm_model.py:81-88 forms them without wrapping, BOTH angles of
    impact lie in the area of `worst` (pi / 2: the side areas) -- or, with ``rng``, a random position and the headings as they are"""
    if rng is not None:
        return theta, yaw, rng.uniform(-6.0, 6.0, size=2)
    assert worst == math.pi / 2.0
    d = wrap(yaw - theta - math.pi)
    feasible = [e for e in np.linspace(-math.pi, math.pi, 2881)[1:-1] if in_side(e) and in_side(wrap(e - d))]
    assert feasible, (theta, yaw)
    runs, run = [], [feasible[0]]
    for e in feasible[1:]:
        if e - run[-1] > 2.0 * math.pi / 2880 * 1.5:
            runs.append(run)
            run = []
        run.append(e)
    runs.append(run)
    run = max(runs, key=len)
    e = run[len(run) // 2]                                            # the middle of the widest feasible interval
    rel = wrap(theta + e)
    pos = (3.0 * math.cos(rel), 3.0 * math.sin(rel))
    rel = math.atan2(pos[1], pos[0])
    theta2 = theta + 2.0 * math.pi * round((rel - theta - e) / (2.0 * math.pi))
    obs = wrap(e - d)
    yaw2 = yaw + 2.0 * math.pi * round((math.pi + rel - yaw - obs) / (2.0 * math.pi))
    assert in_side(rel - theta2) and in_side(math.pi + rel - yaw2)
    return theta2, yaw2, pos


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
    worst = max((0.0, 0.0), (area["side"], math.pi / 2), (area["rear"], math.pi))[1]

    def one(kind, theta, v_ego, yaw, pos, v_obs):
        am = G.AgentManager(0.1)
        am.phantom_agents.append(G.Agent(10000, kind))
        length, width = GI.dims(kind)
        pred = {"pos_list": np.array([pos], dtype=np.float64), "v_list": np.array([v_obs]), "orientation_list": np.array([yaw]),
                "shape": {"length": length, "width": width}}
        traj = G.Traj([0.0, 0.1 * v_ego * np.cos(theta)], [0.0, 0.1 * v_ego * np.sin(theta)], [theta, theta], [v_ego, v_ego], [0.0, 0.0])
        ego, obst = get_harm(am, traj, {100000: pred}, vp, modes, coeffs)
        return float(np.ravel(ego[100000])[0]), float(np.ravel(obst[100000])[0])

    bound, rand = [], []
    for k, kind in enumerate(KINDS):
        for v_ego in EGO_SPEEDS:
            for v_obs in USER_SPEEDS:
                for deg, byte, slack in COMBOS:
                    theta = math.radians(deg)
                    yaw = maximiser(theta, byte, slack)
                    theta2, yaw2, pos = placed(theta, yaw, worst)
                    ego, obst = one(kind, theta2, v_ego, yaw2, pos, v_obs)
                    bound.append((k, v_ego, v_obs, theta, byte, slack, yaw, ego, obst))
    rng = np.random.default_rng(20240923)
    steps = np.deg2rad(45.0 * np.arange(8))
    for k, kind in enumerate(KINDS):
        for _ in range(N_RANDOM):
            theta = rng.uniform(-math.pi, math.pi)
            while True:                                               # the byte of one or two lanelets by the builder's predicate
                lanes = rng.uniform(-math.pi, math.pi, size=int(rng.integers(1, 3)))
                byte = 0
                for phi in lanes:
                    byte |= int(((np.cos(steps - phi) >= math.cos(math.radians(67.5))) * (1 << np.arange(8))).sum())
                if central(byte):
                    break
            slack = float(rng.choice([0.0, 0.2]))
            kc = int(rng.choice(central(byte)))
            yaw = kc * math.pi / 4.0 + rng.uniform(-(BASE + slack), BASE + slack)
            v_ego, v_obs = rng.uniform(0.0, 16.0), rng.uniform(0.0, 15.0)
            _, _, pos = placed(theta, yaw, worst, rng)
            ego, obst = one(kind, theta, v_ego, yaw, pos, v_obs)
            rand.append((k, v_ego, v_obs, theta, byte, slack, yaw, ego, obst))
    bound, rand = np.array(bound), np.array(rand)
    out = dict(kinds=np.array(KINDS), dims=np.array([GI.dims(k) for k in KINDS]), ego_mass=np.float64(vp.mass),
               coeff=np.array([area["const"], area["speed"], area["side"], area["rear"], coeffs["log_reg"]["ignore_angle"]["const"],
                               coeffs["log_reg"]["ignore_angle"]["speed"], coeffs["pedestrian"]["const"], coeffs["pedestrian"]["speed"]]))
    for name, rows in (("bound", bound), ("rand", rand)):
        out.update({f"{name}_kind": rows[:, 0].astype(np.int32), f"{name}_v_ego": rows[:, 1], f"{name}_v_obs": rows[:, 2],
                    f"{name}_theta": rows[:, 3], f"{name}_byte": rows[:, 4].astype(np.int32), f"{name}_slack": rows[:, 5],
                    f"{name}_yaw": rows[:, 6], f"{name}_ego_harm": rows[:, 7], f"{name}_obst_harm": rows[:, 8]})
    np.savez_compressed(os.path.join(G.OUT, "hidden_impact_lanes.npz"), **out)
    print(f"hidden_impact_lanes.npz: {len(bound)} pairs at the bound, {len(rand)} random pairs")


if __name__ == "__main__":
    main()
