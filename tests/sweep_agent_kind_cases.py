"""The agent set of tests/test_sweep_agent_kinds_gpu.py (its reference side is pinned in tests/test_sweep_agent_kinds_cpu.py):
the smallest batch at which choosing the queue kernel's per-agent body once per agent can go wrong.  NumPy and the CPU oracle
only.

The queue kernel runs everything it does per agent in one of three copies, by harm model (fo_sweep_queue.hpp, agent_body):
LR4S (cars, trucks), DVMAX (the two-coefficient models -- pedestrian, bicycle -- with the usual signs of the speed
coefficients) and GENERIC (no harm model, or a speed coefficient of unusual sign).  One agent set holds

* M = 70 candidates: one full tile plus six real lanes; T = 31 and T = 10 (chunks end at 8: a last chunk of seven, and of two);
* A = 9 agents, the four phantom types and one agent without a harm model interleaved, so that the agents one wave takes one
  after the other (four agents per wave: 0-3, 4-7, 8) change body in every order: LR4S -> inactive -> DVMAX -> LR4S, DVMAX ->
  GENERIC -> DVMAX -> LR4S; and GENERIC <-> LR4S, GENERIC -> GENERIC under the second coefficient set;
* prediction lengths 0, 1, 8, 9, 30, 31 and 34 (longer than T, on a table of 34 samples), the inactive slot between two active
  ones: every slot and chunk that has to take the range-checked form of pass 1;
* a car, a pedestrian and the agent without a harm model that the candidates drive through: in-gate samples and DCE = 0 in
  every body.

The speed coefficients belong to the context (fo_sweep_configure), not to an agent: "an agent whose speed coefficients have an
unusual sign" is the same set under a second coefficient set (`ped_speed` negated), under which every two-coefficient agent
takes GENERIC instead of DVMAX."""
import numpy as np

M, A, TA, DT = 70, 9, 34, 0.1
HORIZONS = (31, 10)
TYPE_NONE = 11     # no ObstacleType of the reference: protection class 2, harm 1 on both sides
#         kind          type  len  x     y     yaw            speed
AGENTS = (("car",        0,   31,  9.0,  0.5,  0.0,           3.0),    # driven into from behind
          ("pedestrian", 4,   0,   8.0,  3.0,  -np.pi / 2,    1.4),    # inactive slot
          ("bicycle",    3,   8,   9.0,  -2.0, np.pi / 2,     5.0),    # crosses the candidates' path
          ("truck",      1,   9,   20.0, 4.0,  np.pi,         10.0),   # oncoming, one lane over
          ("pedestrian", 4,   31,  7.0,  -1.0, np.pi / 2,     1.4),    # walks across the path: driven through
          ("pedestrian", TYPE_NONE, 30, 6.0, 1.0, -np.pi / 2, 0.5),    # no harm model: driven through
          ("bicycle",    3,   34,  15.0, 2.0,  np.pi,         5.0),
          ("car",        0,   1,   10.0, -3.0, 0.0,           10.0),
          ("pedestrian", 4,   31,  25.0, -6.0, np.pi / 2,     1.4))
LENGTHS = (0, 1, 8, 9, 30, 31, 34)
HM_LR4S, HM_DVMAX, HM_GENERIC = "lr4s", "dvmax", "generic"
PROT1 = (0, 1, 2, 5, 6, 7, 9)      # fo_obstacle_protection: the LR4S types
PROT0 = (3, 4, 8, 10)              # the two-coefficient types


def harm_coeffs(O):
    """(name, coefficient set): the reference's, and `ped_speed` negated (the obstacle-side slope of the two-coefficient models)"""
    flipped = dict(O.HARM_COEFF)
    flipped["ped_speed"] = -flipped["ped_speed"]
    return (("usual", dict(O.HARM_COEFF)), ("ped_speed negated", flipped))


def body_of(type_code, hc):
    """the copy of the per-agent body the kernel takes (fo_agent_rows.hpp c[10], c[11]; the mass shares are >= 0)"""
    if type_code in PROT1:
        return HM_LR4S
    if type_code in PROT0 and hc["lr1s_speed"] >= 0.0 and hc["ped_speed"] >= 0.0:
        return HM_DVMAX
    return HM_GENERIC


def make_case(T):
    from frenetix_occlusion import synthetic as S
    traj = S.make_trajectories(M, T, DT, seed=20240131 + 77)
    p0 = np.array([[a[3], a[4]] for a in AGENTS])
    agents = S.predictions_from_spawns(p0, [a[5] for a in AGENTS], [a[0] for a in AGENTS], TA, DT, speed=[a[6] for a in AGENTS])
    agents["type"] = np.array([a[1] for a in AGENTS], dtype=np.int32)
    agents["len"] = np.array([a[2] for a in AGENTS], dtype=np.int32)
    return traj, agents, S.VEHICLE_BMW320I, DT


_REF = {}


def thresholds(O, T):
    """a risk and a cp threshold inside the range of the candidates' own values (the medians of the oracle's run without
    thresholds under the usual coefficients): both verdicts are common, and a wrong maximum flips `safe`"""
    if ("thr", T) not in _REF:
        traj, agents, veh, dt = make_case(T)
        c = O.sweep(traj, agents, veh, dt, want_lists=False)["cost"]
        _REF[("thr", T)] = {"risk": float(np.median(c[:, O.COST["max_obst_risk_all"]])),
                            "cp": float(np.quantile(c[:, O.COST["max_collision_probability_all"]], 0.75))}
    return _REF[("thr", T)]


def oracle_run(O, T, hc_name):
    """the oracle on the set (the six default metrics, thresholds(O, T)); cached: treat as read-only"""
    if (T, hc_name) not in _REF:
        traj, agents, veh, dt = make_case(T)
        _REF[(T, hc_name)] = O.sweep(traj, agents, veh, dt, thr=thresholds(O, T), harm_coeff=dict(harm_coeffs(O))[hc_name])
    return _REF[(T, hc_name)]


def assert_every_body_is_exercised(O, T, hc_name):
    """every body the coefficient set reaches holds a pair with an in-gate sample and a pair with DCE = 0 inside its harm
    length -- and the set is what the header says it is"""
    hc = dict(harm_coeffs(O))[hc_name]
    ref = oracle_run(O, T, hc_name)
    types, lens = [a[1] for a in AGENTS], [a[2] for a in AGENTS]
    assert len(AGENTS) == A and sorted(set(lens)) == list(LENGTHS) and max(lens) > max(HORIZONS)
    assert lens[1] == 0 and lens[0] > 0 and lens[2] > 0
    assert {0, 1, 3, 4} <= set(types)
    bodies = [body_of(t, hc) for t in types]
    want = {HM_LR4S, HM_GENERIC} | ({HM_DVMAX} if hc_name == "usual" else set())
    assert set(bodies) == want, bodies
    # consecutive active agents of one wave (four agents per wave) change body in both directions
    steps = set()
    for w0 in range(0, A, 4):
        act = [bodies[k] for k in range(w0, min(w0 + 4, A)) if lens[k] > 0]
        steps |= set(zip(act, act[1:]))
    if hc_name == "usual":
        assert {(HM_LR4S, HM_DVMAX), (HM_DVMAX, HM_LR4S), (HM_DVMAX, HM_GENERIC), (HM_GENERIC, HM_DVMAX)} <= steps, steps
    else:
        assert {(HM_LR4S, HM_GENERIC), (HM_GENERIC, HM_LR4S), (HM_GENERIC, HM_GENERIC)} <= steps, steps
    cp = ref["lists"][:, :, O.LST["cp"], :]
    dce = ref["pair_f"][..., O.PF["dce"]]
    for body in want:
        ks = [k for k in range(A) if bodies[k] == body and lens[k] > 1]
        gate = {k: int((cp[:, k, :] > 0).any(axis=-1).sum()) for k in ks}
        zero = {k: int((dce[:, k] == 0.0).sum()) for k in ks}
        assert max(gate.values()) > 0 and max(zero.values()) > 0, (T, hc_name, body, gate, zero)
        # ... and pairs that never reach the gate, so that both row forms of pass 2 run in the body
        assert any(g < M for g in gate.values()) or any((cp[:, k, :] == 0).any() for k in ks), (T, hc_name, body)
    # the inactive slot: no output of its own
    assert np.isnan(ref["pair_f"][:, 1, O.PF["dce"]]).all() and np.isnan(ref["lists"][:, 1]).all()
    assert 0.0 < ref["safe"].mean() < 1.0, (T, hc_name, float(ref["safe"].mean()))
    return bodies
