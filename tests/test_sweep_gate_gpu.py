"""The sweep kernels at the places where a kernel can be wrong and stay within the continuous 1e-9 of tests/test_sweep_gpu.py:

* the collision-probability gate at its boundary (tests/golden/cp_gate_boundary.npz, the reference's own code on ego samples
  within three ulps of the 5 m circle): every in / out decision exactly, in every kernel form that runs the gate;
* saturated gate work -- full pool rounds of the queue kernel, empty queues and dead waves in one workgroup -- and the
  tapered launch plans with ragged phases, against the oracle;
* bit-identical maxima (the first index wins, np.argmax) and thresholds equal to the device's own values (the reference's
  `>` / `<`, metric.py:58-95).

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

from golden_util import load_case
from test_sweep_gpu import ATOL, _compare, _hip_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


# (env, forms): the library's own choice, both queue-kernel forms forced, the generic kernel
KERNEL_FORMS = [("auto", {}), ("queue, no split", {"FO_SWEEP_SPLIT": "0"}), ("queue, split", {"FO_SWEEP_SPLIT": "1"}),
                ("generic", {"FO_SWEEP_GENERIC": "1"})]


def _set_env(monkeypatch, env):
    for k in ("FO_SWEEP_SPLIT", "FO_SWEEP_GENERIC", "FO_SWEEP_APW", "FO_SWEEP_TAPER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------ the CP gate's boundary
@pytest.mark.parametrize("form,env", KERNEL_FORMS, ids=[f[0] for f in KERNEL_FORMS])
def test_cp_gate_boundary_decisions_match_the_reference(torch_cuda, oracle, monkeypatch, form, env):
    from frenetix_occlusion import _native as N
    g, traj, agents, veh, dt = load_case("cp_gate_boundary")
    ing = g["ref_in_gate"]
    mxc = g["ref_max_collision_probability"]
    # a cp threshold inside the range of the trajectories' maxima: a flipped sample that holds a maximum flips `safe`
    thr = {"cp": float(np.median(g["ref_max_collision_probability_all"]))}
    ref = oracle.sweep(traj, agents, veh, dt, thr=thr)
    assert 0 < ref["safe"].mean() < 1
    _set_env(monkeypatch, env)
    got = _hip_sweep(torch_cuda, traj, agents, veh, dt, thr=thr)
    gx = _hip_sweep(torch_cuda, traj, agents, veh, dt, thr=thr, lists="f32x")
    red = _hip_sweep(torch_cuda, traj, agents, veh, dt, thr=thr, mode="reduced")
    cp = got["lists"][:, :, N.LST["cp"], :]
    bad = np.argwhere((cp > 0.0) != ing)
    assert len(bad) == 0, f"{form}: {len(bad)} gate decisions differ from the reference's, (m, a, t-1) e.g. {bad[:10].tolist()}"
    np.testing.assert_allclose(cp, g["ref_cp"], rtol=0, atol=ATOL)
    cpx = gx["lists"][:, :, N.LST["cp"], :]
    assert np.array_equal(cpx > 0.0, ing) and np.array_equal(cpx, cp.astype(np.float32))
    for out in (got, gx):
        pf, pi = out["pair_f"], out["pair_i"]
        np.testing.assert_allclose(pf[..., N.PF["max_collision_probability"]], mxc, rtol=0, atol=ATOL)
        np.testing.assert_allclose(pf[..., N.PF["max_obst_harm_with_cp"]], g["ref_max_obst_harm_with_cp"], rtol=0, atol=ATOL)
        assert np.array_equal(pi[..., N.PI["cp_argmax"]], g["ref_cp_argmax"])
        assert np.array_equal(out["safe"], ref["safe"])
    for out in (got, gx, red):
        np.testing.assert_allclose(out["cost"][:, N.COST["max_collision_probability_all"]],
                                   g["ref_max_collision_probability_all"], rtol=0, atol=ATOL)
        assert np.array_equal(out["safe"], ref["safe"])
    assert np.array_equal(red["cost"], got["cost"], equal_nan=True)
    _compare(oracle, ref, got)


# ------------------------------------------------------------------------------------------ saturated and empty gate pools
def _fan(M, T, seed, x0=0.0):
    """a tight trajectory fan: all lanes of a tile within ~2 m of each other, straight ahead at 6-8 m/s"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * 0.1
    v = rng.uniform(6.0, 8.0, M)
    lat = rng.uniform(-0.5, 0.5, M)
    x = x0 + v[:, None] * t[None, :]
    y = lat[:, None] * (t[None, :] / max(t[-1], 0.1))
    th = np.arctan2(np.gradient(y, axis=1), np.gradient(x, axis=1)) if T > 1 else np.zeros((M, T))
    return {"x": x, "y": y, "theta": th, "v": np.repeat(v[:, None], T, 1), "a": np.zeros((M, T))}


def _riders(A, T, seed, far_every=5):
    """agents riding along the fan (every sample of every pair in the gate) interleaved with agents far away (empty queues);
    diagonal, weakly and strongly correlated covariances alternate, so one pooled batch holds all kinds"""
    from frenetix_occlusion import synthetic as S
    rng = np.random.default_rng(seed)
    ag = S.make_agents(A, T, 0.1, seed=seed)
    t = np.arange(T) * 0.1
    for k in range(A):
        v = rng.uniform(6.0, 8.0)
        off = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5)])
        if k % far_every == far_every - 1:
            off = off + np.array([500.0, 300.0])
        ag["pos"][k] = off + np.stack((v * t, np.zeros(T)), -1)
        ag["yaw"][k] = 0.0
        ag["v"][k] = v
        sxx, syy = rng.uniform(0.2, 1.5, 2)
        rho = (0.0, 0.2, -0.85)[k % 3]
        ag["cov"][k] = np.array([[sxx, rho * np.sqrt(sxx * syy)], [rho * np.sqrt(sxx * syy), syy]])
    ag["len"][:] = T
    return ag


@pytest.mark.parametrize("T", [31, 10])
def test_saturated_gate_pools_match_the_oracle(torch_cuda, oracle, monkeypatch, T):
    """Every in-gate sample is queued per wave and pooled over the workgroup's four waves (2 048 samples a round at one agent
    per wave): a round must fill up completely, next to waves with empty queues and dead waves past the last agent"""
    from frenetix_occlusion import synthetic as S
    from frenetix_occlusion import _native as N
    M, A = 256, 23                                   # ragged: the last chunk of four agents has one live wave and ...
    traj, agents = _fan(M, T, 11), _riders(A, T, 12)
    thr = {"harm": 0.3, "risk": 0.2, "ttc": 1.0, "dce": 0.05, "cp": 0.5}
    ref = oracle.sweep(traj, agents, S.VEHICLE_BMW320I, 0.1, thr=thr, nthreads=8)
    cp = ref["lists"][:, :, N.LST["cp"], :]
    near = np.array([k % 5 != 4 for k in range(A)])
    assert (cp[:, near, :] > 0).mean() >= 0.9, (cp[:, near, :] > 0).mean()
    assert (cp[:, ~near, :] == 0).all()
    # a full pool round: four consecutive agents of one chunk (one per wave) entirely in the gate over one 8-sample chunk of
    # a 64-lane tile -- 4 x 64 x 8 = 2 048 queued samples
    full = False
    for k0 in range(0, A - 3, 4):
        for t0 in range(0, T - 1, 8):
            if t0 + 8 <= T - 1:
                blk = cp[:64, k0:k0 + 4, t0:t0 + 8] > 0
                full |= bool(blk.all())
    assert full, "no full pool round in the batch"
    seen = set()
    for form, env in [("auto", {}), ("queue, no split", {"FO_SWEEP_SPLIT": "0"}), ("apw 1", {"FO_SWEEP_APW": "1", "FO_SWEEP_SPLIT": "0"}),
                      ("generic", {"FO_SWEEP_GENERIC": "1"})]:
        _set_env(monkeypatch, env)
        got = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr=thr)
        _compare(oracle, ref, got)
        gx = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr=thr, lists="f32x")
        for k in ("cost", "safe", "pair_i"):
            assert np.array_equal(gx[k], got[k]), (form, k)
        assert np.array_equal(gx["lists"], got["lists"].astype(np.float32), equal_nan=True), form
        seen.add((form, got["launch"]["agents_per_wave"]))
        red = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr=thr, mode="reduced")
        assert np.array_equal(red["safe"], ref["safe"]), form
        np.testing.assert_allclose(red["cost"], ref["cost"], rtol=0, atol=ATOL)
    assert ("apw 1", 1) in seen, seen


# ---------------------------------------------------------------------------------------- tapered plans, ragged phases
# (M, A, env, tapered): A = wpb * apw * k -+ 1 with wpb = 4, so every phase boundary of the taper and its tail are ragged.
# `tapered` is what the planner (plan_sweep, fo_sweep_plan.hpp) does with that shape TODAY: a planner
# change that moves a case from one form to the other must update this table, knowingly -- the matrix must meet both.
TAPER_CASES = [
    (4095, 255, {}, True),                          # the default apw = 2 taper: 85 % at apw 2, 10 % at 1, the apw 1 tail
    (4097, 257, {}, True),
    (6143, 255, {"FO_SWEEP_APW": "8"}, True),       # three phases 8 / 4 / 2 plus the apw 1 tail
    (9857, 129, {"FO_SWEEP_APW": "8"}, True),
    (4095, 255, {"FO_SWEEP_TAPER": "0"}, False),    # the untapered control
]


def _corridor(M, A, seed):
    from frenetix_occlusion import synthetic as S
    traj = S.make_trajectories(M, 31, 0.1, seed=seed)
    agents = S.make_agents(A, 31, 0.1, seed=seed, lateral=6.0)
    return traj, agents


@pytest.mark.parametrize("M,A,env,tapered", TAPER_CASES, ids=[f"{c[0]}x{c[1]}-{'-'.join(c[2].values()) or 'default'}" for c in TAPER_CASES])
def test_tapered_plans_with_ragged_phases_match_the_oracle(torch_cuda, oracle, monkeypatch, M, A, env, tapered):
    from frenetix_occlusion import synthetic as S
    from frenetix_occlusion import _native as N
    traj, agents = _corridor(M, A, 20241016 + A)
    thr = {"harm": 0.3, "risk": 0.2, "ttc": 1.0, "dce": 0.05, "cp": 0.5}
    ref = oracle.sweep(traj, agents, S.VEHICLE_BMW320I, 0.1, thr=thr, nthreads=16, want_lists=False)
    mxc = ref["pair_f"][..., N.PF["max_collision_probability"]]
    assert (mxc > 0).mean() >= 0.10, (mxc > 0).mean()                                    # >= 10 % in the gate
    assert (ref["pair_f"][..., N.PF["dce"]] == 0).mean() >= 0.01                          # ... and >= 1 % colliding
    _set_env(monkeypatch, env)
    monkeypatch.setenv("FO_SWEEP_SPLIT", "0")
    got = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr=thr, mode="pair")
    got["lists"] = None
    _compare(oracle, {**ref, "lists": None}, got)
    red = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr=thr, mode="reduced")
    assert np.array_equal(red["safe"], ref["safe"])
    np.testing.assert_allclose(red["cost"], ref["cost"], rtol=0, atol=ATOL)
    launch = got["launch"]
    apw = launch["agents_per_wave"]
    n_tiles = (M + 63) // 64
    untapered = n_tiles * ((A + 4 * apw - 1) // (4 * apw))
    is_tapered = apw >= 2 and launch["grid"] != untapered
    assert is_tapered == tapered, (f"planner moved case {M}x{A} {env}: launch {launch}, untapered grid {untapered}; "
                                   "update TAPER_CASES so that the matrix still meets the tapered and the untapered form")
    if "FO_SWEEP_APW" in env:
        assert apw == int(env["FO_SWEEP_APW"])


# ------------------------------------------------------------------------------------------ exact ties, threshold equality
def _tie_batch(M=70, T=31):
    """a stationary ego (after 5 samples far away) beside stationary agents: from sample 5 on every sample gives the
    bit-identical CP, harm and risk.  Agents 2, 5, 8 are identical copies (in different waves of one workgroup), the
    others sit elsewhere; agent 0 is far away"""
    from frenetix_occlusion import synthetic as S
    ag = S.make_agents(9, T, 0.1, seed=3)
    ex = np.where(np.arange(T) < 5, -200.0, 0.0)[None, :] + np.linspace(0, 0.9, M)[:, None] * (np.arange(T) >= 5)
    traj = {"x": ex, "y": np.full((M, T), 1.0), "theta": np.zeros((M, T)), "v": np.zeros((M, T)), "a": np.zeros((M, T))}
    rng = np.random.default_rng(4)
    for k in range(9):
        if k == 0:
            p = (400.0, 400.0)
        elif k in (2, 5, 8):
            p = (3.0, 3.0)
        else:
            p = (rng.uniform(-8.0, -5.0), rng.uniform(-2.0, 4.0))      # farther from the ego than the tied copies
        ag["pos"][k] = p
        ag["yaw"][k] = np.pi / 2 if k in (2, 5, 8) else rng.uniform(-3, 3)
        ag["v"][k] = 0.0
        ag["cov"][k] = np.array([[1.5, 0.0], [0.0, 2.0]]) if k != 7 else np.array([[1.5, 0.4], [0.4, 2.0]])
        ag["shape"][k], ag["raw_dims"][k], ag["type"][k] = ag["shape"][2], ag["raw_dims"][2], ag["type"][2]
    ag["len"][:] = T
    return traj, ag


@pytest.mark.parametrize("form,env", KERNEL_FORMS, ids=[f[0] for f in KERNEL_FORMS])
def test_bit_identical_maxima_take_the_first_index(torch_cuda, oracle, monkeypatch, form, env):
    from frenetix_occlusion import synthetic as S
    from frenetix_occlusion import _native as N
    traj, agents = _tie_batch()
    ref = oracle.sweep(traj, agents, S.VEHICLE_BMW320I, 0.1, thr={"ttc": 1.0})
    cp = ref["lists"][:, :, N.LST["cp"], :]
    orisk = ref["lists"][:, :, N.LST["obst_risk"], :]
    # the batch is what it claims: bit-identical plateaus from sample 5 on, the maxima ON them, tied agents
    assert (cp[:, 2, 4:] == cp[:, 2, 4:5]).all() and (cp[:, 2, 4] > 0).all() and (cp[:, 2, :4] == 0).all()
    assert (orisk[:, 2, 4:] == orisk[:, 2, 4:5]).all()
    assert (ref["pair_i"][:, 2, N.PI["cp_argmax"]] == 4).all() and (ref["pair_i"][:, 2, N.PI["max_obst_risk_index"]] == 4).all()
    for k in (5, 8):
        assert np.array_equal(ref["pair_f"][:, k], ref["pair_f"][:, 2], equal_nan=True)
    dce = ref["pair_f"][..., N.PF["dce"]]
    assert (dce.min(axis=1) == dce[:, 2]).all()
    assert (ref["cost"][:, N.COST["argmin_dce"]] == np.argmin(dce, axis=1)).all()
    _set_env(monkeypatch, env)
    for lists in ("f64", "f32x"):
        got = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr={"ttc": 1.0}, lists=lists)
        for name in ("cp_argmax", "max_obst_risk_index", "time_dce"):
            assert np.array_equal(got["pair_i"][..., N.PI[name]], ref["pair_i"][..., N.PI[name]]), (form, lists, name)
        for name in ("argmin_dce", "argmin_ttc", "argmax_risk"):
            assert np.array_equal(got["cost"][:, N.COST[name]], ref["cost"][:, N.COST[name]]), (form, lists, name)
        if lists == "f64":
            _compare(oracle, ref, got)
    red = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr={"ttc": 1.0}, mode="reduced")
    for name in ("argmin_dce", "argmin_ttc", "argmax_risk"):
        assert np.array_equal(red["cost"][:, N.COST[name]], ref["cost"][:, N.COST[name]]), (form, "reduced", name)


@pytest.mark.parametrize("mode", ["full", "reduced"])
def test_thresholds_equal_to_the_devices_own_values(torch_cuda, monkeypatch, mode):
    """`safe` with a threshold set to exactly the device's own per-trajectory value and to its neighbouring doubles:
    harm / risk / cp are unsafe above (`>`), ttc / dce below (`<`) (metric.py:58-95).  `reduced` decides in the reduction
    kernel, a code path of its own"""
    from frenetix_occlusion import synthetic as S
    from frenetix_occlusion import _native as N
    _set_env(monkeypatch, {})
    traj, agents = S.make_batch(300, 16, config_id=2)
    base = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1)
    c = base["cost"]
    checks = {"harm": ("max_obst_harm_with_cp_all", "gt"), "risk": ("max_obst_risk_all", "gt"),
              "cp": ("max_collision_probability_all", "gt"), "ttc": ("wttc", "lt"), "dce": ("min_dce", "lt")}
    n = 0
    for key, (col, op) in checks.items():
        vals = c[:, N.COST[col]]
        fin = np.unique(vals[np.isfinite(vals) & (vals > 0)])
        assert len(fin) >= 3, key
        for v in (fin[len(fin) // 2], fin[-1], fin[0]):
            for thr in (v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)):
                got = _hip_sweep(torch_cuda, traj, agents, S.VEHICLE_BMW320I, 0.1, thr={key: float(thr)}, mode=mode)
                want = ~(vals > thr) if op == "gt" else ~(vals < thr)
                assert np.array_equal(got["safe"].astype(bool), want), (mode, key, thr)
                n += 1
    assert n == 45
