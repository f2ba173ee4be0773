"""The device's brake evaluation (fo_be_prep_kernel, fo_be_kernel, the max_btn fold of fo_reduce_kernel:
csrc/fo_sweep_be_reduce.hpp) on the cases of tests/brake_evaluation_cases.py, whose reference side is proven on the host in
tests/test_brake_evaluation_cpu.py.  Every test runs in three kernel forms (the library's own choice, FO_SWEEP_SPLIT=0,
FO_SWEEP_GENERIC=1): all of them feed the brake kernel through be_mask.

* exact touch and known answers: be_decel, be_btn, max_btn and `safe` with `==` against the exact reference, in `full` and in
  `reduced` mode; all touch agents in one launch (two tiles, 188 blocks of four agents);
* a `be` threshold equal to the device's own max_btn (safe) and one ulp below it (unsafe), the deciding agent in every wave
  residue and block row of the reduction;
* the smallest and oddest shapes against the oracle: exact outside the near-touch band G, the NaN pattern, be_btn == be_decel
  / a_max, max_btn == the row maximum, `reduced` bit-equal to `full`;
* the retained buffers: four runs of different size and activity on one context, each bit-equal to a fresh context's;
* the fused planning step with `be` selected against a MetricSweep over the agents it spawned.

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import brake_evaluation_cases as K
import ref_brake_evaluation as R
from test_sweep_gate_gpu import _set_env
from test_sweep_gpu import _hip_sweep

pytestmark = pytest.mark.gpu

FORMS = [("default", {}), ("no split", {"FO_SWEEP_SPLIT": "0"}), ("generic", {"FO_SWEEP_GENERIC": "1"})]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


@pytest.fixture(autouse=True, params=FORMS, ids=[f[0] for f in FORMS])
def kernel_form(request, monkeypatch):
    _set_env(monkeypatch, request.param[1])
    return request.param[0]


def _exact(want, got, what):
    bad = np.argwhere(~((want == got) | (np.isnan(want) & np.isnan(got))))
    assert len(bad) == 0, (f"{what}: differs at {len(bad)} places, e.g. {bad[:8].tolist()}: got "
                           f"{[float(got[tuple(b)]) for b in bad[:8]]}, want {[float(want[tuple(b)]) for b in bad[:8]]}")


def _check_exact_case(torch, O, case, expected, form):
    """be_decel / be_btn / max_btn / safe of a dyadic case against `expected` [M, A] with ==, full and reduced"""
    a_max = case["veh"][4]
    btn = expected / a_max                                    # (a_max = 8: exact)
    max_btn = np.fmax.reduce(btn, axis=1, initial=0.0)
    levels = np.unique(max_btn)
    thr = float(levels[(len(levels) - 1) // 2])               # one of the rows' own maxima: `>` keeps those rows safe
    want_safe = (~(max_btn > thr)).astype(np.uint8)
    assert 0 < want_safe.mean() < 1
    full = _hip_sweep(torch, case["traj"], case["agents"], case["veh"], case["dt"], metrics=K.METRICS, thr={"be": thr})
    _exact(expected, full["pair_f"][..., O.PF["be_decel"]], f"{form} be_decel")
    _exact(btn, full["pair_f"][..., O.PF["be_btn"]], f"{form} be_btn")
    red = _hip_sweep(torch, case["traj"], case["agents"], case["veh"], case["dt"], metrics=K.METRICS, thr={"be": thr}, mode="reduced")
    for mode, out in (("full", full), ("reduced", red)):
        _exact(max_btn, out["cost"][:, O.COST["max_btn"]], f"{form} {mode} max_btn")
        _exact(want_safe, out["safe"], f"{form} {mode} safe")
        _exact(want_safe.astype(np.float64), out["cost"][:, O.COST["safe"]], f"{form} {mode} cost.safe")
    assert np.array_equal(red["cost"], full["cost"], equal_nan=True)
    return full


def test_exact_touch(torch_cuda, oracle, kernel_form):
    tc = K.touch()
    M = tc["traj"]["x"].shape[0]
    expected = tc["expected"][np.arange(M) % 2]
    assert tc["flips"] >= 20 and M > 64 and expected.shape[1] > 64      # more than one tile, many blocks of four agents
    _check_exact_case(torch_cuda, oracle, tc, expected, kernel_form)


def test_known_answers(torch_cuda, oracle, kernel_form):
    kn = K.known_answers()
    full = _check_exact_case(torch_cuda, oracle, kn, kn["expected"], kernel_form)
    decel = full["pair_f"][..., oracle.PF["be_decel"]]
    for m, k, want, what in kn["literal"]:
        assert decel[m, k] == want or (np.isnan(want) and np.isnan(decel[m, k])), (kernel_form, what, decel[m, k], want)
    assert np.isnan(full["pair_f"][:, 4, :]).all()            # no prediction: NaN pair rows, and nothing in the maximum


@pytest.mark.parametrize("slot", [0, 3, 4, 7, 8, 16])
def test_threshold_equal_to_the_brake_threat_number(torch_cuda, oracle, kernel_form, slot):
    """metric.py:54-61 `>`: safe at thr == max_btn, unsafe one ulp below.  17 agents, the deciding one in slot 0 / 3 / 4 / 7 / 8
    / 16: every `k % 8` wave of the reduction's fold that holds more or fewer agents than its neighbours, and every row of the
    brake kernel's blocks of four"""
    front = K.VEH[2] + K.VEH[0] / 2
    others = [((18.3046875 + 0.5 * (k % 5), 0.0), (0.5, 0.5), K.T) if k % 3 else ((20.0, 6.0), (0.5, 0.5), K.T) for k in range(16)]
    rows = others[:slot] + [((front + 0.75, 0.0), (0.5, 0.5), K.T)] + others[slot:]
    agents = K.agents_dict(rows, K.T)
    traj = K.straight_rows([8.0] * 65)
    btn = K.ALL_HIT / K.VEH[4]
    full = _hip_sweep(torch_cuda, traj, agents, K.VEH, K.DT, metrics=K.METRICS, thr={"be": btn})
    got = full["pair_f"][..., oracle.PF["be_btn"]]
    assert (got[:, slot] == btn).all() and (np.delete(got, slot, axis=1) < btn).all() and (np.delete(got, slot, axis=1) > 0).any()
    assert (full["safe"] == 1).all() and (full["cost"][:, oracle.COST["max_btn"]] == btn).all(), (kernel_form, slot)
    for thr, mode, safe in ((btn, "reduced", 1), (float(np.nextafter(btn, 0)), "reduced", 0), (float(np.nextafter(btn, 0)), "full", 0)):
        out = _hip_sweep(torch_cuda, traj, agents, K.VEH, K.DT, metrics=K.METRICS, thr={"be": thr}, mode=mode)
        assert (out["cost"][:, oracle.COST["max_btn"]] == btn).all(), (kernel_form, slot, mode)
        assert (out["safe"] == safe).all(), (kernel_form, slot, thr, mode)


def test_shapes_match_the_oracle(torch_cuda, oracle, kernel_form):
    O = oracle
    inside, n_active = [], 0
    for b in K.shapes(O):
        what = f"{kernel_form} {b['shape']}"
        full = _hip_sweep(torch_cuda, b["traj"], b["agents"], b["veh"], b["dt"], metrics=K.METRICS, thr={"be": 0.2})
        ref = b["ref"]
        want, got = ref["pair_f"][..., O.PF["be_decel"]], full["pair_f"][..., O.PF["be_decel"]]
        btn = full["pair_f"][..., O.PF["be_btn"]]
        assert np.array_equal(np.isnan(want), np.isnan(got)), what
        assert np.array_equal(np.isnan(ref["pair_f"]), np.isnan(full["pair_f"])), what
        band = b["active"] & ~(b["min_abs_sep"] > K.G)
        _exact(np.where(band, 0.0, want), np.where(band, 0.0, got), f"{what} be_decel")
        for m, k in np.argwhere(band):          # near touch: the oracle's node or the one a predicate G to either side gives
            tr, ag = K.row(b["traj"], m), K.agent(b["agents"], k)
            ag["len"] = min(ag["len"], b["shape"][3])
            either = {want[m, k]} | {R.be_float(tr, ag, b["veh"], b["dt"], slack=s)[0] for s in (-K.G, K.G)}
            inside.append((b["shape"], int(m), int(k), float(got[m, k]), sorted(either)))
            assert got[m, k] in either, inside
        _exact(got / b["veh"][4], btn, f"{what} be_btn")
        assert np.array_equal(btn > 0, b["active"]), what
        _exact(np.fmax.reduce(btn, axis=1, initial=0.0), full["cost"][:, O.COST["max_btn"]], f"{what} max_btn")
        if not band.any():
            _exact(ref["cost"][:, O.COST["max_btn"]], full["cost"][:, O.COST["max_btn"]], f"{what} max_btn against the oracle")
            _exact(ref["safe"], full["safe"], f"{what} safe")
        red = _hip_sweep(torch_cuda, b["traj"], b["agents"], b["veh"], b["dt"], metrics=K.METRICS, thr={"be": 0.2}, mode="reduced")
        assert np.array_equal(red["cost"], full["cost"], equal_nan=True) and np.array_equal(red["safe"], full["safe"]), what
        n_active += int(b["active"].sum())
    assert n_active >= 200 and len(inside) <= 0.01 * n_active, inside


def _run(torch, sw, traj, agents=None):
    if agents is not None:
        sw.set_agents(*[agents[k] for k in K.AGENT_KEYS])
    out = sw.run(traj["x"], traj["y"], traj["theta"], traj["v"], traj["a"], mode="full")
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (out.cost, out.safe, out.pair_f, out.pair_i)]


def test_retained_buffers_on_one_context(torch_cuda, oracle, kernel_form):
    """d_be_mask, d_be_btn and d_be_dist outlive a run (fo_reserve): 129 candidates with every pair colliding, then one, then 65
    with nothing colliding, then a larger agent set -- each bit-equal to the same run on a fresh context"""
    from frenetix_occlusion.sweep import MetricSweep
    few = K.agents_dict([((12.0 + 1.5 * k, 0.0), (0.5, 0.5), K.T) for k in range(5)], K.T)
    many = K.agents_dict([((9.0 + 0.75 * k, 0.0 if k % 2 else 1.0), (0.5, 0.5), K.T - k) for k in range(17)], K.T)
    lane = K.straight_rows([8.0 - 0.03125 * m for m in range(129)])
    away = {k: v[:65].copy() for k, v in lane.items()}
    away["y"] += 64.0
    runs = ((lane, few), ({k: v[:1] for k, v in lane.items()}, None), (away, None), ({k: v[:65] for k, v in lane.items()}, many))
    thr = {"be": 0.3}
    sw = MetricSweep(K.VEH, K.DT, metrics=K.METRICS, thresholds=thr)
    got = [_run(torch_cuda, sw, traj, agents) for traj, agents in runs]
    current = None
    for i, (traj, agents) in enumerate(runs):
        current = agents or current
        fresh = _run(torch_cuda, MetricSweep(K.VEH, K.DT, metrics=K.METRICS, thresholds=thr), traj, current)
        for a, b in zip(got[i], fresh):
            assert np.array_equal(a, b, equal_nan=True), (kernel_form, i)
    btn = [g[2][oracle.PF["be_btn"]] for g in got]
    assert (btn[0] > 0).all() and (btn[1] > 0).all() and (btn[2] == 0).all() and (btn[3] > 0).any()
    assert got[2][1].all() and not got[0][1].all()


def test_fused_step_with_brake_evaluation(torch_cuda, oracle, kernel_form):
    """PlanningStep / fo_step_run takes the tile table from the ray kernel; with `be` selected its max_btn and `safe` (and
    the pair columns) equal, bit for bit, a MetricSweep.run over the agents the step spawned"""
    torch = torch_cuda
    import test_rules_step_gpu as RS
    from frenetix_occlusion.sweep import DEFAULT_METRICS, MetricSweep
    metrics, thr = DEFAULT_METRICS + ("be",), {"be": 0.3}
    n_btn = n_unsafe = 0
    for name, lanelets, obstacles, path, ego, yaw, v, inter, step in RS._scenes()[:4]:
        k = RS._stack(torch, lanelets, obstacles, path, inter, step, ego=ego, yaw=yaw)
        k.sw.configure(RS.VEH, thresholds=thr, metrics=metrics)
        k.sm.upload_obstacles(k.obs)
        out = k.step().run(ego, yaw, v)                        # (the step holds x, y, theta, v and a)
        torch.cuda.synchronize()
        sw2 = MetricSweep(RS.VEH, 0.1, metrics=metrics, thresholds=thr)
        sw2.set_agents(*k.sl.batch.sweep_args(), check=False)
        ref = sw2.run(*k.tr, mode="pair")
        torch.cuda.synchronize()
        c, rc = out.cost.cpu().numpy(), ref.cost.cpu().numpy()
        assert np.array_equal(c[:, oracle.COST["max_btn"]], rc[:, oracle.COST["max_btn"]]), (kernel_form, name)
        assert np.array_equal(out.safe.cpu().numpy(), ref.safe.cpu().numpy()), (kernel_form, name)
        pf, rf = out.pair_f.cpu().numpy(), ref.pair_f.cpu().numpy()
        for col in ("be_decel", "be_btn", "ttc"):
            assert np.array_equal(pf[oracle.PF[col]], rf[oracle.PF[col]], equal_nan=True), (kernel_form, name, col)
        n_btn += int((c[:, oracle.COST["max_btn"]] > 0).sum())
        n_unsafe += int((c[:, oracle.COST["max_btn"]] > thr["be"]).sum())
    assert n_btn > 0, "no candidate of any scene meets a spawned agent: the comparison says nothing about be"
    print(f"{kernel_form}: {n_btn} candidates with a brake threat number, {n_unsafe} above the threshold")
