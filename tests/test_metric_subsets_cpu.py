"""The reference side of tests/test_metric_subsets_gpu.py, pinned without a GPU (cases: tests/metric_subset_cases.py):

* the dependency closure leaves 33 selections, and the three statements of it -- the oracle's `fo_oracle_required_metrics`,
  oracle/fo_numpy_ref.py's `Metric` and what the reference's own class reported in tests/golden/thresholds.npz -- agree;
* for each of them the oracle's output is its all-seven output restricted to the evaluated metrics, bit for bit, with the
  neutral values of the table below everywhere else;
* fo_numpy_ref computes the same values as the oracle on the selections it knows (all without 'be');
* the batch keeps every metric busy and each threshold splits it."""
import itertools

import numpy as np
import pytest

import metric_subset_cases as K
from test_sweep_gpu import ATOL, _cp_plateau


@pytest.fixture(scope="module")
def case(oracle):
    return K.oracle_case(oracle)


@pytest.fixture(scope="module")
def sels(oracle):
    return K.selections(oracle)


def test_the_closure_leaves_33_selections(oracle, sels):
    O = oracle
    assert len(sels) == K.N_SELECTIONS == 33
    assert sels[0] == ((), 0)                                                     # the empty one included
    assert all(K.closed_mask(O, names) == m == K.closed_mask(O, K.mask_names(O, m)) for names, m in sels)
    raw = [K.closed_mask(O, n) for r in range(8) for n in itertools.combinations(K.NAMES, r)]
    assert len(raw) == 128 and set(raw) == {m for _, m in sels}
    in_kernel = O.metric_mask(("dce", "cp", "ttc", "ttce", "hr"))                # wttc and be act outside the sweep kernel
    assert len({m & in_kernel for _, m in sels}) == 15
    assert sum(1 for _, m in sels if not m & O.METRIC_BITS["be"]) == 21
    assert sum(1 for _, m in sels if m & in_kernel == in_kernel) == 4            # the compile-time metric set, +- wttc, +- be
    assert K.closed_mask(O, ("hr", "ttc")) in {m for _, m in sels}               # BASELINE config 1


def test_the_host_layers_ordering_agrees_with_the_closure(oracle):
    """metrics/metric.py's check_required_metrics orders the result dict; 'be' does not pull 'ttc' into that list (the
    reference's be.py:39 raises KeyError there), the library evaluates it all the same"""
    from frenetix_occlusion.metrics.metric import check_required_metrics
    for r in range(8):
        for names in itertools.combinations(K.NAMES, r):
            host = set(check_required_metrics(list(names)))
            if "be" in names:
                host.add("ttc")
            assert host == set(K.mask_names(oracle, K.closed_mask(oracle, names))), names


def test_the_batch_keeps_every_metric_busy_and_each_threshold_splits_it(oracle, case):
    O = oracle
    traj, agents, veh, dt, thr, ref = case
    assert ref["pair_f"].shape == (K.M, K.A, O.NPF) and ref["lists"].shape == (K.M, K.A, O.NL, K.T - 1)
    c, pf = ref["cost"], ref["pair_f"]
    fin_ttc = np.isfinite(c[:, O.COST["wttc"]]).mean()
    assert 0.25 < fin_ttc < 0.75, fin_ttc                                         # colliding and collision-free candidates
    ttc = pf[..., O.PF["ttc"]]
    assert (np.isfinite(ttc) & (ttc > 0)).sum() >= 50                             # BE is active (be.py:49-50)
    assert (pf[..., O.PF["be_btn"]] > 0).sum() >= 50
    assert (ref["lists"][:, :, O.LST["cp"], :] > 0).sum() >= 1000                 # the gate is open
    assert len(np.unique(c[:, O.COST["min_dce"]])) >= 20
    assert set(thr) == set(K.THR_KEYS) and thr["dce"] == 0.05
    assert all(np.isfinite(v) and v > 0 for v in thr.values()), thr
    for key in K.THR_KEYS:
        share = float(K.oracle_run(O, K.NAMES, {key: thr[key]})["safe"].mean())
        assert K.SAFE_SHARE[0] <= share <= K.SAFE_SHARE[1], (key, thr[key], share)
    both = K.oracle_run(O, K.NAMES)["safe"].mean()
    assert 0 < both < 1, both


def test_neutral_values_of_a_metric_that_is_not_evaluated(oracle, case):
    """the table, column by column, on the empty selection: metric.py:44 returns ({}, True) there"""
    O = oracle
    out = K.oracle_run(O, ())
    assert np.isnan(out["pair_f"]).all() and not out["pair_i"].any() and np.isnan(out["lists"]).all()
    assert (out["safe"] == 1).all() and (out["cost"][:, O.COST["safe"]] == 1).all()
    table = {"wttc": np.inf, "min_dce": np.inf, "min_ttce": np.inf, "max_ego_risk_all": 0.0, "max_obst_risk_all": 0.0,
             "max_ego_harm_all": 0.0, "max_obst_harm_all": 0.0, "max_collision_probability_all": 0.0,
             "max_obst_harm_with_cp_all": 0.0, "max_btn": 0.0, "argmin_dce": -1.0, "argmin_ttc": -1.0, "argmax_risk": -1.0}
    assert table == K.COST_NEUTRAL and set(table) | {"safe"} == set(O.COST)
    for name, v in table.items():
        assert (out["cost"][:, O.COST[name]] == v).all(), name
    assert not out["cost"][:, len(O.COST):].any()                                 # the reserved columns


def test_the_oracle_restricted_is_the_oracle_on_the_selection(oracle, case, sels):
    O = oracle
    traj, agents, veh, dt, thr, ref_all = case
    for names, mask in sels:
        for t in (thr, None):
            out = K.oracle_run(O, names, t)
            want = K.restrict(O, ref_all, mask, t)
            for k in ("pair_f", "pair_i", "lists", "cost", "safe"):
                assert K.bit_equal(out[k], want[k]), (names, k, "thresholds" if t else "no thresholds")
        # ... and said once more without the helper: whatever a metric outside the closure owns is neutral
        off = lambda owner: not mask & O.METRIC_BITS[owner]
        for name, owner in K.PAIR_F_OWNER.items():
            assert np.isnan(out["pair_f"][..., O.PF[name]]).all() == off(owner), (names, name)
        for name, owner in K.LIST_OWNER.items():
            assert np.isnan(out["lists"][:, :, O.LST[name], :]).all() == off(owner), (names, name)
        for name, owner in K.COST_OWNER.items():
            if off(owner):
                assert (out["cost"][:, O.COST[name]] == K.COST_NEUTRAL[name]).all(), (names, name)
        if off("hr"):
            assert not out["pair_i"][..., O.PI["hr_valid"]].any()


# ------------------------------------------------------------------------------------------------ fo_numpy_ref
def _numpy_ref_arrays(O, results, A, Tm1):
    """fo_numpy_ref's per-trajectory result dicts in the oracle's layout; what a selection does not evaluate stays neutral"""
    M = len(results)
    pf = np.full((M, A, O.NPF), np.nan)
    pi = np.zeros((M, A, O.NPI), dtype=np.int32)
    lists = np.full((M, A, O.NL, Tm1), np.nan)
    cost = {n: np.full(M, v) for n, v in K.COST_NEUTRAL.items()}
    for m, r in enumerate(results):
        for k, d in r.get("dce", {}).items():
            pf[m, k, O.PF["dce"]], pi[m, k, O.PI["time_dce"]] = d["dce"], d["time_dce"]
        for name in ("ttc", "ttce"):
            for k, v in r.get(name, {}).items():
                pf[m, k, O.PF[name]] = v
        for k, v in r.get("cp", {}).items():
            lists[m, k, O.LST["cp"], :] = v
        if "dce" in r:
            cost["min_dce"][m] = min(d["dce"] for d in r["dce"].values())
        if "ttc" in r:
            cost["wttc"][m] = min(r["ttc"].values())
        if "wttc" in r:
            assert r["wttc"] == cost["wttc"][m]
        if "ttce" in r:
            cost["min_ttce"][m] = min(r["ttce"].values())
        for k, d in r.get("hr", {}).items():
            if not isinstance(d, dict):
                cost[k][m] = d
                continue
            for name in ("max_ego_risk", "max_obst_risk", "max_obst_harm_with_cp", "max_ego_harm", "max_obst_harm",
                         "max_collision_probability"):
                pf[m, k, O.PF[name]] = d[name]
            pi[m, k, O.PI["max_obst_risk_index"]], pi[m, k, O.PI["hr_valid"]] = d["max_obst_risk_index"], 1
            pi[m, k, O.PI["cp_argmax"]] = int(np.argmax(d["collision_probability"]))        # hr.py:81
            for name in ("ego_harm", "obst_harm", "ego_risk", "obst_risk"):
                v = np.asarray(d[name + "_traj"], dtype=np.float64)
                lists[m, k, O.LST[name], :len(v)] = v
    return pf, pi, lists, cost


def test_the_closure_three_ways_and_fo_numpy_ref_agrees_with_the_oracle(oracle, case, sels):
    from golden_util import load_threshold_case
    from oracle import fo_numpy_ref as R
    O = oracle
    traj, agents, veh, dt, thr, _ = case
    # the reference's own class (thresholds.npz) = the oracle's closure = fo_numpy_ref's ordering
    recorded = load_threshold_case()[4]
    assert len(recorded) >= 6
    for activated, _, evaluated, _ in recorded:
        assert sorted(K.mask_names(O, K.closed_mask(O, activated))) == evaluated, activated
        if "be" not in activated:
            assert sorted(n for n, _ in R.Metric(veh, dt, activated).metrics) == evaluated, activated
    nthr = {k: v for k, v in thr.items() if k != "be"}
    done = 0
    for names, mask in sels:
        if mask & O.METRIC_BITS["be"]:
            continue                        # (fo_numpy_ref has no brake evaluation)
        # (fo_numpy_ref walks trajectory by trajectory in Python: 4 s per selection, the slow test of this file)
        rows = slice(None)
        results, safe = R.sweep({k: v[rows] for k, v in traj.items()}, agents, veh, dt, metrics=names, thr=nthr)
        want = set(K.mask_names(O, mask))
        assert all(set(r) == want for r in results), names                       # the keys the Metric class produces
        ref = {k: v[rows] for k, v in K.oracle_run(O, names, nthr).items()}
        assert np.array_equal(safe, ref["safe"]), names
        pf, pi, lists, cost = _numpy_ref_arrays(O, results, K.A, K.T - 1)
        for k, a, b in (("pair_f", ref["pair_f"], pf), ("lists", ref["lists"], lists)):
            assert np.array_equal(np.isnan(a), np.isnan(b)), (names, k)
            assert np.array_equal(np.isinf(a), np.isinf(b)), (names, k)
        # max_obst_harm_with_cp = obst_harm[argmax cp] jumps where several samples hold the maximum within rounding:
        # _compare's plateau rule (the harm at the index fo_numpy_ref picked), for that one column and nothing else
        plateau = _cp_plateau(O, ref, {"pair_f": pf, "pair_i": pi}, ATOL)
        fin = np.isfinite(ref["pair_f"])
        fin[..., O.PF["max_obst_harm_with_cp"]] &= ~plateau
        np.testing.assert_allclose(pf[fin], ref["pair_f"][fin], rtol=0, atol=ATOL, err_msg=str(names))
        fin = np.isfinite(ref["lists"])
        np.testing.assert_allclose(lists[fin], ref["lists"][fin], rtol=0, atol=ATOL, err_msg=str(names))
        for name in ("time_dce", "hr_valid"):
            assert np.array_equal(pi[..., O.PI[name]], ref["pair_i"][..., O.PI[name]]), (names, name)
        sure = ~plateau & (ref["pair_i"][..., O.PI["hr_valid"]] > 0) & (ref["pair_f"][..., O.PF["max_collision_probability"]] > 1e-9)
        assert np.array_equal(pi[..., O.PI["cp_argmax"]][sure], ref["pair_i"][..., O.PI["cp_argmax"]][sure]), names
        for name, col in cost.items():
            if name.startswith("arg") or name == "max_btn":
                continue
            a = ref["cost"][:, O.COST[name]]
            assert np.array_equal(np.isinf(a), np.isinf(col)), (names, name)
            fin = np.isfinite(a) & ~(plateau.any(axis=1) & (name == "max_obst_harm_with_cp_all"))
            np.testing.assert_allclose(col[fin], a[fin], rtol=0, atol=ATOL, err_msg=f"{names} {name}")
        done += 1
    assert done == 21


# ------------------------------------------------------------------------------------------------ compare_total
def _copy(out):
    return {k: v.copy() for k, v in out.items()}


def test_compare_total_accepts_the_oracle_and_misses_no_output(oracle, case, sels):
    """the comparison the GPU test relies on: passes on equal outputs of every selection, and fails on one wrong element of
    each kind of output -- the ones tests/test_sweep_gpu.py's _compare leaves out among them"""
    O = oracle
    for names, _ in sels:
        ref = K.oracle_run(O, names)
        assert K.compare_total(O, ref, _copy(ref)) == 0.0
    ref = K.oracle_run(O, K.NAMES)
    PF, PI, C, LST = O.PF, O.PI, O.COST, O.LST
    risk = ref["cost"][:, C["max_obst_risk_all"]]
    m_risk = int(np.argmax(risk))
    assert risk[m_risk] > 1e-3
    btn = ref["pair_f"][..., PF["be_btn"]]
    m_b, k_b = (int(q) for q in np.argwhere(btn > 0)[0])
    inf_ttc = np.argwhere(np.isinf(ref["pair_f"][..., PF["ttc"]]))[0]

    def bump(key, idx, value):
        def f(out):
            out[key][idx] = value(out[key][idx]) if callable(value) else value
        return f
    breaks = {
        "be_btn": bump("pair_f", (m_b, k_b, PF["be_btn"]), lambda v: v + 1e-6),
        "be_decel": bump("pair_f", (m_b, k_b, PF["be_decel"]), lambda v: v + 1e-6),
        "max_btn": bump("cost", (m_b, C["max_btn"]), lambda v: v + 1e-6),
        "argmax_risk": bump("cost", (m_risk, C["argmax_risk"]), lambda v: (v + 1) % K.A),
        "cost NaN": bump("cost", (3, C["max_ego_harm_all"]), np.nan),
        "cost -inf": bump("cost", (int(np.argwhere(np.isinf(ref["cost"][:, C["wttc"]]))[0, 0]), C["wttc"]), -np.inf),
        "reserved column": bump("cost", (0, 15), 1.0),
        "spare pair column": bump("pair_f", (0, 0, 11), 0.0),
        "ttc -inf": bump("pair_f", (inf_ttc[0], inf_ttc[1], PF["ttc"]), -np.inf),
        "dce by less than atol": bump("pair_f", (5, 5, PF["dce"]), lambda v: v + 1e-10),
        "min_dce by less than atol": bump("cost", (5, C["min_dce"]), lambda v: v + 1e-10),
        "list beyond the harm length": bump("lists", (0, 1, LST["ego_harm"], 5), 0.25),
        "list": bump("lists", (0, 0, LST["obst_risk"], 7), lambda v: v + 1e-8),
        "hr_valid": bump("pair_i", (0, 0, PI["hr_valid"]), 0),
        "cp_argmax out of range": bump("pair_i", (0, 0, PI["cp_argmax"]), K.T - 1),
        "safe": bump("safe", (0,), lambda v: 1 - v),
    }
    for what, f in breaks.items():
        got = _copy(ref)
        f(got)
        with pytest.raises(AssertionError):
            K.compare_total(O, ref, got)
            pytest.fail(f"compare_total passed a wrong {what}", pytrace=False)
    # a metric that is not evaluated: the reference holds NaN, a number on the device side must not pass
    ref = K.oracle_run(O, ("dce",))
    for key, idx in (("pair_f", (0, 0, PF["ttc"])), ("pair_f", (0, 0, PF["max_obst_risk"])), ("lists", (0, 0, LST["cp"], 0))):
        got = _copy(ref)
        assert np.isnan(got[key][idx])
        got[key][idx] = 0.0
        with pytest.raises(AssertionError):
            K.compare_total(O, ref, got)
