"""Cases shared by tests/test_metric_subsets_cpu.py and tests/test_metric_subsets_gpu.py: every metric selection a caller's
`activated_metrics` can amount to, one batch that keeps every metric busy, thresholds inside the range of the batch's own
values, which output belongs to which metric, and a comparison that leaves no output out.  NumPy and the CPU oracle only.

The dependency closure (metric.py:125-147; `fo_oracle_required_metrics`) maps the 128 subsets of the seven metric names
onto 33 closed selections, the empty one included.  The queue kernel tells 15 of them apart (dce / ttc / ttce x cp / hr);
'wttc' and 'be' act outside it (the reduction's thresholds, the brake kernel)."""
import itertools

import numpy as np

from test_sweep_gpu import ATOL, _assert_argmax, _compare, _cp_plateau

NAMES = ("dce", "cp", "ttc", "ttce", "wttc", "be", "hr")
N_SELECTIONS = 33
M, A, T, DT = 130, 9, 31, 0.1      # three tiles (the last with two live lanes), three chunks of four agents (dead waves)
AGENT_LEN = (31, 1, 2, 30, 17, 31, 5, 29, 3)
THR_KEYS = ("harm", "risk", "cp", "ttc", "dce", "be")
SAFE_SHARE = (0.1, 0.9)            # every single-threshold run of the oracle must leave both verdicts common

# ---------------------------------------------------------------------------------------- which output is whose
# the metric that writes an output; everything the metric's absence leaves behind is the neutral value below
PAIR_F_OWNER = {"dce": "dce", "ttc": "ttc", "ttce": "ttce", "max_ego_risk": "hr", "max_obst_risk": "hr",
                "max_obst_harm_with_cp": "hr", "max_ego_harm": "hr", "max_obst_harm": "hr",
                "max_collision_probability": "hr", "be_decel": "be", "be_btn": "be"}
PAIR_I_OWNER = {"time_dce": "dce", "max_obst_risk_index": "hr", "cp_argmax": "hr", "hr_valid": "hr"}
LIST_OWNER = {"cp": "cp", "ego_harm": "hr", "obst_harm": "hr", "ego_risk": "hr", "obst_risk": "hr"}
# (the 'wttc' column holds the smallest ttc whenever ttc is evaluated, with or without 'wttc' in the list: wttc.py:32-42 only
# names it)
COST_OWNER = {"wttc": "ttc", "min_dce": "dce", "max_ego_risk_all": "hr", "max_obst_risk_all": "hr", "max_ego_harm_all": "hr",
              "max_obst_harm_all": "hr", "max_collision_probability_all": "hr", "max_obst_harm_with_cp_all": "hr",
              "min_ttce": "ttce", "argmin_dce": "dce", "argmin_ttc": "ttc", "argmax_risk": "hr", "max_btn": "be"}
# what a cost column holds when its metric is not evaluated: +inf for minima, 0 for maxima, -1 for indices
COST_NEUTRAL = {"wttc": np.inf, "min_dce": np.inf, "min_ttce": np.inf,
                "max_ego_risk_all": 0.0, "max_obst_risk_all": 0.0, "max_ego_harm_all": 0.0, "max_obst_harm_all": 0.0,
                "max_collision_probability_all": 0.0, "max_obst_harm_with_cp_all": 0.0, "max_btn": 0.0,
                "argmin_dce": -1.0, "argmin_ttc": -1.0, "argmax_risk": -1.0}
PAIR_F_NEUTRAL, PAIR_I_NEUTRAL, LIST_NEUTRAL = np.nan, 0, np.nan
# outputs both sides round to the millimetre or to the step (dce.py:79, ttc.py:43-46, ttce.py:39) or count: exact
EXACT_PAIR_F = ("dce", "ttc", "ttce")
EXACT_PAIR_I = ("time_dce", "hr_valid")
EXACT_COST = ("argmin_dce", "argmin_ttc", "min_dce", "min_ttce", "wttc", "safe")


def closed_mask(O, names):
    return int(O.lib().fo_oracle_required_metrics(O.metric_mask(names)))


def mask_names(O, mask):
    return tuple(n for n in NAMES if mask & O.METRIC_BITS[n])


def selections(O):
    """[(name list, closed mask)]: the first -- shortest -- name list of every distinct closed mask, in the order the subsets
    of NAMES come (by size, then by NAMES' order), the empty selection first"""
    seen, out = set(), []
    for n in range(len(NAMES) + 1):
        for names in itertools.combinations(NAMES, n):
            m = closed_mask(O, names)
            if m not in seen:
                seen.add(m)
                out.append((names, m))
    return out


def selection_id(names):
    return "+".join(names) or "none"


def make_batch():
    from frenetix_occlusion import synthetic as S
    traj, agents = S.make_batch(M, A, config_id=1)
    assert traj["x"].shape == (M, T)
    agents["len"] = np.array(AGENT_LEN, dtype=np.int32)
    return traj, agents, S.VEHICLE_BMW320I, DT


def thresholds(O, ref_all):
    """one threshold per key, each the median of the oracle's own per-trajectory value in the all-seven run (dce: 0.05)"""
    c = ref_all["cost"]
    return {"harm": float(np.median(c[:, O.COST["max_obst_harm_with_cp_all"]])),
            "risk": float(np.median(c[:, O.COST["max_obst_risk_all"]])),
            "cp": float(np.median(c[:, O.COST["max_collision_probability_all"]])),
            "ttc": float(np.median(c[:, O.COST["wttc"]])),
            "dce": 0.05,
            "be": float(np.median(ref_all["pair_f"][..., O.PF["be_btn"]].max(axis=1)))}


_REF = {}


def oracle_case(O):
    """(traj, agents, vehicle, dt, thresholds, all-seven run without thresholds), made once per process"""
    if "case" not in _REF:
        traj, agents, veh, dt = make_batch()
        ref_all = O.sweep(traj, agents, veh, dt, metrics=NAMES)
        _REF["case"] = (traj, agents, veh, dt, thresholds(O, ref_all), ref_all)
    return _REF["case"]


def oracle_run(O, names, thr="all"):
    """the oracle on the batch for one selection; thr: 'all' (the six thresholds), None, or a dict.  Cached: treat as read-only"""
    traj, agents, veh, dt, thr_all, _ = oracle_case(O)
    t = thr_all if thr == "all" else thr
    key = (tuple(names), None if t is None else tuple(sorted(t.items())))
    if key not in _REF:
        _REF[key] = O.sweep(traj, agents, veh, dt, metrics=tuple(names), thr=t)
    return _REF[key]


def expected_safe(O, ref_all, mask, thr):
    """metric.py:50-98 on the all-seven run's own values: a threshold counts only where its metric is evaluated"""
    c, bit = ref_all["cost"], O.METRIC_BITS
    ok = np.ones(len(c), dtype=bool)
    g = lambda k: thr.get(k) if thr else None
    if mask & bit["hr"]:
        for key, col in (("harm", "max_obst_harm_with_cp_all"), ("risk", "max_obst_risk_all"), ("cp", "max_collision_probability_all")):
            if g(key) is not None:
                ok &= ~(c[:, O.COST[col]] > g(key))
    if mask & bit["ttc"] and g("ttc") is not None:
        ok &= ~(c[:, O.COST["wttc"]] < g("ttc"))
    if mask & bit["dce"] and g("dce") is not None:
        ok &= ~(ref_all["pair_f"][..., O.PF["dce"]] < g("dce")).any(axis=1)
    if mask & bit["be"] and g("be") is not None:
        ok &= ~(c[:, O.COST["max_btn"]] > g("be"))
    return ok.astype(np.uint8)


def restrict(O, ref_all, mask, thr):
    """the all-seven run restricted to the metrics of `mask`: everything a metric outside it owns becomes its neutral value"""
    on = lambda owner: bool(mask & O.METRIC_BITS[owner])
    pf, pi = ref_all["pair_f"].copy(), ref_all["pair_i"].copy()
    lists, cost = ref_all["lists"].copy(), ref_all["cost"].copy()
    for name, owner in PAIR_F_OWNER.items():
        if not on(owner):
            pf[..., O.PF[name]] = PAIR_F_NEUTRAL
    for name, owner in PAIR_I_OWNER.items():
        if not on(owner):
            pi[..., O.PI[name]] = PAIR_I_NEUTRAL
    for name, owner in LIST_OWNER.items():
        if not on(owner):
            lists[:, :, O.LST[name], :] = LIST_NEUTRAL
    for name, owner in COST_OWNER.items():
        if not on(owner):
            cost[:, O.COST[name]] = COST_NEUTRAL[name]
    safe = expected_safe(O, ref_all, mask, thr)
    cost[:, O.COST["safe"]] = safe
    return {"pair_f": pf, "pair_i": pi, "lists": lists, "cost": cost, "safe": safe}


def bit_equal(a, b):
    """same dtype, same shape, same values, NaNs at the same places"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---------------------------------------------------------------------------------------- the total comparison
def _same_specials(a, b, what):
    for kind, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        bad = np.argwhere(f(a) != f(b))
        assert len(bad) == 0, f"{what}: {kind} pattern differs at {len(bad)} places, e.g. {bad[:5].tolist()}"


def _close(a, b, atol, what, skip=None):
    _same_specials(a, b, what)
    fin = np.isfinite(a)
    if skip is not None:
        fin = fin & ~skip
    err = np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0))
    bad = np.argwhere(err > atol)
    assert len(bad) == 0, f"{what}: off by up to {err.max():.3g} at {len(bad)} places, e.g. {bad[:5].tolist()}"
    return float(err.max()) if err.size else 0.0


def _exact(a, b, what):
    bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)))
    assert len(bad) == 0, f"{what}: differs at {len(bad)} places, e.g. {bad[:5].tolist()}: got {b[tuple(bad[0])]!r}, want {a[tuple(bad[0])]!r}"


def compare_total(O, ref, got, atol=ATOL, what=""):
    """ref = the oracle's output of a `full` run, got = the device's, both in the oracle's layout: every pair float, every
    pair integer, every list row, every cost column and `safe`.  NaN, +inf and -inf sit at the same places everywhere; finite
    floats agree within atol; what both sides round or count agrees exactly; the arg-max indices and max_obst_harm_with_cp
    follow _compare's plateau rule.  Returns the largest deviation seen."""
    assert ref["lists"] is not None and got.get("lists") is not None, "compare_total wants the lists of a `full` run"
    for k in ("pair_f", "pair_i", "lists", "cost", "safe"):
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
    PF, PI, LST, C = O.PF, O.PI, O.LST, O.COST
    for name in ("max_obst_risk_index", "cp_argmax"):      # in range, before anything is indexed with them
        gi = got["pair_i"][..., PI[name]]
        assert ((gi >= 0) & (gi < max(ref["lists"].shape[-1], 1))).all(), f"{what} {name} out of range"
    worst = _compare(O, ref, got, atol)          # what every other sweep test asks, the plateau rule included
    plateau = _cp_plateau(O, ref, got, atol)
    # pair floats: all twelve columns (the spare one too)
    named = {v: k for k, v in PF.items()}
    for col in range(ref["pair_f"].shape[-1]):
        name = named.get(col, f"pair_f[{col}]")
        a, b = ref["pair_f"][..., col], got["pair_f"][..., col]
        if name in EXACT_PAIR_F:
            _exact(a, b, f"{what} {name}")
        else:
            worst = max(worst, _close(a, b, atol, f"{what} {name}", skip=plateau if name == "max_obst_harm_with_cp" else None))
    # pair integers: all four columns; the two arg-max indices under the plateau rule (_compare above)
    for name in EXACT_PAIR_I:
        _exact(ref["pair_i"][..., PI[name]], got["pair_i"][..., PI[name]], f"{what} {name}")
    for name in ("max_obst_risk_index", "cp_argmax"):
        off = ~(ref["pair_i"][..., PI["hr_valid"]] > 0)
        _exact(ref["pair_i"][..., PI[name]][off], got["pair_i"][..., PI[name]][off], f"{what} {name} without a harm model")
    # lists: every row
    for name, row in LST.items():
        worst = max(worst, _close(ref["lists"][:, :, row, :], got["lists"][:, :, row, :], atol, f"{what} list {name}"))
    # cost vector: the special values of the whole matrix, then column by column
    _same_specials(ref["cost"], got["cost"], f"{what} cost")
    cnamed = {v: k for k, v in C.items()}
    for col in range(ref["cost"].shape[-1]):
        name = cnamed.get(col, f"cost[{col}]")
        a, b = ref["cost"][:, col], got["cost"][:, col]
        if name in EXACT_COST or name not in C:                    # (the reserved columns hold zeros)
            _exact(a, b, f"{what} cost {name}")
        elif name == "argmax_risk":
            mx = ref["cost"][:, C["max_obst_risk_all"]]
            assert ((b >= -1) & (b < ref["pair_f"].shape[1]) & (b == np.round(b))).all(), f"{what} argmax_risk out of range"
            live = mx > 1e-9          # below that the maximum is zero or noise: the oracle says -1 or any agent holding it
            assert (b[live] >= 0).all() and (a[live] >= 0).all(), f"{what} argmax_risk unset beside a risk"
            _assert_argmax(ref["pair_f"][..., PF["max_obst_risk"]][live], mx[live], a[live].astype(np.int64),
                           b[live].astype(np.int64), atol, f"{what} argmax_risk")
            none = (mx == 0.0) & (got["cost"][:, C["max_obst_risk_all"]] == 0.0)
            _exact(a[none], b[none], f"{what} argmax_risk without any risk")
        else:
            skip = plateau.any(axis=1) if name == "max_obst_harm_with_cp_all" else None
            worst = max(worst, _close(a, b, atol, f"{what} cost {name}", skip=skip))
    _exact(ref["safe"], got["safe"], f"{what} safe")
    return worst
