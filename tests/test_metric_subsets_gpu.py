"""Every metric selection on every form of the sweep kernels (cases: tests/metric_subset_cases.py; their reference side is
pinned in tests/test_metric_subsets_cpu.py).

The queue kernel exists in two compiled copies: the default metric set as compile-time constants (ALLM = true) and the copy
that reads the selection from the mask at run time, which is what a caller gets for any other `activated_metrics` list; the
generic kernel only has the run-time form.  For each of the 33 closed selections, in each kernel form and output mode:

(a) `full` / float64 lists against the oracle run with the same selection and all six thresholds, output by output
    (compare_total), the empty selection included;
(b) the float32 list formats against the float64 lists and the oracle, everything else bit-equal across the formats;
(c) `pair` and `reduced` bit-equal to `full`;
(d) every output of a metric bit-identical in all selections that evaluate it and run the same machine code: one metric's
    flag must not reach another metric's arithmetic;
(e) 'be' alone and beside 'hr' (part of (a): be_decel, be_btn, max_btn and `safe` under the be threshold);
(f) the launch is the form asked for.

Needs a real MI355X: run with `pytest -m gpu`."""
import itertools
import json

import numpy as np
import pytest

import metric_subset_cases as K
from test_sweep_gate_gpu import KERNEL_FORMS, _set_env
from test_sweep_gpu import LIST32_ATOL

pytestmark = pytest.mark.gpu

MODES = (("full", "f64"), ("full", "f32x"), ("full", "f32"), ("pair", "f64"), ("reduced", "f64"))
AGENT_KEYS = ("pos", "yaw", "v", "cov", "shape", "raw_dims", "type", "len")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


def _to_host(torch, sw, out):
    torch.cuda.synchronize()
    res = {"cost": out.cost.cpu().numpy(), "safe": out.safe.cpu().numpy(), "launch": sw.ctx.last_launch()}
    if out.pair_f is not None:
        res["pair_f"] = out.pair_f.permute(2, 1, 0).cpu().numpy()    # -> [M,A,NPF] (oracle layout)
        res["pair_i"] = out.pair_i.permute(2, 1, 0).cpu().numpy()
    if out.lists is not None:
        res["lists"] = out.lists.permute(3, 1, 0, 2).cpu().numpy()   # -> [M,A,NL,T-1]
    return res


def _run_selection(torch, case, names, modes=MODES):
    """one MetricSweep (one context) for the selection, every output mode on it"""
    from frenetix_occlusion.sweep import MetricSweep
    traj, agents, veh, dt, thr, _ = case
    sw = MetricSweep(veh, dt, metrics=names, thresholds=thr)
    try:
        sw.set_agents(*[agents[k] for k in AGENT_KEYS])
        outs = {}
        for mode, lists in modes:
            out = sw.run(traj["x"], traj["y"], traj["theta"], traj["v"], traj["a"], mode=mode, lists=lists)
            outs[(mode, lists)] = _to_host(torch, sw, out)
        return outs
    finally:
        sw.ctx.close()


@pytest.fixture(scope="module", params=KERNEL_FORMS, ids=[f[0] for f in KERNEL_FORMS])
def form_runs(request, torch_cuda, oracle):
    """(form, selections, {names: {(mode, lists): outputs}}): all 33 selections x 5 output modes of one kernel form, run once for
    the tests below (the FO_SWEEP_* knobs are read per run)"""
    form, env = request.param
    case, sels = K.oracle_case(oracle), K.selections(oracle)
    mp = pytest.MonkeyPatch()
    try:
        _set_env(mp, env)
        runs = {names: _run_selection(torch_cuda, case, names) for names, _ in sels}
    finally:
        mp.undo()
    return form, sels, runs


# --------------------------------------------------------------------------------------------------------- (a), (e)
def test_every_selection_matches_the_oracle_output_by_output(oracle, form_runs):
    form, sels, runs = form_runs
    worst = 0.0
    for names, mask in sels:
        ref = K.oracle_run(oracle, names)
        worst = max(worst, K.compare_total(oracle, ref, runs[names][("full", "f64")], what=f"{form} {K.selection_id(names)}:"))
    print(f"{form}: largest deviation from the oracle over {len(sels)} selections {worst:.3g}")
    # the empty selection: ({}, True) for every candidate (metric.py:44), every output the neutral value
    got = runs[()][("full", "f64")]
    assert (got["safe"] == 1).all() and np.isnan(got["pair_f"]).all() and np.isnan(got["lists"]).all() and not got["pair_i"].any()
    for name, v in K.COST_NEUTRAL.items():
        assert (got["cost"][:, oracle.COST[name]] == v).all(), name


def test_brake_evaluation_alone_and_beside_the_harm_model(torch_cuda, oracle, form_runs):
    """('be',) and ('be', 'hr'): be_mask is written by the sweep kernel of every form from ttc (be.py:49-50), the brake kernel
    and the reduction take it from there"""
    O = oracle
    form, sels, runs = form_runs
    thr = K.oracle_case(O)[4]
    for names in (("be",), ("be", "hr")):
        assert names in runs
        ref, got = K.oracle_run(O, names), runs[names][("full", "f64")]
        ttc = ref["pair_f"][..., O.PF["ttc"]]
        active = np.isfinite(ttc) & (ttc > 0)
        assert active.sum() >= 50
        btn = got["pair_f"][..., O.PF["be_btn"]]
        assert np.array_equal(btn > 0, active) and not np.isnan(btn).any(), (form, names)
        assert np.array_equal(got["pair_f"][..., O.PF["be_decel"]] > 0, active), (form, names)
        assert np.abs(got["cost"][:, O.COST["max_btn"]] - btn.max(axis=1)).max() == 0.0
        only_be = K.oracle_run(O, names, {"be": thr["be"]})
        assert 0.1 <= only_be["safe"].mean() <= 0.9
        for mode in (("full", "f64"), ("reduced", "f64")):
            assert np.array_equal(runs[names][mode]["safe"], ref["safe"]), (form, names, mode)
    # the be threshold decides by itself: a run with that threshold alone
    mp = pytest.MonkeyPatch()
    try:
        _set_env(mp, dict(KERNEL_FORMS)[form])
        case = list(K.oracle_case(O))
        case[4] = {"be": thr["be"]}
        got = _run_selection(torch_cuda, case, ("be",), modes=(("reduced", "f64"),))[("reduced", "f64")]
    finally:
        mp.undo()
    assert np.array_equal(got["safe"], K.oracle_run(O, ("be",), {"be": thr["be"]})["safe"]), form


# --------------------------------------------------------------------------------------------------------------- (b)
def test_list_formats_agree_in_every_selection(oracle, form_runs):
    form, sels, runs = form_runs
    for names, mask in sels:
        ref = K.oracle_run(oracle, names)["lists"]
        g64, gx, g32 = (runs[names][("full", f)] for f in ("f64", "f32x", "f32"))
        what = (form, names)
        assert g64["lists"].dtype == np.float64 and gx["lists"].dtype == np.float32 and g32["lists"].dtype == np.float32
        assert np.array_equal(gx["lists"], g64["lists"].astype(np.float32), equal_nan=True), what
        for g in (gx, g32):
            # (also where nothing writes the lists -- the all-ones fill -- and where only the cp row is written)
            assert np.array_equal(np.isnan(g["lists"]), np.isnan(ref)), what
            assert not np.isinf(g["lists"]).any(), what
            for k in ("cost", "safe", "pair_f", "pair_i"):
                assert K.bit_equal(g[k], g64[k]), (what, k)
        fin = np.isfinite(ref)
        if fin.any():
            err = float(np.abs(g32["lists"][fin].astype(np.float64) - ref[fin]).max())
            assert err < LIST32_ATOL, (what, err)


# --------------------------------------------------------------------------------------------------------------- (c)
def test_output_modes_agree_in_every_selection(form_runs):
    form, sels, runs = form_runs
    for names, mask in sels:
        full, pair, red = (runs[names][m] for m in (("full", "f64"), ("pair", "f64"), ("reduced", "f64")))
        assert "lists" not in pair and "pair_f" not in red
        for other in (pair, red):
            assert K.bit_equal(other["cost"], full["cost"]) and K.bit_equal(other["safe"], full["safe"]), (form, names)
        assert K.bit_equal(pair["pair_f"], full["pair_f"]) and K.bit_equal(pair["pair_i"], full["pair_i"]), (form, names)


# --------------------------------------------------------------------------------------------------------------- (d)
def _fields(O, out):
    """(name, owner metric, array) of every output a single metric owns"""
    for name, owner in K.PAIR_F_OWNER.items():
        yield "pair_f." + name, owner, out["pair_f"][..., O.PF[name]]
    for name, owner in K.PAIR_I_OWNER.items():
        yield "pair_i." + name, owner, out["pair_i"][..., O.PI[name]]
    for name, owner in K.LIST_OWNER.items():
        yield "lists." + name, owner, out["lists"][:, :, O.LST[name], :]
    for name, owner in K.COST_OWNER.items():
        yield "cost." + name, owner, out["cost"][:, O.COST[name]]


def test_selections_cannot_see_each_other(oracle, form_runs):
    """Within one kernel form every selection but the ones that hold the default five runs the same machine code with other
    flags (the generic kernel: all of them), so an output of a metric is bit-identical in every selection that evaluates it;
    compared against the first selection of the loop that does.  The selections with the default five run the copy compiled
    with the metric set as constants: bit-identical among themselves; against the run-time copy the largest difference per
    output is reported, not asserted ((a) holds both to the oracle)."""
    O = oracle
    form, sels, runs = form_runs
    all5 = O.metric_mask(("dce", "cp", "ttc", "ttce", "hr"))
    first, compared = {}, 0
    for names, mask in sels:
        copy = "constants" if (form != "generic" and mask & all5 == all5) else "run time"
        for fmt in ("f64", "f32"):
            for field, owner, arr in _fields(O, runs[names][("full", fmt)]):
                if not mask & O.METRIC_BITS[owner]:
                    continue
                base = first.setdefault((copy, fmt, field), (names, arr))
                if base[0] != names:
                    bad = np.argwhere(~((arr == base[1]) | ((arr != arr) & (base[1] != base[1]))))
                    assert len(bad) == 0, (f"{form}, {fmt} lists: {field} under {K.selection_id(names)} differs from the same output "
                                           f"under {K.selection_id(base[0])} at {len(bad)} places, e.g. {bad[:5].tolist()}")
                    compared += 1
    assert compared > 300, compared
    # the examples of the issue are among the pairs compared
    assert first[("run time", "f64", "lists.cp")][0] == ("cp",) and first[("run time", "f64", "pair_f.dce")][0] == ("dce",)
    assert first[("run time", "f64", "lists.obst_harm")][0] == ("hr",)
    if form != "generic":
        diff = {}
        for (copy, fmt, field), (names, arr) in first.items():
            if copy == "constants" and fmt == "f64" and ("run time", fmt, field) in first:
                other = first[("run time", fmt, field)][1]
                assert np.array_equal(np.isnan(arr), np.isnan(other)), field
                fin = np.isfinite(arr) & np.isfinite(other)
                diff[field] = float(np.abs(arr[fin].astype(np.float64) - other[fin]).max()) if fin.any() else 0.0
        print("ALLM-vs-run-time " + json.dumps({"form": form, "max_abs_diff": diff}))


# --------------------------------------------------------------------------------------------------------------- (f)
def test_every_selection_launches_the_form_asked_for(torch_cuda, oracle, form_runs):
    """last_launch after every run: no selection or output mode falls back to another plan.  Both kernels run 256 threads; the
    horizon-split form is one workgroup per (tile, agent), the others one per (tile, four agents) at one agent per wave (tiles
    in rounds of eight, fo_sweep_plan.hpp).  The generic kernel and the unsplit queue kernel share that plan; they are told
    apart by their arithmetic: the generic kernel takes libm's route, the queue kernel its tables, and the harm lists of the
    two differ in the last bits (both within 1e-9 of the oracle)."""
    form, sels, runs = form_runs
    tile_slots = (K.M + 63) // 64
    tile_slots = (tile_slots + 7) // 8 * 8
    split = form in ("auto", "queue, split")            # 3 x 9 (tile, agent) pairs, T - 1 = 30: auto splits
    want = {"grid": tile_slots * (K.A if split else (K.A + 3) // 4), "block": 256, "agents_per_wave": 1}
    for names, mask in sels:
        for mode, out in runs[names].items():
            assert out["launch"] == want, (form, names, mode, out["launch"], want)
    if form == "generic":
        mp = pytest.MonkeyPatch()
        try:
            _set_env(mp, {"FO_SWEEP_SPLIT": "0"})
            queue = _run_selection(torch_cuda, K.oracle_case(oracle), ("hr",), modes=(("full", "f64"),))[("full", "f64")]
        finally:
            mp.undo()
        assert queue["launch"] == want
        assert not np.array_equal(queue["lists"], runs[("hr",)][("full", "f64")]["lists"], equal_nan=True), \
            "FO_SWEEP_GENERIC=1 gave the queue kernel's bits: the generic kernel did not run"


# ------------------------------------------------------------------------------- the closure inside the library
def test_the_librarys_closure_on_all_128_subsets(torch_cuda, oracle, monkeypatch):
    """fo_sweep_configure closes the mask (required_metrics, fo_sweep_be_reduce.hpp); nothing exports the closed mask, so it
    is read off the outputs: which metric's outputs are written, and every raw subset bit-equal to the first subset with the
    same closure.  ('wttc' leaves no output of its own: it shows in the ttc it pulls in.)"""
    from frenetix_occlusion.sweep import MetricSweep
    O = oracle
    _set_env(monkeypatch, {})
    case = K.oracle_case(O)
    traj, agents, veh, dt, thr, _ = case
    sw = MetricSweep(veh, dt, metrics=(), thresholds=thr)
    sw.set_agents(*[agents[k] for k in AGENT_KEYS])
    seen, n = {}, 0
    try:
        for names in (c for r in range(len(K.NAMES) + 1) for c in itertools.combinations(K.NAMES, r)):
            sw.configure(veh, thr, metrics=names)
            got = _to_host(torch_cuda, sw, sw.run(traj["x"], traj["y"], traj["theta"], traj["v"], traj["a"], mode="full"))
            written = {"dce": not np.isnan(got["pair_f"][..., O.PF["dce"]]).all(),
                       "ttc": not np.isnan(got["pair_f"][..., O.PF["ttc"]]).all(),
                       "ttce": not np.isnan(got["pair_f"][..., O.PF["ttce"]]).all(),
                       "cp": not np.isnan(got["lists"][:, :, O.LST["cp"], :]).all(),
                       "hr": bool(got["pair_i"][..., O.PI["hr_valid"]].any()),
                       "be": not np.isnan(got["pair_f"][..., O.PF["be_btn"]]).all()}
            closed = K.closed_mask(O, names)
            assert {k for k, v in written.items() if v} == set(K.mask_names(O, closed)) - {"wttc"}, names
            base = seen.setdefault(closed, got)
            for k in ("cost", "safe", "pair_f", "pair_i", "lists"):
                assert K.bit_equal(got[k], base[k]), (names, k)
            n += 1
    finally:
        sw.ctx.close()
    assert n == 128 and len(seen) == K.N_SELECTIONS
