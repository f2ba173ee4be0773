"""The queue kernel chooses the copy of its per-agent body -- LR4S, DVMAX or GENERIC, by the agent's harm model -- once per
agent (fo_sweep_queue.hpp, agent_body); the horizon-split form carries the model as a run-time value through one copy.  The
agent set of tests/sweep_agent_kind_cases.py (70 x 9, T = 31 and 10; what it holds and why: its header) in every output mode
and list format, at one and at four agents per wave and in the horizon-split form, under both coefficient sets:

(a) against the oracle through oracle/fo_compare.py at the tolerances bench.py's parity leg holds: floats 1e-9, float64 lists
    1e-9, float32 storage of float64 results 1e-9 before the rounding, float32 arithmetic 1e-6, no integer and no pattern
    mismatch;
(b) against each other, bit for bit: `pair` and `reduced` equal to `full`, the float32 formats equal to the float64 run in
    every other output, `f32x` lists equal to the float64 lists rounded, one agent per wave equal to four, split equal to
    unsplit (but for the lists of float32 arithmetic);
(c) the launch is the form asked for, and every body holds in-gate pairs and pairs with DCE = 0 (the oracle's own outputs).

Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

import sweep_agent_kind_cases as K
from test_sweep_gate_gpu import _set_env

pytestmark = pytest.mark.gpu

MODES = (("full", "f64"), ("full", "f32x"), ("full", "f32"), ("pair", "f64"), ("reduced", "f64"))
FORMS = (("one agent per wave", {"FO_SWEEP_SPLIT": "0", "FO_SWEEP_APW": "1"}),
         ("four agents per wave", {"FO_SWEEP_SPLIT": "0", "FO_SWEEP_APW": "4"}),
         ("horizon split", {"FO_SWEEP_SPLIT": "1"}))
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


@pytest.fixture(scope="module", params=[(T, i) for T in K.HORIZONS for i in (0, 1)],
                ids=[f"T{T}-{('usual', 'flipped')[i]}" for T in K.HORIZONS for i in (0, 1)])
def runs(request, torch_cuda, oracle):
    """(T, coefficient set's name, {form: {(mode, lists): outputs}}): one context per kernel form, every output mode on it (the
    FO_SWEEP_* knobs are read per run)"""
    from frenetix_occlusion.sweep import MetricSweep
    T, i = request.param
    hc_name, hc = K.harm_coeffs(oracle)[i]
    traj, agents, veh, dt = K.make_case(T)
    thr = K.thresholds(oracle, T)
    mp = pytest.MonkeyPatch()
    got = {}
    try:
        for form, env in FORMS:
            _set_env(mp, env)
            sw = MetricSweep(veh, dt, thresholds=thr, harm_coeff=hc)
            try:
                sw.set_agents(*[agents[k] for k in AGENT_KEYS])
                got[form] = {(mode, lists): _to_host(torch_cuda, sw, sw.run(traj["x"], traj["y"], traj["theta"], traj["v"], traj["a"],
                                                                           mode=mode, lists=lists))
                             for mode, lists in MODES}
            finally:
                sw.ctx.close()
    finally:
        mp.undo()
    return T, hc_name, got


# ------------------------------------------------------------------------------------------------------------------- (a)
def test_every_form_and_mode_matches_the_oracle(oracle, runs):
    from oracle import fo_compare as CMP
    T, hc_name, got = runs
    K.assert_every_body_is_exercised(oracle, T, hc_name)
    ref = K.oracle_run(oracle, T, hc_name)
    for form, outs in got.items():
        for (mode, lists), out in outs.items():
            what = (T, hc_name, form, mode, lists)
            if mode == "reduced":      # no pair outputs: the cost vector and the verdicts (the rest of it under (b))
                for name in CMP.COST_FLOATS:
                    a, b = ref["cost"][:, oracle.COST[name]], out["cost"][:, oracle.COST[name]]
                    assert np.array_equal(np.isinf(a), np.isinf(b)) and not np.isnan(b).any(), (what, name)
                    fin = np.isfinite(a)
                    assert not fin.any() or np.abs(a[fin] - b[fin]).max() <= 1e-9, (what, name)
                assert np.array_equal(out["safe"], ref["safe"]), what
                continue
            res = CMP.compare(ref, out)
            print(what, res)
            assert res["pairs"] == K.M * K.A
            assert res["int_mismatches"] == 0 and res["pattern_mismatches"] == 0, (what, res)
            assert res["float_max_abs_err"] <= 1e-9, (what, res)
            if mode == "full":
                assert res["list_max_abs_err"] <= (1e-9 if lists == "f64" else 1e-6), (what, res)
                if lists == "f32x":
                    assert res["list_err_beyond_f32_rounding"] <= 1e-9, (what, res)


# ------------------------------------------------------------------------------------------------------------------- (b)
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_modes_formats_and_forms_agree_bit_for_bit(runs):
    T, hc_name, got = runs
    for form, outs in got.items():
        full, fx, f32, pair, red = (outs[m] for m in MODES)
        what = (T, hc_name, form)
        assert "lists" not in pair and "pair_f" not in red
        for other in (fx, f32, pair, red):
            assert _same(other["cost"], full["cost"]) and _same(other["safe"], full["safe"]), what
        for other in (fx, f32, pair):
            assert _same(other["pair_f"], full["pair_f"]) and _same(other["pair_i"], full["pair_i"]), what
        assert full["lists"].dtype == np.float64 and fx["lists"].dtype == np.float32 and f32["lists"].dtype == np.float32
        assert _same(fx["lists"], full["lists"].astype(np.float32)), what
        assert np.array_equal(np.isnan(f32["lists"]), np.isnan(full["lists"])), what
    base = got[FORMS[0][0]]
    for form, _ in FORMS[1:]:
        for m in MODES:
            for k, v in base[m].items():
                # (float32 ARITHMETIC of the list entries: a row that seeds a wave's maxima is evaluated in float64 and
                # rounded, and the split form has four such rows per agent -- those lists are held to the oracle under (a),
                # not to each other)
                if k != "launch" and (m, k) != (("full", "f32"), "lists"):
                    assert _same(got[form][m][k], v), (T, hc_name, form, m, k)


# ------------------------------------------------------------------------------------------------------------------- (c)
def test_the_launch_is_the_form_asked_for(runs):
    """256 threads; tiles in rounds of eight; one workgroup per (tile, agent) in the horizon-split form, else per (tile, four
    waves x agents per wave) (fo_sweep_plan.hpp)"""
    T, hc_name, got = runs
    tile_slots = ((K.M + 63) // 64 + 7) // 8 * 8
    want = {"one agent per wave": {"grid": tile_slots * ((K.A + 3) // 4), "block": 256, "agents_per_wave": 1},
            "four agents per wave": {"grid": tile_slots * ((K.A + 15) // 16), "block": 256, "agents_per_wave": 4},
            "horizon split": {"grid": tile_slots * K.A, "block": 256, "agents_per_wave": 1}}
    for form, outs in got.items():
        for m, out in outs.items():
            assert out["launch"] == want[form], (T, hc_name, form, m, out["launch"])
