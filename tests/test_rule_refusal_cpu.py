"""The host side of refused spawn-rule steps (include/fo_hip.h, "A refused rule list"), without a GPU: the sample-count formula
and the set-up warning against the one place the table size is written down, ``select_trajectory`` on a matrix without a
verdict, the host views of a batch that carries the refusal mark, and the reduce kernel's verdict (csrc/fo_verdict.hpp, built
with the host C++ compiler like csrc/fo_rule_plan.hpp in tests/test_rule_plan_cpu.py) over refused x covariance x agents."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include <cstdio>
#include "fo_rule_plan.hpp"
#include "fo_verdict.hpp"
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'C') {          // C -> RL_MAXSAMP FO_LEN_REFUSED
      printf("%d %d\n", RL_MAXSAMP, FO_LEN_REFUSED);
    } else if (what == 'V') {   // V A mask cov refused, then the six thresholds and the fourteen folded values -> ok + the fourteen
      int A, cov, refused;
      unsigned mask;
      fo_thresholds_t t;
      fo_folded_t f;
      if (scanf("%d %u %d %d", &A, &mask, &cov, &refused) != 4) return 1;
      if (scanf("%lf %lf %lf %lf %lf %lf", &t.harm, &t.risk, &t.be, &t.cp, &t.ttc, &t.dce) != 6) return 1;
      double *v = &f.min_ttc;
      for (int i = 0; i < 14; ++i) if (scanf("%lf", v + i) != 1) return 1;
      const bool ok = fo_verdict(A, mask, t, cov != 0, refused != 0, f);
      printf("%d", (int)ok);
      for (int i = 0; i < 14; ++i) printf(" %.17g", v[i]);
      printf("\n");
    } else {
      return 1;
    }
  }
  return 0;
}
"""
FOLDED = ("min_ttc", "min_dce", "max_er", "max_or", "max_eh", "max_oh", "max_cp", "max_hwc", "min_ttce", "arg_dce", "arg_ttc", "arg_or",
          "max_btn", "flag")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("verdict")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(d / "driver.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [ln.split() for ln in out[:-1]]
    return run


# ------------------------------------------------------------------------------------------------ one number, written down once
@needs_cxx
def test_the_sample_table_bound_is_the_headers(ask):
    import rule_refusal_cases as RC
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import spawn_locator as SL
    maxsamp, len_refused = (int(v) for v in ask(["C"])[0])
    assert N.RULE_MAX_SAMPLES == SL.RULE_MAX_SAMPLES == RC.MAXSAMP == maxsamp == 1024
    assert N.LEN_REFUSED == len_refused == -2**31      # INT32_MIN: any other negative length stays an unused slot


def test_host_formula_of_the_sample_count():
    """ns = ceil((total + step / 2) / step), step = cell / 8 (fo_rule_pedestrian.hpp:38,154): the restatement the scenes are
    placed by, SpawnLocator's own, and the lengths on either side of the table's edge"""
    import rule_refusal_cases as RC
    from frenetix_occlusion import spawn_locator as SL
    for cs in (0.5, 0.3125, 0.25, 0.31085):
        step = cs / 8.0
        for total in (0.01, 1.0, 17.3, 31.96875, 32.00625, 39.75, 63.9, 64.1):
            want = int(math.ceil((total + 0.5 * step) / step))
            assert RC.samples(total, cs) == SL.rule_line_samples(total, cs) == want
        # the longest line that fits: total <= (MAXSAMP - 1/2) step; the scenes stand half a sample inside / 0.7 outside
        assert RC.samples(RC.total_for(1023.5, cs), cs) == 1024 and RC.samples(RC.total_for(1024.7, cs), cs) == 1025
        edge = (SL.RULE_MAX_SAMPLES - 0.5) * step
        assert RC.samples(edge * (1 - 1e-12), cs) == 1024 and RC.samples(edge * (1 + 1e-9), cs) == 1025
    # the walls of the static scenes at 0.25 m cells: 30.369 m and 30.406 m of obstacle
    assert RC.total_for(1023.5, 0.25) - 1.6 == pytest.approx(30.36875) and RC.total_for(1024.7, 0.25) - 1.6 == pytest.approx(30.40625)
    ob = RC.wall(17.0, RC.total_for(1023.5, 0.25))
    assert RC.cross_line_total(ob, None) == pytest.approx(RC.total_for(1023.5, 0.25), abs=1e-12)
    # the turn scene: a window of about 40 m, the cell sizes that put it on 1 024 and on 1 025 samples
    total = RC.turn_window_length()
    assert RC.samples(total, RC.turn_cell_size(1023.5)) == 1024 and RC.samples(total, RC.turn_cell_size(1024.7)) == 1025
    assert RC.samples(total, 0.25) > 1024 and RC.samples(total, 0.5) < 1024


def test_warning_thresholds_follow_the_exported_constant(monkeypatch):
    from frenetix_occlusion import spawn_locator as SL
    n = SL.RULE_MAX_SAMPLES
    assert SL.turn_line_min_cell() == 8.0 * 40.0 / (n - 2.0)
    assert not SL.turn_line_outgrows_table(SL.turn_line_min_cell() * (1 + 1e-12))
    assert SL.turn_line_outgrows_table(SL.turn_line_min_cell() * (1 - 1e-12))
    assert SL.cross_line_limit(0.5) == n * 0.5 / 8.0 == 64.0 and SL.cross_line_limit(0.25) == 32.0
    # a line at the limit is the longest whose samples fit, to within the half step the kernel adds
    for cs in (0.5, 0.25):
        assert SL.rule_line_samples(SL.cross_line_limit(cs) - cs / 8.0, cs) <= n < SL.rule_line_samples(SL.cross_line_limit(cs), cs)
    monkeypatch.setattr(SL, "RULE_MAX_SAMPLES", 2048)          # the numbers move with the constant, nothing is typed in twice
    assert SL.turn_line_min_cell() == 320.0 / 2046.0 and SL.cross_line_limit(0.5) == 128.0
    assert "2048 samples" in SL.rule_table_warning(0.1, True, True) and "25.6 m" in SL.rule_table_warning(0.1, True, True)


def test_warning_names_both_rules_and_the_number_of_the_check():
    from frenetix_occlusion import spawn_locator as SL
    text = SL.rule_table_warning(0.25, True, True)
    assert "turn rule" in text and "static-obstacle rule" in text and "cross line" in text
    assert f"{SL.turn_line_min_cell():.4f} m" in text and "0.3131" in text and "0.32 " not in text
    assert f"{SL.cross_line_limit(0.25):g} m" in text and "32 m" in text
    assert f"{SL.RULE_MAX_SAMPLES} samples" in text
    # raised exactly where the check says so, naming only the rules that are on
    assert SL.rule_table_warning(0.5, True, True) is None and SL.rule_table_warning(0.25, False, False) is None
    lo, hi = SL.turn_line_min_cell() * (1 - 1e-9), SL.turn_line_min_cell() * (1 + 1e-9)
    assert SL.rule_table_warning(lo, True, True) is not None and SL.rule_table_warning(hi, True, True) is None
    only_static = SL.rule_table_warning(0.25, False, True)
    assert "static-obstacle rule" in only_static and "turn rule" not in only_static
    only_turn = SL.rule_table_warning(0.25, True, False)
    assert "turn rule" in only_turn and "static-obstacle rule" not in only_turn


# ------------------------------------------------------------------------------------------------ select_trajectory
def test_select_trajectory_refuses_a_matrix_without_a_verdict():
    import torch
    from frenetix_occlusion import _native as N
    from frenetix_occlusion.distributed import select_trajectory
    M = 130
    refused = torch.full((M, 16), float("nan"), dtype=torch.float64)
    refused[:, N.COST["safe"]] = 0.0
    refused[:, 14:] = 0.0
    with pytest.raises(RuntimeError, match="no verdict"):
        select_trajectory(refused)
    # one safe row: today's answer -- the safe one, whatever the others hold
    one = refused.clone()
    one[77] = 0.5
    one[77, N.COST["safe"]] = 1.0
    assert select_trajectory(one) == 77
    # nobody safe but the fallback column holds numbers: the smallest of them, as before
    c = torch.zeros((4, 16), dtype=torch.float64)
    c[:, N.COST["max_obst_harm_with_cp_all"]] = torch.tensor([0.5, 0.4, 0.3, 0.9])
    assert select_trajectory(c) == 2
    c[2, N.COST["max_obst_harm_with_cp_all"]] = float("nan")
    assert select_trajectory(c) == int(torch.argmin(c[:, N.COST["max_obst_harm_with_cp_all"]]).item())   # (unchanged: not ALL NaN)
    assert select_trajectory(c[:0]) == -1


# ------------------------------------------------------------------------------------------------ host views
def _batch(len_words, rule_n, n_rule_points=2, R=1, T=2):
    """a PhantomBatch on the CPU whose body and head hold what the device would have left"""
    import torch
    from frenetix_occlusion.spawn_locator import PhantomBatch
    S_ = len(len_words)
    A = S_ // R
    f = lambda *shape: np.zeros(shape)
    body = b"".join(a.tobytes() for a in (f(S_, T, 2), f(S_, T), f(S_, T), f(S_, T, 2, 2), f(S_, 2), f(S_, 2))) + \
        np.asarray(len_words, dtype=np.int32).tobytes()
    head = f(A, 2).tobytes() + f(A).tobytes() + f(n_rule_points, 8).tobytes() + np.asarray([0, rule_n], dtype=np.int32).tobytes() + \
        np.full(S_, 4, dtype=np.int32).tobytes()
    t = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    z = torch.zeros
    return PhantomBatch(n=z(1, dtype=torch.int32), cell=z(0, dtype=torch.int32), pos0=z(A, 2), yaw0=z(A), pos=z(S_, T, 2), yaw=z(S_, T),
                        v=z(S_, T), cov=z(S_, T, 2, 2), shape=z(S_, 2), raw_dims=z(S_, 2), type=z(S_, dtype=torch.int32),
                        len=torch.as_tensor(len_words, dtype=torch.int32), R=R, head=t(head), n_cell_agents=0,
                        n_rule_points=n_rule_points, body=t(body))


def test_no_negative_length_reaches_a_host_view():
    from frenetix_occlusion import _native as N
    b = _batch([N.LEN_REFUSED, 0, -3], rule_n=-1, n_rule_points=3)
    assert b.host_body()["len"].tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match="table space"):
        b.host_head()
    with pytest.raises(RuntimeError, match="table space"):
        b.live_agents()
    ok = _batch([2, 0], rule_n=1)
    assert ok.host_body()["len"].tolist() == [2, 0] and ok.live_agents() == [0] and ok.host_head()["rule_n"] == 1


# ------------------------------------------------------------------------------------------------ the reduce kernel's verdict
M_DCE, M_CP, M_TTC, M_TTCE, M_WTTC, M_BE, M_HR = 1, 2, 4, 8, 16, 32, 64
THR = dict(harm=0.1, risk=1.0, be=0.8, cp=0.5, ttc=1.0, dce=2.0)
CALM = dict(min_ttc=math.inf, min_dce=7.5, max_er=0.01, max_or=0.02, max_eh=0.03, max_oh=0.04, max_cp=0.05, max_hwc=0.06, min_ttce=math.inf,
            arg_dce=3.0, arg_ttc=-1.0, arg_or=2.0, max_btn=0.1, flag=0.0)
HARSH = dict(CALM, min_ttc=0.4, max_hwc=0.7, max_or=1.5, max_cp=0.9, flag=1.0, max_btn=0.95, arg_ttc=5.0)


def expected_verdict(A, mask, cov, refused, f):
    """restatement of include/fo_hip.h: thresholds only with agents; the covariance poison only with agents and a metric that
    reads a collision probability; a refused rule list always, and over everything"""
    f = dict(f)
    ok = True
    if A > 0:
        if mask & M_HR and (f["max_hwc"] > THR["harm"] or f["max_or"] > THR["risk"] or f["max_cp"] > THR["cp"]):
            ok = False
        if mask & M_TTC and f["min_ttc"] < THR["ttc"]:
            ok = False
        if mask & M_DCE and f["flag"] > 0:
            ok = False
        if mask & M_BE and f["max_btn"] > THR["be"]:
            ok = False
        if cov and mask & (M_CP | M_HR):
            ok = False
            for k in ("max_cp", "max_er", "max_or", "max_hwc"):
                f[k] = math.nan
    if refused:
        ok = False
        for k in FOLDED[:-1]:
            f[k] = math.nan
    return ok, f


@needs_cxx
def test_verdict_over_refused_x_covariance_x_agents(ask):
    masks = (M_DCE, M_DCE | M_TTC, M_DCE | M_TTC | M_BE, M_DCE | M_CP, M_DCE | M_CP | M_TTC | M_HR, 127)
    cases = list(itertools.product((0, 1, 7), masks, (0, 1), (0, 1), (CALM, HARSH)))
    fmt = lambda v: "nan" if v != v else "inf" if v == math.inf else "-inf" if v == -math.inf else repr(float(v))
    lines = ["V %d %d %d %d " % c[:4] + " ".join(fmt(THR[k]) for k in ("harm", "risk", "be", "cp", "ttc", "dce")) + " " +
             " ".join(fmt(c[4][k]) for k in FOLDED) for c in cases]
    got = ask(lines)
    seen = set()
    for (A, mask, cov, refused, f), g in zip(cases, got):
        ok, want = expected_verdict(A, mask, cov, refused, f)
        vals = [float(v) for v in g[1:]]
        assert int(g[0]) == int(ok), (A, mask, cov, refused)
        for k, v in zip(FOLDED, vals):
            assert (v != v) == (want[k] != want[k]) and (v != v or v == want[k]), (A, mask, cov, refused, k, v, want[k])
        seen.add((A > 0, bool(cov), bool(refused), ok))
    # a refused set is never safe and keeps no number -- with no agent slot at all and under masks without CP / HR as well
    for (A, mask, cov, refused, f), g in zip(cases, got):
        if refused:
            assert g[0] == "0" and all(v == "nan" for v in g[1:14]), (A, mask, cov)
        elif A == 0:
            assert g[0] == "1" and "nan" not in g[1:], (mask, cov)              # no agents -> ({}, True), nothing poisoned
        elif cov and not mask & (M_CP | M_HR):
            assert "nan" not in g[1:], mask                                      # the covariance poison stays gated
    assert {(a, c, r) for a, c, r, _ in seen} == set(itertools.product((False, True), repeat=3))
    assert (True, False, False, True) in seen and (True, False, False, False) in seen
