"""The host side of the hidden-traffic harm ladder (DESIGN.md §5.10 "Harm ladder"), without a GPU: the value rules
(csrc/fo_hidden_harm_ladder.hpp) and the launch plan (csrc/fo_scene_plan.hpp brake_harm_ladder_lds_bytes) built with the host C++
compiler, as tests/test_hidden_brake_ladder_verdict_cpu.py builds its headers, against the plain statement
tests/ref_hidden_brake_harm_ladder.py; the conditions the device tests rest on, by the checker alone on every scene they use; the
refusals of the Python layers that need no GPU; the library's symbols."""
import itertools
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_ladder_users_scenes as S
import hidden_harm_ladder_cases as HC
import ref_hidden_brake_harm_ladder as RH
from test_hidden_brake_ladder_verdict_cpu import expected_plan, most_classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

# the driver walks ONE trajectory as the kernel's lanes do: a lane per (b, l) prices nothing (the harms come in) but forms its over
# mask and its state with the header's rules; a group of L lanes forms its answers as hblu_required does; the states of equal level
# are merged over the brake starts -- in DESCENDING b, the order no lane of the kernel visits them in: the merge must not care
DRIVER = r"""
#include <cstdio>
#include <cmath>
#include "fo_scene_plan.hpp"
#include "fo_hidden_ladder_verdict.hpp"
#include "fo_hidden_harm_ladder.hpp"
static const int BS[6] = {1, 2, 3, 5, 8, 31};
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'C') {          // C -> NOT_FINITE NO_CLASS exchange bound
      printf("%d %d %d %zu\n", FO_HIDDEN_VERDICT_NOT_FINITE, FO_HIDDEN_HARM_LADDER_NO_CLASS, BRAKE_HARM_LADDER_EXCHANGE_BYTES, brake_harm_ladder_lds_bound());
    } else if (what == 'H') {   // H C L B finite limit, levels[L], then per (c, b, l): hit harm -> need at blocking user decel need_of[3] (harm_at user_at)[L]
      int C, L, B, finite;
      double limit, levels[3], ho[3][2][3];
      int hit[3][2][3];
      if (scanf("%d %d %d %d %lf", &C, &L, &B, &finite, &limit) != 5 || C > 3 || L > 3 || B > 2) return 1;
      for (int l = 0; l < L; ++l) if (scanf("%lf", levels + l) != 1) return 1;
      for (int c = 0; c < C; ++c) for (int b = 0; b < B; ++b) for (int l = 0; l < L; ++l)
        if (scanf("%d %lf", &hit[c][b][l], &ho[c][b][l]) != 2) return 1;
      int32_t key = FO_HIDDEN_LADDER_NO_KEY, need_of[3] = {-1, -1, -1};
      fo_hidden_harm_ladder_best_t lane[2][3];
      for (int b = 0; b < B; ++b) {
        bool over[3][3];
        for (int l = 0; l < L; ++l) {
          lane[b][l] = fo_hidden_harm_ladder_none();
          for (int c = 0; c < C; ++c) {
            over[c][l] = fo_hidden_harm_ladder_over(hit[c][b][l] != 0, ho[c][b][l], limit);
            if (hit[c][b][l]) fo_hidden_harm_ladder_take(lane[b][l], ho[c][b][l], c);
          }
        }
        int ra = -1;
        for (int l = L - 1; l >= 0; --l) { bool any = false; for (int c = 0; c < C; ++c) any |= over[c][l]; if (!any) ra = l; }
        const int lvl = ra < 0 ? L - 1 : ra - 1;
        int blk = 0;
        for (int c = 0; c < C; ++c) {
          if (lvl >= 0 && over[c][lvl]) blk |= 1 << c;
          int req = -1;
          for (int l = L - 1; l >= 0; --l) if (!over[c][l]) req = l;
          need_of[c] = fo_hidden_ladder_max(need_of[c], fo_hidden_ladder_rank(req, L));
        }
        key = fo_hidden_ladder_max(key, fo_hidden_ladder_key(fo_hidden_ladder_rank(ra, L), b, blk));
      }
      fo_hidden_ladder_verdict_t r = fo_hidden_ladder_verdict_of(key, L, finite != 0);
      const int nl = r.need >= 0 && r.need < L ? r.need : 0;
      r.decel = fo_hidden_ladder_decel(r.need, L, levels[nl]);
      printf("%d %d %d %d %.17g %d %d %d", r.need, r.at, r.blocking, r.user, r.decel, need_of[0], need_of[1], need_of[2]);
      for (int l = 0; l < L; ++l) {
        fo_hidden_harm_ladder_best_t s = fo_hidden_harm_ladder_none();
        for (int b = B - 1; b >= 0; --b) fo_hidden_harm_ladder_take(s, lane[b][l].harm, lane[b][l].cls);
        double h;
        int32_t u;
        fo_hidden_harm_ladder_curve(s, finite != 0, &h, &u);
        printf(" %.17g %d", h, u);
      }
      printf("\n");
    } else if (what == 'P') {   // P T K -> for L = 1 .. 64, B in {1, 2, 3, 5, 8, 31, T} (those <= T; else zeros), at the most classes C <= 8 that T and
                                // L admit: the ladder verdict's bytes and the harm ladder's
      int T, K;
      if (scanf("%d %d", &T, &K) != 2) return 1;
      for (int L = 1; L <= 64; ++L) {
        int C = 8;
        while (C > 1 && (C * T > BRAKE_USERS_MAX_TABLE || 4 * C * T + 8 * L > BRAKE_LADDER_USERS_MAX_ARG_BYTES)) --C;
        for (int i = 0; i < 7; ++i) {
          const int B = i < 6 ? BS[i] : T;
          if (B > T) { printf("0 0 "); continue; }
          printf("%zu %zu ", brake_ladder_verdict_lds_bytes(T, K, C, L, B), brake_harm_ladder_lds_bytes(T, K, C, L, B));
        }
      }
      printf("\n");
    } else {
      return 1;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("hidden_harm_ladder")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           str(d / "driver.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [ln.split() for ln in out[:-1]]
    return run


# ------------------------------------------------------------------------------------------------ the value rules
LOW, HIGH, LIMIT = 0.125, 0.75, 0.5                 # a harm below the limit and one above it
LEVELS = (1.0, 2.5, 6.0)


def _line(cells, C, L, B, finite, limit):
    """the driver's line and the checker's grid for the states ``cells [C][B][L]``: None = no hit, else the harm"""
    flat = " ".join(f"{0 if h is None else 1} {0.0 if h is None else h!r}" for c in range(C) for b in range(B) for h in cells[c][b])
    return f"H {C} {L} {B} {int(finite)} {limit!r} {' '.join(repr(a) for a in LEVELS[:L])} {flat}"


def _same(got, want, C, L, what):
    need, at, blocking, user, decel, need_of, harm_at, user_at = want[:8]
    assert [int(v) for v in got[:4]] == [need, at, blocking, user], (what, got, want[:8])
    assert float(got[4]) == decel and [int(v) for v in got[5:5 + C]] == need_of, (what, got, want[:8])
    curve = got[8:]
    assert [float(v) for v in curve[0::2]] == harm_at and [int(v) for v in curve[1::2]] == user_at, (what, got, want[:8])


@needs_cxx
def test_value_rules_against_the_checker_exhaustively(ask):
    """every pattern of {no hit, a harm below the limit, one above it, a NaN harm} over three classes x two levels at one brake start
    (4 096), every pattern of the first three over two classes x two levels x two brake starts (6 561) -- equal harms are everywhere,
    the classes share the two values -- and both with a non-finite candidate: need, at, blocking, user, decel, need_of, harm_at and
    user_at are the checker's"""
    lines, wants = [], []
    for states, (C, L, B) in (((None, LOW, HIGH, math.nan), (3, 2, 1)), ((None, LOW, HIGH), (2, 2, 2))):
        for n, combo in enumerate(itertools.product(states, repeat=C * B * L)):
            cells = [[list(combo[(c * B + b) * L:(c * B + b + 1) * L]) for b in range(B)] for c in range(C)]
            for finite in ((True, False) if n % 7 == 0 else (True,)):
                lines.append(_line(cells, C, L, B, finite, LIMIT))
                wants.append((RH.reduce_one(cells, LEVELS[:L], B, LIMIT, finite), C, L))
    assert len(lines) > 4096 + 6561
    seen = set()
    for ln, got, (want, C, L) in zip(lines, ask(lines), wants):
        _same(got, want, C, L, ln)
        seen.add((want[0], want[3]))
    assert {(-1 + 1, -1), (1, 0), (2, 0), (2, -2), (1, 1)} <= seen          # need 0 unblocked, blocked levels, "no level", fails closed


@needs_cxx
def test_value_rules_on_rows_written_out_by_hand(ask):
    """three levels, two starts, three classes, limit 0.5: start 0 is hit by class 1 at 0.75 at level 0 and by class 2 at 0.6 at level 1
    -> it needs level 2, blocked by class 2; start 1 is hit by class 0 at 0.4 everywhere -> level 0.  The curve: level 0 holds 0.75 of
    class 1, level 1 holds 0.6 of class 2, level 2 the 0.4 of class 0; with equal harms the lower class is named; a limit AT a harm does
    not count it as over; nothing hit is 0.0 / -1"""
    N_ = None
    cells = [[[N_, N_, N_], [0.4, 0.4, 0.4]], [[0.75, N_, N_], [N_, N_, N_]], [[N_, 0.6, N_], [N_, N_, N_]]]
    got = ask([_line(cells, 3, 3, 2, True, 0.5), _line(cells, 3, 3, 2, True, 0.75), _line(cells, 3, 3, 2, True, 0.6),
               _line([[[0.3, N_, N_]], [[0.3, N_, N_]]], 2, 3, 1, True, 0.1), _line([[[N_, N_, N_]]], 1, 3, 1, True, 0.0)])
    assert got[0] == ["2", "0", "4", "2", "6", "0", "1", "0", "0.75", "1", "0.59999999999999998", "2", "0.40000000000000002", "0"]
    assert got[1][:5] == ["0", "0", "0", "-1", "1"]                        # 0.75 is not above 0.75: every level suffices
    assert got[2][:5] == ["1", "0", "2", "1", "2.5"]                       # 0.6 is not above 0.6: level 1 suffices, class 1 blocks below
    assert got[3][:5] == ["1", "0", "3", "0", "2.5"] and got[3][8:] == ["0.29999999999999999", "0", "0", "-1", "0", "-1"]
    assert got[4] == ["0", "0", "0", "-1", "1", "0", "-1", "-1", "0", "-1", "0", "-1", "0", "-1"]
    for cells_, C, L, B, limit in ((cells, 3, 3, 2, 0.5), (cells, 3, 3, 2, 0.75)):
        _same(ask([_line(cells_, C, L, B, True, limit)])[0], RH.reduce_one(cells_, LEVELS[:L], B, limit), C, L, limit)


# ------------------------------------------------------------------------------------------------ the plan
@needs_cxx
def test_lds_bytes_against_the_bound_over_every_shape_a_call_admits(ask):
    """brake_harm_ladder_lds_bytes over T = 1 .. 254 x K = 1 .. 3 x L = 1 .. 64 x B in {1, 2, 3, 5, 8, 31, T} at the most classes the
    argument admits: the ladder verdict's bytes rounded up to 8, and 256 * 12 bytes of exchange exactly where a trajectory has more than
    a wave (G > 64); never above brake_harm_ladder_lds_bound, which is under the 64 KB of a workgroup"""
    from frenetix_occlusion import _native as N
    head = ask(["C"])[0]
    assert [int(v) for v in head] == [N.HIDDEN_VERDICT_NOT_FINITE, 2 ** 31 - 1, 256 * 12, 39568]
    bound, worst, with_exchange = 39568, 0, 0
    assert bound < 65536
    Ts = list(range(1, 255))
    got = ask([f"P {T} {K}" for T in Ts for K in (1, 2, 3)])
    for (T, K), row in zip(((T, K) for T in Ts for K in (1, 2, 3)), got):
        vals = [int(v) for v in row]
        assert len(vals) == 64 * 7 * 2
        for L in range(1, 65):
            for i, B in enumerate((1, 2, 3, 5, 8, 31, T)):
                base, mine = vals[((L - 1) * 7 + i) * 2:((L - 1) * 7 + i) * 2 + 2]
                if B > T:
                    assert (base, mine) == (0, 0)
                    continue
                _, G, _, _, lds = expected_plan(T, K, most_classes(T, L), L, B, 1)
                assert base == lds, (T, K, L, B)
                want = (base + 7) // 8 * 8 + (256 * 12 if G > 64 else 0)
                assert mine == want <= bound and mine % 8 == 0, (T, K, L, B, base, mine, want)
                worst, with_exchange = max(worst, mine), with_exchange + (G > 64)
    assert with_exchange > 0 and worst > 32768
    print(f"largest brake_harm_ladder_lds_bytes over the shapes: {worst} of {bound} bytes")


# ------------------------------------------------------------------------------------------------ the conditions of the device tests
def _conditions(sc, lu, what):
    """on one scene and its walk: the in-between limit exists, no hit's harm lies within 1e-9 of it, at least one hit is over it and one
    is not; no two classes' maxima at one (m, l) lie within 1e-9 of each other unless equal"""
    res = HC.check(sc, lu, 0.0)
    zero, inf, mid = HC.limits(res["hits"])
    assert (zero, inf) == (0.0, math.inf) and mid is not None, (what, "a scene with fewer than two distinct harms is no case: replace it")
    hits = np.array(res["hits"])
    assert np.isfinite(hits).all() and (hits > 0.0).all() and (hits < 1.0).all(), what
    assert np.abs(hits - mid).min() >= RH.OPEN_TOL and (hits > mid).any() and (hits < mid).any(), (what, mid)
    assert res["closest"] >= RH.OPEN_TOL, (what, res["closest"])
    at_mid = HC.check(sc, lu, mid)
    at_inf = HC.check(sc, lu, math.inf)
    for name in ("harm_at", "user_at", "first"):                             # the curve does not depend on the limit
        assert at_mid[name].tobytes() == res[name].tobytes() == at_inf[name].tobytes(), (what, name)
    assert (at_mid["need"] <= res["need"]).all() and (at_inf["need"] <= at_mid["need"]).all() and (at_inf["need"] <= 0).all(), what
    return res, at_mid, mid


def test_conditions_the_device_tests_rest_on():
    """every raw-entry scene tests/test_hidden_harm_ladder_gpu.py holds the device to the checker on -- the seven scenes of
    tests/hidden_harm_ladder_cases.CHECKER_CASES, the hand case, the non-monotone case -- by the checker alone on the walk of
    tests/ref_hidden_brake_ladder_users.py; and the consequences (a) - (d) of the definition on them"""
    import ref_hidden_brake_ladder_verdict as LV
    moved = 0
    for spec in HC.CHECKER_CASES:
        sc, lu = S.checked(spec)
        res, at_mid, mid = _conditions(sc, lu, spec)
        # (a): at limit 0 every hit is over -- the ladder verdict's fold of the ladder-users outputs
        want = LV.verdict(lu.required_all, lu.blocking, lu.required, lu.first, list(sc.levels), sc.starts, sc.T, sc.lens)
        for name in RH.SHARED:
            assert res[name].tobytes() == want[name].tobytes(), (spec, name)
        # (c)
        L = len(sc.levels)
        below = at_mid["harm_at"] <= mid
        lowest = np.where(below.any(axis=1), below.argmax(axis=1), L)
        asked = at_mid["need"] >= 0
        assert (at_mid["need"][asked] <= lowest[asked]).all() and (at_mid["harm_at"][at_mid["need"] == L] > mid).all(), spec
        moved += int((at_mid["need"] < res["need"]).sum())
    assert moved > 0                                                         # the in-between limit changes an answer somewhere
    h = HC.hand_case()
    import hidden_brake_scenes as SC
    import ref_hidden_brake_ladder_users as LU
    lu = LU.ladder_users(h.keys, h.win, h.road, h.qmins, SC.ORIGIN, SC.CS, h.x, h.y, h.head, h.arc, h.v, SC.HL, SC.HW, SC.WB, h.levels, h.starts,
                         h.dt, h.thr, h.map_of, h.lens)
    assert lu.brake_first.tolist() == [[[[2, 2]]], [[[2, 2]]]] and lu.stop.tolist() == [[[8, 4]]] and lu.required_all.tolist() == [[-1]]
    res = RH.harm_ladder(lu.brake_first, lu.stop, lu.first, h.v, list(h.levels), h.dt, 1, h.rows.tolist(), h.speed_of, HC.HAND_LIMIT)
    assert res["hits"] == [HC.HAND_PED[0], HC.HAND_CAR[0], HC.HAND_PED[1], HC.HAND_CAR[1]]
    assert HC.HAND_PED[1] + RH.OPEN_TOL < HC.HAND_LIMIT < HC.HAND_PED[0] - RH.OPEN_TOL and max(HC.HAND_CAR) < HC.HAND_LIMIT
    assert (res["need"].tolist(), res["at"].tolist(), res["blocking"].tolist(), res["user"].tolist(), res["decel"].tolist()) == ([1], [0], [1], [0], [4.0])
    assert res["harm_at"].tolist() == [list(HC.HAND_PED)] and res["user_at"].tolist() == [[0, 0]] and res["closest"] >= RH.OPEN_TOL
    assert abs(HC.HAND_PED[0] - 1.0 / (1.0 + math.exp(3.164 - 0.26951159804844643 * 8.0))) <= 1e-15
    n = HC.non_monotone_case()
    lu = S.check(n)
    res = RH.harm_ladder(lu.brake_first, lu.stop, lu.first, n.v, list(n.levels), n.dt, 1, n.rows.tolist(), n.speed_of, 0.05)
    assert res["harm_at"][0, 0] == 0.0 < res["harm_at"][0, 1] and res["harm_at"][0, 2] == 0.0 and res["user_at"][0].tolist() == [-1, 0, -1]
    assert res["need"][0] == 0 and np.abs(np.array(res["hits"]) - 0.05).min() >= RH.OPEN_TOL      # the first sufficient level, not the last insufficient one


# ------------------------------------------------------------------------------------------------ the library and the Python layers
def test_library_exports_the_entry_and_keeps_the_abi():
    from frenetix_occlusion import _native as N
    import ctypes as C
    lib = N.load()
    assert "fo_scene_hidden_brake_harm_ladder" in N.EXPORTS and hasattr(lib, "fo_scene_hidden_brake_harm_ladder")
    assert lib.fo_abi_version() == 12
    # the ladder verdict's structure, and: speed_of, rows, harm_limit, harm_at, user_at
    assert C.sizeof(N.HiddenBrakeHarmLadder) == C.sizeof(N.HiddenBrakeLadderVerdict) + 5 * 8
    assert [n for n, _ in N.HiddenBrakeHarmLadder._fields_][:len(N.HiddenBrakeLadderVerdict._fields_)] == [n for n, _ in N.HiddenBrakeLadderVerdict._fields_]


def _hl(**over):
    kw = dict(vehicle=(4.5, 1.8, 1.4), ego_mass=1200.0, users=((2.0, "road", "any"),), kinds=(("Pedestrian", 0.4, 0.6),), dt=0.1, starts=5,
              harm_limit=0.1)
    kw.update(over)
    return kw


def test_stage_options_without_a_gpu():
    """two of the four stages are refused before anything is allocated; the new stage's dict is checked like its siblings'; the
    existing option functions answer their current callers as before"""
    from frenetix_occlusion.step import PlanningStep, hidden_ladder_verdict_options, hidden_stage_options, hidden_stages
    stage = SimpleNamespace(ctx=object())
    iv = dict(_hl(), a_brake=8.0)
    hv = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, a_brake=8.0, starts=5, commit_min=5)
    lv = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, levels=[1.0, 2.0], starts=5, a_limit=8.0)
    step = lambda **kw: PlanningStep(stage, stage, stage, None, None, None, None, **kw)
    for two in (dict(hidden_verdict=hv, hidden_harm_ladder_verdict=_hl()), dict(hidden_ladder_verdict=lv, hidden_harm_ladder_verdict=_hl()),
                dict(hidden_impact_verdict=iv, hidden_harm_ladder_verdict=_hl()),
                dict(hidden_verdict=hv, hidden_ladder_verdict=lv, hidden_impact_verdict=iv, hidden_harm_ladder_verdict=_hl())):
        with pytest.raises(ValueError, match="same two reserved cost columns"):
            step(**two)
    for bad in (dict(users=_hl()["users"]), {k: v for k, v in _hl().items() if k != "harm_limit"}, _hl(a_brake=8.0), _hl(commit_min=1),
                _hl(approach="lanes"), 5, "kinds"):
        with pytest.raises(ValueError, match="hidden_harm_ladder_verdict"):
            step(hidden_harm_ladder_verdict=bad)
    assert hidden_stages(None, None, None, None) == (None, None, None) and hidden_stages(hv, None, None, None) == (None, None, None)
    given = _hl(levels=[1.0, 2.0], a_limit=4.0, coeff=dict(a=1), lengths=[1], margin=0.5, inflate=0.1)
    got = hidden_stages(None, None, None, given)[2]
    assert got == given and got is not given
    assert hidden_stage_options(None, None, None) == (None, None) and hidden_stage_options(None, lv, None)[0] == lv
    assert hidden_ladder_verdict_options(None, lv) == lv and hidden_stage_options(None, None, iv)[1] == iv
    with pytest.raises(ValueError, match="same two reserved cost columns"):
        hidden_stage_options(hv, lv, None)


def test_refusals_of_the_sensor_model_call_without_a_gpu():
    """what SensorModel.hidden_brake_harm_ladder refuses before it touches the device"""
    from frenetix_occlusion.hidden_traffic import HiddenBrakeHarmLadder, hidden_brake_harm_ladder
    from frenetix_occlusion.sensor_model import SensorModel
    assert SensorModel.hidden_brake_harm_ladder is hidden_brake_harm_ladder
    x = np.zeros((2, 8))
    sm = SimpleNamespace()
    call = lambda **over: hidden_brake_harm_ladder(sm, x, x, x, x, **_hl(**over))
    for bad in (dict(users=()), dict(a_limit=-1.0), dict(a_limit=float("nan")), dict(a_limit="fast"), dict(levels=None),
                dict(levels=[2.0, 1.0]), dict(levels=[]), dict(levels=[-1.0]), dict(levels=list(range(1, 66))), dict(kinds=()),
                dict(levels=[1.0], kinds=(("Pedestrian", 0.4),)), dict(levels=[1.0], harm_limit=-0.1), dict(levels=[1.0], harm_limit=float("nan")),
                dict(levels=[1.0], harm_limit=None)):
        with pytest.raises(ValueError, match="hidden_brake_harm_ladder"):
            call(**bad)
    import torch
    t = lambda *shape: torch.zeros(shape)
    res = HiddenBrakeHarmLadder(need=t(3), at=t(3), blocking=t(3), user=torch.tensor([0, -1, -2], dtype=torch.int32), decel=torch.tensor([2.0, 0.0, math.inf]),
                                need_of=t(1, 3), first=t(1, 3), harm_at=torch.tensor([[0.3, 0.2, 0.2], [0.0, 0.1, 0.0], [1.0, 1.0, 1.0]]),
                                user_at=t(3, 3), levels=np.array([1.0, 2.0, 4.0]), starts=5, harm_limit=0.1, a_limit=math.inf,
                                rows=np.zeros((1, 4)), speed_of=np.zeros(1))
    assert res.monotone().tolist() == [True, False, True] and res.required_deceleration() is res.decel
    assert res.brake_threat_number(4.0).tolist() == [0.5, 0.0, math.inf] and res.critical_user().tolist() == [0, -1, -2]
    levels, harm_at, user_at = res.harm_curve()
    assert levels is res.levels and harm_at is res.harm_at and user_at is res.user_at
