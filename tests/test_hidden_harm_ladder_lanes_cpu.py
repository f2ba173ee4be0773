"""The host side of the hidden-traffic harm ladder by approach angle (DESIGN.md §5.10 "Harm ladder by approach angle"), without a GPU:
the plain statement tests/ref_hidden_brake_harm_ladder_lanes.py against its two parents' checkers; the conditions the device tests
rest on -- no open choice on any scene and limit they use -- by the checkers alone on the walk of
tests/ref_hidden_brake_ladder_users.py; the plan's LDS function (csrc/fo_scene_plan.hpp brake_harm_ladder_lanes_lds_bytes) built with
the host C++ compiler against its formula and bound; the hand numbers from the rows alone; the refusals of the Python layers that need
no GPU; the library's symbol."""
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_scenes as SC
import hidden_harm_ladder_lanes_cases as HLC
import hidden_impact_lanes_cases as LC
import ref_hidden_brake_harm_ladder as RH
import ref_hidden_brake_users as BU
import ref_hidden_impact_lanes as RL
import ref_hidden_reach_flow as RF
from test_hidden_brake_ladder_verdict_cpu import expected_plan, most_classes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
TOL = 1e-9

DRIVER = r"""
#include <cstdio>
#include "fo_scene_plan.hpp"
static const int BS[6] = {1, 2, 3, 5, 8, 31};
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'C') {          // C -> the two bounds
      printf("%zu %zu\n", brake_harm_ladder_lds_bound(), brake_harm_ladder_lanes_lds_bound());
    } else if (what == 'P') {   // P T K -> for L = 1 .. 64, B in {1, 2, 3, 5, 8, 31, T} (those <= T; else zeros), at the most classes C <= 8 that T and
                                // L admit: C, the harm ladder's bytes and this stage's
      int T, K;
      if (scanf("%d %d", &T, &K) != 2) return 1;
      for (int L = 1; L <= 64; ++L) {
        int C = 8;
        while (C > 1 && (C * T > BRAKE_USERS_MAX_TABLE || 4 * C * T + 8 * L > BRAKE_LADDER_USERS_MAX_ARG_BYTES)) --C;
        for (int i = 0; i < 7; ++i) {
          const int B = i < 6 ? BS[i] : T;
          if (B > T) { printf("0 0 0 "); continue; }
          printf("%d %zu %zu ", C, brake_harm_ladder_lds_bytes(T, K, C, L, B), brake_harm_ladder_lanes_lds_bytes(T, K, C, L, B));
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
    d = tmp_path_factory.mktemp("hidden_harm_ladder_lanes")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           str(d / "driver.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [ln.split() for ln in out[:-1]]
    return run


# ------------------------------------------------------------------------------------------------ the plan
@needs_cxx
def test_lds_bytes_against_the_formula_and_the_bound(ask):
    """brake_harm_ladder_lanes_lds_bytes over the (T, K, L, B) of the ladder verdict's plan test -- T = 1 .. 254 x K = 1 .. 3 x L = 1 .. 64 x
    B in {1, 2, 3, 5, 8, 31, T} at the most classes the argument admits: the harm ladder's bytes (a multiple of 8) and one float64 per
    class and trajectory of the workgroup behind them; never above brake_harm_ladder_lanes_lds_bound, the harm ladder's bound and 256
    trajectories of 8 classes, which is under the 64 KB of a workgroup"""
    bounds = [int(v) for v in ask(["C"])[0]]
    assert bounds == [39568, 39568 + 256 * 8 * 8] and bounds[1] < 65536
    worst, most = 0, 0
    Ts = list(range(1, 255))
    got = ask([f"P {T} {K}" for T in Ts for K in (1, 2, 3)])
    for (T, K), row in zip(((T, K) for T in Ts for K in (1, 2, 3)), got):
        vals = [int(v) for v in row]
        assert len(vals) == 64 * 7 * 3
        for L in range(1, 65):
            for i, B in enumerate((1, 2, 3, 5, 8, 31, T)):
                C_, base, mine = vals[((L - 1) * 7 + i) * 3:((L - 1) * 7 + i) * 3 + 3]
                if B > T:
                    assert (C_, base, mine) == (0, 0, 0)
                    continue
                assert C_ == most_classes(T, L)
                _, _, per, _, _ = expected_plan(T, K, C_, L, B, 1)
                assert base % 8 == 0 and mine == base + per * C_ * 8 <= bounds[1], (T, K, L, B, base, mine, per, C_)
                worst, most = max(worst, mine), max(most, per * C_ * 8)
    assert most == 256 * 8 * 8 and worst > 32768                            # B = 1, L = 1: a lane a trajectory, eight classes each
    print(f"largest brake_harm_ladder_lanes_lds_bytes over the shapes: {worst} of {bounds[1]} bytes; the met harms take up to {most}")


# ------------------------------------------------------------------------------------------------ checker against checker
def _head_on(sc, lu, limit):
    return RH.harm_ladder(lu.brake_first, lu.stop, lu.first, sc.v, list(sc.levels), sc.dt, sc.starts, sc.rows.tolist(), sc.speed_of, limit, sc.lens)


def _same(a, b, what, names=RH.OUTPUTS):
    for name in names:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (what, name)


@pytest.fixture(scope="module")
def walks():
    """every raw scene with its ladder-users walk on the host, once"""
    out = []
    for case in range(len(HLC.RAW_CASES)):
        sc = HLC.raw_case(case)
        out.append((sc, HLC.walk_on_the_host(sc)))
    return out


def test_checker_against_the_checkers_of_its_parents(walks):
    """on every raw scene: (a) with dir_mask = 0, with a table of 0xFF alone and with heading_slack = pi the new checker is
    tests/ref_hidden_brake_harm_ladder.harm_ladder in every bit of every output, at limit 0, at the scene's limits and at inf; (b) with
    the scene's own mask, table and slack no ho, no harm_at, no need and no need_of is above head-on's; (c) harm_at[:, l] is the obstacle
    harm of tests/ref_hidden_impact_lanes.impact_lanes at a_brake = levels[l] on the users walk of that level, and user_at its user"""
    below = 0
    for case, (sc, lu) in enumerate(walks):
        what = HLC.RAW_CASES[case]
        own = HLC.check(sc, lu, 0.0)
        lims = HLC.limits(own["hits"])
        every = (1 << len(sc.thr)) - 1
        for limit in (0.0, math.inf) + lims:
            ref = _head_on(sc, lu, limit)
            for name, kw in (("dir_mask = 0", dict(mask=0)), ("a table of 0xFF", dict(mask=every, moves=LC.table("any"))),
                             ("slack = pi", dict(mask=every, slack=math.pi))):
                _same(HLC.check(sc, lu, limit, **kw), ref, (what, limit, name))                 # (a)
            got = HLC.check(sc, lu, limit)
            assert (got["harm_at"] <= ref["harm_at"]).all() and (got["need"] <= ref["need"]).all(), (what, limit)     # (b)
            assert (got["need_of"] <= ref["need_of"]).all() and np.array_equal(got["first"], ref["first"]), (what, limit)
            _same(got, own, (what, limit, "the curve does not depend on the limit"), ("harm_at", "user_at", "first"))
        head = HLC.check(sc, lu, 0.0, mask=0)["ho"]
        hit = ~np.isnan(own["ho"])
        assert np.array_equal(hit, ~np.isnan(head)) and (own["ho"][hit] <= head[hit]).all(), what
        below += int((own["harm_at"] < _head_on(sc, lu, 0.0)["harm_at"]).sum())
        cos_h, sin_h = RL.host_h(sc.slack)
        for l, level in enumerate(sc.levels):                                                   # (c)
            bf, stop, _, first = BU.brake_users(sc.keys, sc.win, sc.road, sc.qmins, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW,
                                                SC.WB, float(level), sc.dt, sc.thr, sc.map_of, sc.lens)
            assert np.array_equal(np.asarray(bf)[:, :, :sc.starts], lu.brake_first[..., l]) and np.array_equal(first, lu.first), (what, l)
            harm, user, _, _, _, n_open, _ = RL.impact_lanes(sc.keys, sc.win, sc.road, sc.moves, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v,
                                                             SC.HL, SC.HW, SC.WB, float(level), sc.dt, sc.thr, sc.map_of, sc.starts, sc.rows.tolist(),
                                                             sc.speed_of, sc.mask, cos_h, sin_h, bf, stop, first, sc.lens)
            assert n_open == 0 and np.abs(own["harm_at"][:, l] - harm[:, 0]).max() <= 1e-15, (what, l)
            assert np.array_equal(own["user_at"][:, l], user), (what, l)
    print(f"{below} pairs (m, l) with harm_at strictly below head-on over the raw scenes")
    assert below >= 10


def test_no_open_choice_on_any_scene_and_limit_of_the_device_test(walks):
    """the condition -- not a tolerance -- under which tests/test_hidden_harm_ladder_lanes_gpu.py compares integers exactly: on every raw
    scene and each of its two limits no ho lies within 1e-9 of the limit and no two classes' level maxima lie within 1e-9 of each other
    unless equal; each limit lies strictly between two recorded harms, with at least one hit over it and one under it; no scene is left
    out.  The same on the hand scenes at HAND_LIMIT."""
    for case, (sc, lu) in enumerate(walks):
        what = HLC.RAW_CASES[case]
        own = HLC.check(sc, lu, 0.0)
        lims = HLC.limits(own["hits"])
        assert lims is not None and len(set(lims)) == 2, (what, "a scene with fewer than three distinct harms is no case: replace it")
        hits = np.array(own["hits"])
        assert np.isfinite(hits).all() and (hits > 0.0).all() and (hits < 1.0).all(), what
        assert own["closest"] >= RH.OPEN_TOL, (what, own["closest"])
        for limit in lims:
            assert np.abs(hits - limit).min() >= RH.OPEN_TOL and (hits > limit).any() and (hits < limit).any(), (what, limit)
            got = HLC.check(sc, lu, limit)
            assert (got["need"] <= own["need"]).all() and got["closest"] >= RH.OPEN_TOL, (what, limit)
    for byte in (RF.sector(90), RF.sector(180), RF.ANY):
        h = HLC.hand_case(byte)
        got = HLC.check(h, HLC.walk_on_the_host(h), HLC.HAND_LIMIT)
        assert len(got["hits"]) == 2 and np.abs(np.array(got["hits"]) - HLC.HAND_LIMIT).min() >= 1e-4, byte


# ------------------------------------------------------------------------------------------------ the hand numbers
def test_hand_numbers_from_the_rows_alone():
    """a car at 13.9 m/s against an east-bound ego that has 6 m/s and 4 m/s left at the hit: head-on 0.03461676 / 0.03176490, from a
    north-bound cross lane at cosine = cos 67.5 deg 0.03071336 / 0.02909951 -- by CAR_ROW and the logistic alone; the limit 0.030 lies
    strictly between the two approaches at 4 m/s and below both at 6 m/s; and the checker on the hand scene says so: need 2 head-on, from
    the oncoming lane and from an off-lane cell, need 1 from the cross lane"""
    p0, p1 = LC.CAR_ROW[:2]
    for n, u in enumerate(HLC.HAND_U):
        head = 1.0 / (1.0 + math.exp(p0 + p1 * (u + 13.9)))
        cross = 1.0 / (1.0 + math.exp(p0 + p1 * math.sqrt(u * u + 13.9 * 13.9 + 2.0 * u * 13.9 * LC.COS_67_5)))
        assert abs(head - HLC.HAND_HEAD_ON[n]) <= 1e-14 and abs(cross - HLC.HAND_CROSS[n]) <= 1e-14, (u, head, cross)
        assert HLC.hand_harm(u, 1.0) == head and abs(HLC.hand_harm(u, LC.COS_67_5) - cross) <= 1e-15
    assert abs(LC.COS_67_5 - math.cos(math.radians(67.5))) <= 1e-15
    assert HLC.HAND_CROSS[1] < HLC.HAND_LIMIT < HLC.HAND_HEAD_ON[1] and HLC.HAND_LIMIT < min(HLC.HAND_CROSS[0], HLC.HAND_HEAD_ON[0])
    for byte, need, harm_at in ((RF.sector(90), 1, HLC.HAND_CROSS), (RF.sector(180), 2, HLC.HAND_HEAD_ON), (RF.ANY, 2, HLC.HAND_HEAD_ON)):
        h = HLC.hand_case(byte)
        lu = HLC.walk_on_the_host(h)
        assert lu.brake_first.tolist() == [[[[2, 2]]]] and lu.first.tolist() == [[2]]
        got = HLC.check(h, lu, HLC.HAND_LIMIT)
        assert got["need"].tolist() == [need] and got["decel"].tolist() == [4.0 if need == 1 else math.inf], (byte, got["need"])
        assert np.abs(got["harm_at"][0] - np.array(harm_at)).max() <= 1e-14 and got["user_at"].tolist() == [[0, 0]], byte
        ref = HLC.check(h, lu, HLC.HAND_LIMIT, mask=0)                      # the same car, not lane-bound: head-on, "no level"
        assert ref["need"].tolist() == [2] and np.abs(ref["harm_at"][0] - np.array(HLC.HAND_HEAD_ON)).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ the library and the Python layers
def test_library_exports_the_entry_and_keeps_the_abi():
    from frenetix_occlusion import _native as N
    import ctypes as C
    lib = N.load()
    assert "fo_scene_hidden_brake_harm_ladder_lanes" in N.EXPORTS and hasattr(lib, "fo_scene_hidden_brake_harm_ladder_lanes")
    assert lib.fo_abi_version() == 12
    head = N.HiddenBrakeHarmLadder._fields_
    assert N.HiddenBrakeHarmLadderLanes._fields_[:len(head)] == head        # the harm ladder's members in their order, and behind them:
    assert [n for n, _ in N.HiddenBrakeHarmLadderLanes._fields_[len(head):]] == ["dir_mask", "cos_h", "sin_h"]
    assert C.sizeof(N.HiddenBrakeHarmLadderLanes) == C.sizeof(N.HiddenBrakeHarmLadder) + 3 * 8
    assert N.HiddenBrakeHarmLadderLanes.dir_mask.offset == C.sizeof(N.HiddenBrakeHarmLadder)


def _hl(**over):
    kw = dict(vehicle=(4.5, 1.8, 1.4), ego_mass=1200.0, users=((2.0, "road", "any"),), kinds=(("Pedestrian", 0.4, 0.6),), dt=0.1, starts=5,
              harm_limit=0.1)
    kw.update(over)
    return kw


def test_stage_options_without_a_gpu():
    """any two of the five stages are refused before anything is allocated; the new stage's dict is checked like its siblings' and takes
    heading_slack; the existing option functions answer as before"""
    from frenetix_occlusion.step import PlanningStep, hidden_stage_options, hidden_stages, hidden_stages_lanes
    stage = SimpleNamespace(ctx=object())
    iv = dict(_hl(), a_brake=8.0)
    hv = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, a_brake=8.0, starts=5, commit_min=5)
    lv = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, levels=[1.0, 2.0], starts=5, a_limit=8.0)
    step = lambda **kw: PlanningStep(stage, stage, stage, None, None, None, None, **kw)
    five = dict(hidden_verdict=hv, hidden_ladder_verdict=lv, hidden_impact_verdict=iv, hidden_harm_ladder_verdict=_hl(),
                hidden_harm_ladder_lanes_verdict=_hl(heading_slack=0.1))
    names = sorted(five)
    for a in range(5):
        for b in range(a + 1, 5):
            with pytest.raises(ValueError, match="same two reserved cost columns"):
                step(**{names[a]: five[names[a]], names[b]: five[names[b]]})
    with pytest.raises(ValueError, match="same two reserved cost columns"):
        step(**five)
    for bad in (dict(users=_hl()["users"]), {k: v for k, v in _hl().items() if k != "harm_limit"}, _hl(a_brake=8.0), _hl(commit_min=1),
                _hl(approach="lanes"), 5, "kinds"):
        with pytest.raises(ValueError, match="hidden_harm_ladder_lanes_verdict"):
            step(hidden_harm_ladder_lanes_verdict=bad)
    with pytest.raises(ValueError, match="hidden_harm_ladder_verdict"):     # the head-on stage still takes neither keyword
        step(hidden_harm_ladder_verdict=_hl(heading_slack=0.1))
    assert hidden_stages_lanes(None, None, None, None, None) == (None, None, None, None)
    given = _hl(levels=[1.0, 2.0], a_limit=4.0, coeff=dict(a=1), lengths=[1], margin=0.5, inflate=0.1, heading_slack=0.2)
    got = hidden_stages_lanes(None, None, None, None, given)
    assert got[:3] == (None, None, None) and got[3] == given and got[3] is not given
    assert hidden_stages(None, None, None, None) == (None, None, None) and hidden_stages(None, None, None, _hl())[2] == _hl()
    assert hidden_stage_options(None, lv, None)[0] == lv and hidden_stages_lanes(None, lv, iv and None, None, None)[0] == lv


def test_refusals_of_the_sensor_model_call_without_a_gpu():
    """what SensorModel.hidden_brake_harm_ladder_lanes refuses before it touches the device: its sibling's list, a bad heading_slack, a
    lane-bound user without a move table; and the result's new trailing fields have defaults"""
    from frenetix_occlusion.hidden_traffic import HiddenBrakeHarmLadder, hidden_brake_harm_ladder_lanes
    from frenetix_occlusion.interface import FOInterface
    from frenetix_occlusion.sensor_model import SensorModel
    assert SensorModel.hidden_brake_harm_ladder_lanes is hidden_brake_harm_ladder_lanes and hasattr(FOInterface, "hidden_brake_harm_ladder_lanes")
    x = np.zeros((2, 8))
    sm = SimpleNamespace(lane_moves=None)
    call = lambda **over: hidden_brake_harm_ladder_lanes(sm, x, x, x, x, **_hl(**over))
    lane = ((7.0, "road", "lanes"),)
    for bad in (dict(users=()), dict(a_limit=-1.0), dict(a_limit=float("nan")), dict(levels=None), dict(levels=[2.0, 1.0]), dict(levels=[]),
                dict(kinds=()), dict(levels=[1.0], harm_limit=-0.1), dict(levels=[1.0], harm_limit=None),
                dict(levels=[1.0], heading_slack=-0.1), dict(levels=[1.0], heading_slack=float("nan")), dict(levels=[1.0], heading_slack=math.inf),
                dict(levels=[1.0], heading_slack="wide"), dict(levels=[1.0], users=lane)):
        with pytest.raises(ValueError, match="hidden_brake_harm_ladder_lanes"):
            call(**bad)
    with pytest.raises(ValueError, match="heading_slack"):                  # named before anything behind it
        call(heading_slack=-1.0, levels=[2.0, 1.0], harm_limit=-1.0)
    with pytest.raises(ValueError, match="lane_moves is None"):
        call(users=lane, levels=[2.0, 1.0])
    with pytest.raises(TypeError):
        call(approach="lanes")
    import torch
    t = lambda *shape: torch.zeros(shape)
    res = HiddenBrakeHarmLadder(need=t(3), at=t(3), blocking=t(3), user=t(3), decel=t(3), need_of=t(1, 3), first=t(1, 3), harm_at=t(3, 3),
                                user_at=t(3, 3), levels=np.array([1.0, 2.0, 4.0]), starts=5, harm_limit=0.1, a_limit=math.inf,
                                rows=np.zeros((1, 4)), speed_of=np.zeros(1))
    assert res.approach == "head_on" and res.heading_slack == 0.0
