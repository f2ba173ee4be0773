"""The host side of the hidden-traffic impact verdict (DESIGN.md §5.10 "Impact verdict"), without a GPU: the harm rows, the logistics,
the choice of the class and the fold (csrc/fo_hidden_impact.hpp) built with the host C++ compiler, as
tests/test_hidden_brake_verdict_cpu.py builds csrc/fo_hidden_verdict.hpp -- against the reference's own harm
(tests/golden/hidden_impact_harm.npz) and against the plain statement tests/ref_hidden_impact.py; the condition the device tests rest
on -- no open choice of the class in any of their scenes -- by the checker alone; the library's symbols."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import hidden_impact_cases as IC
import ref_hidden_impact as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
TOL = 1e-9                                          # the project's stated float tolerance (README, "GPU vs oracle")
TYPE_CODE = {"car": 0, "truck": 1, "bus": 2, "bicycle": 3, "pedestrian": 4, "priorityvehicle": 5, "parkedvehicle": 6, "train": 7,
             "motorcycle": 8, "taxi": 9, "unknown": 10}                # FO_TYPE_* (include/fo_hip.h)

DRIVER = r"""
#include <cstdio>
#include "fo_hidden_verdict.hpp"
#include "fo_hidden_impact.hpp"
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'C') {          // C -> FO_C_SAFE FO_C_RES0 FO_C_RES1 FO_NC NOT_FINITE
      printf("%d %d %d %d %d\n", FO_C_SAFE, FO_C_RES0, FO_C_RES1, FO_NC, FO_HIDDEN_VERDICT_NOT_FINITE);
    } else if (what == 'R') {   // R type size ego_mass, the eight coefficients -> ok p0 p1 p2 p3
      int type;
      double size, ego_mass, c[8], row[4] = {0.0, 0.0, 0.0, 0.0};
      if (scanf("%d %lf %lf", &type, &size, &ego_mass) != 3) return 1;
      for (int i = 0; i < 8; ++i) if (scanf("%lf", c + i) != 1) return 1;
      const fo_harm_coeff_t hc{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
      const bool ok = fo_hidden_impact_row_of(type, size, ego_mass, hc, row);
      printf("%d %.17g %.17g %.17g %.17g\n", (int)ok, row[0], row[1], row[2], row[3]);
    } else if (what == 'L') {   // L p_const p_speed w -> the logistic
      double a, b, w;
      if (scanf("%lf %lf %lf", &a, &b, &w) != 3) return 1;
      printf("%.17g\n", fo_hidden_impact_logistic(a, b, w));
    } else if (what == 'V') {   // V C finite safe harm_limit, four speeds, four ats, four speed_of, sixteen row entries, sixteen costs
      int C, finite, safe_in;   //   -> obst_harm ego_harm user safe + the sixteen
      double limit, speed[4], speed_of[4], rows[16], cost[FO_NC];
      int32_t at[4];
      if (scanf("%d %d %d %lf", &C, &finite, &safe_in, &limit) != 4) return 1;
      for (int i = 0; i < 4; ++i) if (scanf("%lf", speed + i) != 1) return 1;
      for (int i = 0; i < 4; ++i) if (scanf("%d", at + i) != 1) return 1;
      for (int i = 0; i < 4; ++i) if (scanf("%lf", speed_of + i) != 1) return 1;
      for (int i = 0; i < 16; ++i) if (scanf("%lf", rows + i) != 1) return 1;
      for (int i = 0; i < FO_NC; ++i) if (scanf("%lf", cost + i) != 1) return 1;
      const fo_hidden_impact_t r = fo_hidden_impact_classes<4>(speed, at, C, rows, speed_of, finite != 0);
      uint8_t safe = (uint8_t)safe_in;
      fo_hidden_impact_fold(r, limit, cost, &safe);
      printf("%.17g %.17g %d %d", r.obst_harm, r.ego_harm, r.user, (int)safe);
      for (int i = 0; i < FO_NC; ++i) printf(" %.17g", cost[i]);
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
    d = tmp_path_factory.mktemp("hidden_impact")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           str(d / "driver.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [ln.split() for ln in out[:-1]]
    return run


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "hidden_impact_harm.npz"))


def _num(s):
    return float(s)                                 # ("nan", "inf" and "-inf" as printf writes them)


def _r(v):
    return repr(float(v))                           # (a numpy scalar's own repr names its type)


# ------------------------------------------------------------------------------------------------ rows and logistics
@needs_cxx
def test_the_header_names_the_columns_the_checker_names(ask):
    from frenetix_occlusion import _native as N
    got = [int(v) for v in ask(["C"])[0]]
    assert got == [RI.C_SAFE, RI.C_RES0, RI.C_RES1, RI.NC, RI.NOT_FINITE] == [N.COST["safe"], 14, 15, N.NC, N.HIDDEN_VERDICT_NOT_FINITE]
    assert TYPE_CODE == N.TYPE_CODES


def _header_rows(ask, golden):
    coeff = " ".join(repr(float(c)) for c in golden["coeff"])
    lines = [f"R {TYPE_CODE[str(k).lower()]} {float(l) * float(w)!r} {float(golden['ego_mass'])!r} {coeff}"
             for k, (l, w) in zip(golden["kinds"], golden["dims"])]
    got = ask(lines)
    assert all(g[0] == "1" for g in got)
    return np.array([[_num(v) for v in g[1:]] for g in got])


@needs_cxx
def test_rows_attain_the_references_harm_at_the_bound(ask, golden):
    """the reference's unmodified get_harm on pairs built to attain the bound -- head-on, both angles of impact in the worst area -- for
    Car, Bicycle, Pedestrian and Truck x ego speeds {0, 0.5, 3, 8, 15} x user speeds {2.0, 7.0, 13.9}: the header's rows and logistics
    give its ego and obstacle harm to 1e-9, and so do the checker's"""
    assert [str(k) for k in golden["kinds"]] == ["Car", "Bicycle", "Pedestrian", "Truck"]
    assert sorted(set(golden["bound_v_ego"].tolist())) == [0.0, 0.5, 3.0, 8.0, 15.0] and sorted(set(golden["bound_v_obs"].tolist())) == [2.0, 7.0, 13.9]
    assert len(golden["bound_kind"]) == 60 and np.array_equal(golden["coeff"], np.array(list(RI.COEFF.values())))
    rows = _header_rows(ask, golden)
    ref_rows = np.array([RI.row(str(k), l, w, float(golden["ego_mass"])) for k, (l, w) in zip(golden["kinds"], golden["dims"])])
    assert np.abs(rows - ref_rows).max() <= 1e-15
    lines = []
    for k, ve, vo in zip(golden["bound_kind"], golden["bound_v_ego"], golden["bound_v_obs"]):
        lines += [f"L {_r(rows[k, 0])} {_r(rows[k, 1])} {_r(float(ve) + float(vo))}", f"L {_r(rows[k, 2])} {_r(rows[k, 3])} {_r(float(ve) + float(vo))}"]
    got = np.array([_num(g[0]) for g in ask(lines)]).reshape(-1, 2)
    worst_o, worst_e = np.abs(got[:, 0] - golden["bound_obst_harm"]).max(), np.abs(got[:, 1] - golden["bound_ego_harm"]).max()
    print(f"rows against the reference at the bound: worst |obstacle harm| difference {worst_o:.3e}, ego {worst_e:.3e}")
    assert worst_o <= TOL and worst_e <= TOL
    for n, (k, ve, vo) in enumerate(zip(golden["bound_kind"], golden["bound_v_ego"], golden["bound_v_obs"])):
        w = float(ve) + float(vo)
        assert abs(RI.logistic(ref_rows[k, 0], ref_rows[k, 1], w) - golden["bound_obst_harm"][n]) <= TOL
        assert abs(RI.logistic(ref_rows[k, 2], ref_rows[k, 3], w) - golden["bound_ego_harm"][n]) <= TOL
    assert golden["bound_obst_harm"].min() > 0.0 and golden["bound_obst_harm"].max() < 1.0 and len(set(golden["bound_obst_harm"].tolist())) > 40


@needs_cxx
def test_no_recorded_reference_harm_exceeds_the_rows(ask, golden):
    """256 random yaws, positions and speeds per type: the reference's harm never exceeds the row's at w = v_ego + v_obs by more than
    1e-12 -- a larger excess would be a defect in the rows"""
    rows = _header_rows(ask, golden)
    assert all((golden["rand_kind"] == k).sum() >= 200 for k in range(4))
    lines = []
    for k, ve, vo in zip(golden["rand_kind"], golden["rand_v_ego"], golden["rand_v_obs"]):
        lines += [f"L {_r(rows[k, 0])} {_r(rows[k, 1])} {_r(float(ve) + float(vo))}", f"L {_r(rows[k, 2])} {_r(rows[k, 3])} {_r(float(ve) + float(vo))}"]
    got = np.array([_num(g[0]) for g in ask(lines)]).reshape(-1, 2)
    excess_o, excess_e = (golden["rand_obst_harm"] - got[:, 0]).max(), (golden["rand_ego_harm"] - got[:, 1]).max()
    print(f"random pairs: largest excess of the reference's obstacle harm over the row's {excess_o:.3e}, of its ego harm {excess_e:.3e}")
    assert excess_o <= 1e-12 and excess_e <= 1e-12
    assert (got[:, 0] - golden["rand_obst_harm"]).max() > 1e-3          # ... and the bound is a bound, not the value: most pairs lie below


@needs_cxx
def test_types_without_a_protection_entry_have_no_row(ask):
    coeff = " ".join(repr(v) for v in RI.COEFF.values())
    got = ask([f"R {t} 4.0 1000.0 {coeff}" for t in (11, 12, -1, 10, 8)])
    assert [g[0] for g in got] == ["0", "0", "0", "1", "1"]
    with pytest.raises(KeyError):
        RI.row("building", 1.0, 1.0, 1000.0)


# ------------------------------------------------------------------------------------------------ the choice and the fold
ROWS = {"clean": ([0.5 + i for i in range(16)], 1), "unsafe": ([0.25 * i for i in range(16)], 0),
        "poisoned": ([float("nan")] * 12 + [0.0, float("nan"), 0.0, 0.0], 0)}
ROWS["clean"][0][RI.C_SAFE] = 1.0
ROWS["unsafe"][0][RI.C_SAFE] = 0.0
SPEEDS = (0.0, 1.5, 6.0)
ATS = (-1, 0, 3)
# three different users, and three with users 0 and 1 alike: equal speeds then give bit-identical harms, the lowest class keeps them
MIXES = {"different": (IC.KINDS5[0], IC.KINDS5[1], IC.KINDS5[4]), "alike": (IC.KINDS5[1], IC.KINDS5[1], IC.KINDS5[4])}
SPEED_OF = {"different": (2.0, 7.0, 13.9), "alike": (7.0, 7.0, 13.9)}


@needs_cxx
def test_choice_and_fold_exhaustively_against_the_checker(ask):
    """every C <= 3, every at pattern over {-1, 0, 3}, speeds over {0, 1.5, 6} (equal ones among them), finite or not, over a clean, an
    unsafe and a poisoned cost row, harm_limit in {0, a value between two harms, 1, inf}: the header is the checker; and what the
    definition promises of any such row"""
    cases, lines = [], []
    for mix in MIXES:
        rows = IC.rows_of(MIXES[mix])
        harms = sorted({RI.logistic(rows[c][0], rows[c][1], s + SPEED_OF[mix][c]) for c in range(3) for s in SPEEDS})
        between = 0.5 * (harms[len(harms) // 2 - 1] + harms[len(harms) // 2])
        assert harms[0] < between < harms[-1] and between not in harms
        for C_ in (1, 2, 3):
            for at, speed in itertools.product(itertools.product(ATS, repeat=C_), itertools.product(SPEEDS, repeat=C_)):
                for finite, row, limit in itertools.product((0, 1), ROWS, (0.0, between, 1.0, math.inf)):
                    cost, safe = ROWS[row]
                    cases.append((mix, C_, at, speed, finite, row, limit))
                    pad = lambda vals, fill: list(vals) + [fill] * (4 - C_)     # (classes beyond C are not looked at: at 0, speed 99 would win)
                    flat = rows[:C_].ravel().tolist() + [0.0] * (16 - 4 * C_)
                    lines.append(f"V {C_} {finite} {safe} {limit!r} " + " ".join(repr(float(v)) for v in pad(speed, 99.0)) + " "
                                 + " ".join(str(v) for v in pad(at, 0)) + " " + " ".join(repr(v) for v in pad(SPEED_OF[mix][:C_], 0.0)) + " "
                                 + " ".join(repr(v) for v in flat) + " " + " ".join(repr(v) for v in cost))
    assert len(cases) == 2 * (9 + 81 + 729) * 24
    seen, n_open = set(), 0
    mix_rows = {mix: IC.rows_of(MIXES[mix]) for mix in MIXES}
    for case, got in zip(cases, ask(lines)):
        mix, C_, at, speed, finite, row, limit = case
        rows = mix_rows[mix][:C_]
        cost, safe = ROWS[row]
        ho, he, user, is_open = RI.choose(list(speed), list(at), rows, SPEED_OF[mix][:C_], bool(finite))
        want_row, want_safe = RI.fold_row(cost, safe, ho, user, limit)
        g_ho, g_he, g_user, g_safe = _num(got[0]), _num(got[1]), int(got[2]), int(got[3])
        g_row = [_num(v) for v in got[4:]]
        n_open += is_open
        assert abs(g_ho - ho) <= TOL and abs(g_he - he) <= TOL and g_user == user and g_safe == want_safe, case
        for col, (a, b) in enumerate(zip(g_row, want_row)):
            assert (math.isnan(a) and math.isnan(b)) or (abs(a - b) <= TOL if col == RI.C_RES0 else a == b), (case, col)
        # the definition's own promises, not via the checker
        hit = [c for c in range(C_) if at[c] >= 0]
        if not finite:
            assert (g_ho, g_he, g_user, g_safe) == (1.0, 1.0, -2, 0), case                # fails closed, whatever the limit
        elif not hit:
            assert (g_ho, g_he, g_user) == (0.0, 0.0, -1), case
        else:
            per = [RI.logistic(rows[c][0], rows[c][1], speed[c] + SPEED_OF[mix][c]) for c in hit]
            assert g_user == hit[per.index(max(per))] and abs(g_ho - max(per)) <= TOL, case    # the lowest class among the greatest
            assert 0.0 < g_ho < 1.0 and 0.0 < g_he < 1.0, case
        assert g_safe <= safe and g_safe == (0 if (g_ho > limit or not finite) else safe), case     # safety is only ever taken away
        for col in range(16):
            if col not in (RI.C_SAFE, RI.C_RES0, RI.C_RES1):
                assert (math.isnan(cost[col]) and math.isnan(g_row[col])) or cost[col] == g_row[col], case   # NaN rows keep their NaNs
        assert g_row[RI.C_RES0] == g_ho and g_row[RI.C_RES1] == float(g_user), case
        seen.add((g_user, g_safe, row, limit if limit in (0.0, 1.0, math.inf) else "between"))
    assert n_open == 0
    assert {(-2, 0, "clean", math.inf), (-1, 1, "clean", 0.0), (0, 0, "clean", 0.0), (2, 1, "clean", 1.0), (-1, 0, "poisoned", math.inf),
            (0, 1, "clean", "between")} <= seen
    assert any(u >= 0 and s == 0 and row == "clean" and lim == "between" for u, s, row, lim in seen)     # the limit cuts between two harms


def test_speed_and_start_of_the_checker():
    """steps 1 - 3 on rows written out by hand: v = 8 7 6 5, a_brake = 2, dt = 0.5"""
    v = [8.0, 7.0, 6.0, 5.0]
    one = lambda first, bf, st, ends=4: RI.speed_one(first, bf, st, v, 2.0, 0.5, ends)
    assert one(-1, [-1, -1, -1, -1], [4, 4, 4, 4]) == (0.0, -1)                          # no hit start
    assert one(-1, [2, 2, 3, -1], [4, 4, 4, 4]) == (6.0, 0)                              # 8 - 2 * (2 * 0.5) = 6 from b = 0; 7 - 1 = 6 from b = 1: the lower start
    assert one(-1, [3, 2, -1, -1], [4, 4, 4, 4]) == (6.0, 1)                             # 8 - 3 = 5 from b = 0, 7 - 1 = 6 from b = 1
    assert one(-1, [2, -1, -1, -1], [2, 4, 4, 4]) == (0.0, -1)                           # hit at the stop sample: a standing ego carries no harm
    assert one(2, [-1, -1, -1, -1], [4, 4, 4, 4]) == (6.0, 2)                            # the candidate itself is met at sample 2: v[2] from b = 2 on
    assert one(2, [1, -1, -1, -1], [4, 4, 4, 4]) == (7.0, 0)                             # ... and a faster manoeuvre hit before it
    assert one(2, [-1, -1, -1, -1], [4, 4, 4, 4], ends=2) == (0.0, -1)                   # brake starts beyond B are not looked at
    assert RI.speed_one(0, [-1], [1], [float("nan")], 2.0, 0.5, 1) == (0.0, -1)          # a NaN never wins


def test_no_open_choice_in_any_scene_of_the_device_tests():
    """the condition tests/test_hidden_impact_gpu.py compares ``user`` exactly under: in no scene of its raw-entry tests -- the six tie
    scenes at every B, the class-and-map-count scene, the hand cases -- do the checker's best and second-best obstacle harm come
    closer than 1e-9 without being the same number from the same (row, w).  (The step tests' scenes are made on the device: the device
    test holds them to the same condition on what it reads back.)"""
    import hidden_brake_users_scenes as US
    import ref_hidden_brake_users as BU
    import test_hidden_brake_users_gpu as UG
    import test_hidden_brake_verdict_gpu as VG
    SC = IC.SC
    road = SC.road_raster()
    hits = 0
    for T_, spec in VG.TIE_SCENES.items():
        users = UG.THREE if T_ == 254 else US.USERS
        sc = VG._scene(spec, users)
        kinds = IC.kinds_of(users, IC.KINDS5, US.USERS)
        bf, stop, _, first = BU.brake_users(sc.keys, sc.win, road, sc.qmins, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW,
                                            SC.WB, sc.a_brake, sc.dt, sc.thr, sc.map_of, sc.lens)
        for B in VG._starts(T_):
            harm, user, speed, at, n_open = RI.impact(bf, stop, first, sc.v, sc.a_brake, sc.dt, B, IC.rows_of(kinds), [u[0] for u in users], sc.lens)
            assert n_open == 0, (T_, B)
            hits += int((user >= 0).sum())
    sc, keys, qmins, cap = UG._three_maps()
    for C_, K in itertools.product((1, 4, 5, 8), (1, 2, 3)):
        map_of = [(c + 1) % K for c in range(C_)]
        bf, stop, _, first = BU.brake_users(keys[:K], sc.win, road, qmins[:K], SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW,
                                            SC.WB, sc.a_brake, sc.dt, sc.thr[:C_], map_of, sc.lens)
        for B in (1, 5, 31):
            assert RI.impact(bf, stop, first, sc.v, sc.a_brake, sc.dt, B, IC.rows_of(IC.KINDS8[:C_]), UG.SPEEDS8[:C_], sc.lens)[4] == 0, (C_, K, B)
    assert hits > 20


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_entries_and_keeps_the_abi():
    from frenetix_occlusion import _native as N
    import ctypes as C
    lib = N.load()
    for name in ("fo_scene_hidden_brake_impact", "fo_hidden_impact_row"):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.fo_abi_version() == 12
    # the verdict's structure without commit_min, and: speed_of, rows, harm_limit; harm, user, speed, at, commit, first for its four outputs
    assert C.sizeof(N.HiddenBrakeImpact) == C.sizeof(N.HiddenBrakeVerdict) + 3 * 8 + 2 * 8
    hc = N.HarmCoeff(**RI.COEFF)
    row = (C.c_double * 4)()
    for kind, length, width in IC.KINDS8:
        assert lib.fo_hidden_impact_row(N.TYPE_CODES[kind.lower()], length * width, IC.EGO_MASS, C.byref(hc), row) == N.FO_OK
        assert np.abs(np.array(row[:]) - np.array(RI.row(kind, length, width, IC.EGO_MASS))).max() <= 1e-15
    assert lib.fo_hidden_impact_row(11, 4.0, IC.EGO_MASS, C.byref(hc), row) == N.FO_E_ARG          # FO_TYPE_STRUCTURE: no protection entry
    assert lib.fo_hidden_impact_row(0, -1.0, IC.EGO_MASS, C.byref(hc), row) == N.FO_E_ARG
    assert lib.fo_hidden_impact_row(0, 4.0, float("nan"), C.byref(hc), row) == N.FO_E_ARG


def test_python_rows_and_stage_options():
    from frenetix_occlusion.hidden_traffic import hidden_impact_rows
    from frenetix_occlusion.step import PlanningStep, hidden_stage_options
    rows = hidden_impact_rows(IC.KINDS5, IC.EGO_MASS)
    assert np.abs(rows - IC.rows_of(IC.KINDS5)).max() <= 1e-15
    for bad in ((("Building", 1.0, 1.0),), (("Car", -1.0, 2.0),), (("Car", 1.0),), ("Car",)):
        with pytest.raises(ValueError, match="hidden_impact_rows"):
            hidden_impact_rows(bad, IC.EGO_MASS)
    with pytest.raises(ValueError, match="ego_mass"):
        hidden_impact_rows(IC.KINDS5, 0.0)
    from types import SimpleNamespace
    stage = SimpleNamespace(ctx=object())
    iv = dict(vehicle=(4.5, 1.8, 1.4), ego_mass=1200.0, users=((2.0, "road", "any"),), kinds=(("Pedestrian", 0.4, 0.6),), dt=0.1, a_brake=8.0,
              starts=5, harm_limit=0.1)
    hv = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, a_brake=8.0, starts=5, commit_min=5)
    lv = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, levels=[1.0, 2.0], starts=5, a_limit=8.0)
    step = lambda **kw: PlanningStep(stage, stage, stage, None, None, None, None, **kw)
    for two in (dict(hidden_verdict=hv, hidden_impact_verdict=iv), dict(hidden_ladder_verdict=lv, hidden_impact_verdict=iv),
                dict(hidden_verdict=hv, hidden_ladder_verdict=lv), dict(hidden_verdict=hv, hidden_ladder_verdict=lv, hidden_impact_verdict=iv)):
        with pytest.raises(ValueError, match="same two reserved cost columns"):       # raised before anything is allocated
            step(**two)
    for bad in (dict(users=iv["users"]), {k: v for k, v in iv.items() if k != "harm_limit"}, dict(iv, commit_min=1), 5, "kinds"):
        with pytest.raises(ValueError, match="hidden_impact_verdict"):
            step(hidden_impact_verdict=bad)
    assert hidden_stage_options(None, None, None) == (None, None) and hidden_stage_options(hv, None, None) == (None, None)
    got = hidden_stage_options(None, None, dict(iv, coeff=dict(RI.COEFF), lengths=[1]))[1]
    assert got == dict(iv, coeff=dict(RI.COEFF), lengths=[1]) and got is not iv
