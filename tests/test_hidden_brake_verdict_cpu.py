"""The host side of the hidden-traffic fail-safe verdict (DESIGN.md §5.10 "Fail-safe verdict"), without a GPU: the fold
(csrc/fo_hidden_verdict.hpp) and the launch plan (csrc/fo_scene_plan.hpp) built with the host C++ compiler, as
tests/test_rule_refusal_cpu.py builds csrc/fo_verdict.hpp, against the plain statement tests/ref_hidden_brake_verdict.py; a hand case
by the checkers alone; the library's symbols."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_hidden_brake_verdict as BV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include <cstdio>
#include "fo_scene_plan.hpp"
#include "fo_hidden_verdict.hpp"
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'C') {          // C -> FO_C_SAFE FO_C_RES0 FO_C_RES1 FO_NC NOT_FINITE rows bound
      printf("%d %d %d %d %d %d %zu\n", FO_C_SAFE, FO_C_RES0, FO_C_RES1, FO_NC, FO_HIDDEN_VERDICT_NOT_FINITE, BRAKE_LADDER_ROWS_BYTES,
             brake_verdict_lds_bound());
    } else if (what == 'V') {   // V C B commit_min finite safe, four commits of the users entry, sixteen costs -> fail_safe user safe + the sixteen
      int C, B, cmin, finite, safe_in;
      int32_t commit[4];
      double cost[FO_NC];
      if (scanf("%d %d %d %d %d %d %d %d %d", &C, &B, &cmin, &finite, &safe_in, commit, commit + 1, commit + 2, commit + 3) != 9) return 1;
      for (int i = 0; i < FO_NC; ++i) if (scanf("%lf", cost + i) != 1) return 1;
      for (int c = 0; c < 4; ++c) commit[c] = fo_hidden_verdict_commit(commit[c], B);
      const fo_hidden_verdict_t r = fo_hidden_verdict_classes<4>(commit, C, B, finite != 0);
      uint8_t safe = (uint8_t)safe_in;
      fo_hidden_verdict_fold(r, cmin, cost, &safe);
      printf("%d %d %d", r.fail_safe, r.user, (int)safe);
      for (int i = 0; i < FO_NC; ++i) printf(" %.17g", cost[i]);
      printf("\n");
    } else if (what == 'P') {   // P T K B C M -> group per_block blocks lds
      int T, K, B, C, M;
      if (scanf("%d %d %d %d %d", &T, &K, &B, &C, &M) != 5) return 1;
      printf("%d %d %d %zu\n", brake_verdict_group(B), brake_verdict_per_block(T, K, B), brake_verdict_blocks(M, T, K, B),
             brake_verdict_lds_bytes(T, K, C, B));
    } else {
      return 1;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("hidden_verdict")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(d / "driver.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [ln.split() for ln in out[:-1]]
    return run


# ------------------------------------------------------------------------------------------------ the fold
ROWS = {"clean": ([0.5 + i for i in range(16)], 1), "unsafe": ([0.25 * i for i in range(16)], 0),
        "poisoned": ([float("nan")] * 12 + [0.0, float("nan"), 0.0, 0.0], 0)}
ROWS["clean"][0][BV.C_SAFE] = 1.0
ROWS["unsafe"][0][BV.C_SAFE] = 0.0


@needs_cxx
def test_the_header_names_the_columns_the_checker_names(ask):
    from frenetix_occlusion import _native as N
    got = [int(v) for v in ask(["C"])[0]]
    assert got[:5] == [BV.C_SAFE, BV.C_RES0, BV.C_RES1, BV.NC, BV.NOT_FINITE] == [N.COST["safe"], 14, 15, N.NC, N.HIDDEN_VERDICT_NOT_FINITE]


@needs_cxx
def test_fold_exhaustively_against_the_checker(ask):
    """every C <= 3, B <= 4, commit vector in {-1 .. B-1}^C, commit_min in [0, B], finite in {0, 1}, over a clean, an unsafe and a
    poisoned cost row: the header is the checker; and what the definition promises of any such row"""
    cases, lines = [], []
    for C_, B in itertools.product((1, 2, 3), (1, 2, 3, 4)):
        for commit in itertools.product(range(-1, B), repeat=C_):
            for cmin, finite, row in itertools.product(range(B + 1), (0, 1), ROWS):
                cost, safe = ROWS[row]
                cases.append((C_, B, commit, cmin, finite, row))
                padded = list(commit) + [0] * (4 - C_)       # (classes beyond C are not looked at: a 0 there would win every minimum)
                lines.append(f"V {C_} {B} {cmin} {finite} {safe} " + " ".join(str(c) for c in padded) + " " + " ".join(repr(v) for v in cost))
    assert len(cases) == 7536
    seen = set()
    for (C_, B, commit, cmin, finite, row), got in zip(cases, ask(lines)):
        cost, safe = ROWS[row]
        _, fs, user = BV.fold_one(commit, B, bool(finite))
        want_row, want_safe = BV.fold_row(cost, safe, fs, user, cmin)
        g_fs, g_user, g_safe = (int(v) for v in got[:3])
        g_row = [float(v) for v in got[3:]]
        at = (C_, B, commit, cmin, finite, row)
        assert (g_fs, g_user, g_safe) == (fs, user, want_safe), at
        assert all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(g_row, want_row)), at
        # the definition's own promises, not via the checker
        if finite:
            live = [c for c in commit if c >= 0]
            assert g_fs == (min(live) if live else B) and g_user == (commit.index(min(live)) if live else -1), at   # the lowest index
        else:
            assert (g_fs, g_user) == (0, -2), at                                        # fails closed
        assert g_safe <= safe and (g_safe == safe or g_fs < cmin), at                   # safety is only ever taken away
        assert g_safe == (0 if g_fs < cmin else safe), at
        for col in range(16):
            if col not in (BV.C_SAFE, BV.C_RES0, BV.C_RES1):
                assert (math.isnan(cost[col]) and math.isnan(g_row[col])) or cost[col] == g_row[col], at   # NaN rows keep their NaNs
        assert g_row[BV.C_RES0] == float(g_fs) and g_row[BV.C_RES1] == float(g_user), at
        seen.add((g_user, g_safe, row))
    assert {(-2, 0, "clean"), (-1, 1, "clean"), (0, 0, "clean"), (2, 1, "clean"), (-1, 0, "poisoned")} <= seen


@needs_cxx
def test_commits_at_or_beyond_the_walked_starts_do_not_count(ask):
    """step 1: the users entry's commit seen through B brake starts"""
    row = " ".join(repr(v) for v in ROWS["clean"][0])
    got = ask([f"V 3 2 2 1 1 5 2 -1 0 {row}", f"V 3 2 2 1 1 5 1 1 0 {row}", f"V 2 3 1 1 1 -7 300 0 0 {row}"])
    assert [tuple(int(v) for v in g[:3]) for g in got] == [(2, -1, 1), (1, 1, 0), (3, -1, 1)]
    assert BV.fold_one([5, 2, -1], 2) == ([-1, -1, -1], 2, -1) and BV.fold_one([5, 1, 1], 2) == ([-1, 1, 1], 1, 1)


# ------------------------------------------------------------------------------------------------ the plan
@needs_cxx
def test_plan_over_every_shape(ask):
    """every (T, K, B), T in [1, 254], K in {1, 2, 3}, B in [1, T]: the lanes cover every (m, b), LDS within the bound, per_block >= 1"""
    rows_bytes, bound = (int(v) for v in ask(["C"])[0][5:7])
    assert rows_bytes == 32768 and bound == 32768 + 4 * 896 <= 65536
    shapes = [(T, K, B) for T in range(1, 255) for K in (1, 2, 3) for B in range(1, T + 1)]
    lines = []
    for T, K, B in shapes:
        C_ = min(8, 896 // T)
        lines.append(f"P {T} {K} {B} {C_} {1000 + T}")
    groups = set()
    for (T, K, B), got in zip(shapes, ask(lines)):
        G, per, blocks, lds = (int(v) for v in got)
        C_, M = min(8, 896 // T), 1000 + T
        assert G == min(64, 1 << (B - 1).bit_length()) and G & (G - 1) == 0, (T, K, B)      # the power of two >= min(B, 64)
        per_traj = T * (48 + 4 * K)
        assert per == max(1, min(256 // G, rows_bytes // per_traj)), (T, K, B)
        assert per >= 1 and per * G <= 256, (T, K, B)               # every trajectory of the workgroup has its G lanes ...
        assert G >= min(B, 64) and -(-B // G) * G >= B, (T, K, B)   # ... which reach every b < B in ceil(B / G) rounds
        assert blocks == -(-M // per) and blocks * per >= M, (T, K, B)
        assert lds == per * per_traj + 4 * C_ * T <= bound, (T, K, B)
        assert per == 1 or per * per_traj <= rows_bytes, (T, K, B)
        groups.add(G)
    assert groups == {1, 2, 4, 8, 16, 32, 64}
    # the issue's example: 64 trajectories of T = 31, K = 3 would be 119 KB; the plan keeps 17
    assert 64 * 31 * 60 == 119040 and [int(v) for v in ask(["P 31 3 4 3 100"])[0]][:2] == [4, 17]


# ------------------------------------------------------------------------------------------------ a hand case by the checkers
def hand_case():
    """a creeping and a fast candidate towards a stretch of road nobody sees, on the straight road of tests/hidden_brake_scenes.py:
    the hidden stretch starts 20 m ahead, a hidden road user of 4 m/s along the road.  It stands in for the occluded junction of the
    issue: the small raster the checkers share is a straight road, and what the case has to show -- hidden traffic that comes towards
    the ego out of road it cannot see, reached by the fast candidate's braking manoeuvres and by none of the creeping one's -- does not
    need the crossing.  Returns what both test files need"""
    from types import SimpleNamespace
    import hidden_brake_classes_scenes as CS
    import hidden_brake_scenes as SC
    import ref_hidden_clearance as HC
    T, B = 31, 5
    win = SC.WINDOWS[0]
    road = SC.road_raster()
    cls = SC.class_bytes(np.random.default_rng(0), win, road, 0, specks=False)
    ix0, iy0, nx, ny = win
    c0 = int(round((20.0 - SC.ORIGIN[0]) / SC.CS)) - ix0
    sub = cls[:, c0:c0 + 8]
    sub[:] = np.where(sub & 1, 5, 4)                               # occluded across the whole road, 4 m deep
    v0 = np.array([1.0, 14.0])
    k = np.arange(T) * SC.DT
    x = v0[:, None] * k[None, :]
    y = np.full((2, T), -1.75)
    theta = np.zeros((2, T))
    v = np.repeat(v0[:, None], T, axis=1)
    head = np.stack((np.cos(theta), np.sin(theta)), -1)
    users = ((4.0, "road", "any"),)
    tables = CS.reach_tables((4.0,), T)
    thr = CS.thresholds(tables)
    r2_cap = int(tables[0][-1])
    sc = SimpleNamespace(cls=cls, win=win, road=road, hidden=None, entry=SC.ENTRIES[1], moves=SC.lane_table())
    key = np.asarray(CS.key_map(sc, r2_cap))
    qmin = np.asarray(HC.clearance(key, win, road, SC.ORIGIN, SC.CS, x, y, head, SC.HL, SC.HW, SC.WB, None))
    return SimpleNamespace(T=T, B=B, win=win, road=road, cls=cls, x=x, y=y, theta=theta, v=v, head=head, arc=SC.travelled_arc(x, y),
                           users=users, thr=thr, r2_cap=r2_cap, key=key, qmin=qmin, a_brake=8.0, dt=SC.DT)


def test_hand_case_creeping_and_fast():
    """the checker: the creeping candidate is fail-safe throughout the B starts, the fast one not even now -- though neither meets a
    reachable cell while it FOLLOWS its samples for those starts' sake alone (first is late or none): the verdict is about braking"""
    import hidden_brake_scenes as SC
    h = hand_case()
    fail_safe, user, commit, first = BV.brake_verdict([h.key], h.win, h.road, [h.qmin], SC.ORIGIN, SC.CS, h.x, h.y, h.head, h.arc, h.v,
                                                      SC.HL, SC.HW, SC.WB, h.a_brake, h.dt, h.thr, [0], h.B)
    assert fail_safe.tolist() == [h.B, 0] and user.tolist() == [-1, 0]
    assert commit.tolist() == [[-1, 0]] and first[0, 0] == -1 and first[0, 1] > 0
    cost = np.zeros((2, 16))
    cost[:, BV.C_SAFE] = 1.0
    cost2, safe2 = BV.fold(cost, np.ones(2, dtype=np.uint8), fail_safe, user, h.B)
    assert safe2.tolist() == [1, 0] and cost2[:, BV.C_SAFE].tolist() == [1.0, 0.0]
    assert cost2[:, BV.C_RES0].tolist() == [float(h.B), 0.0] and cost2[:, BV.C_RES1].tolist() == [-1.0, 0.0]


def test_finite_flags_of_the_checker():
    x = np.zeros((3, 4))
    bad = x.copy()
    bad[1, 2] = np.inf
    assert BV.finite_flags(x, x, x, bad).tolist() == [1, 0, 1]
    assert BV.finite_flags(x, x, x, bad, [4, 2, 4]).tolist() == [1, 1, 1] and BV.finite_flags(bad, x, x, x, [4, 3, 4]).tolist() == [1, 0, 1]


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_entries_and_keeps_the_abi():
    from frenetix_occlusion import _native as N
    lib = N.load()
    for name in ("fo_scene_hidden_poses", "fo_scene_hidden_brake_verdict"):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.fo_abi_version() == 12
    import ctypes as C
    assert C.sizeof(N.HiddenBrakeVerdict) == C.sizeof(N.HiddenBrakeUsers) + 8 + 3 * 8    # B, commit_min; finite, cost, safe; outputs 4 for 4
    assert C.sizeof(N.HiddenPoses) == 8 + 8 * 8
