"""The host side of the hidden-traffic ladder verdict (DESIGN.md §5.10 "Ladder verdict"), without a GPU: the fold
(csrc/fo_hidden_ladder_verdict.hpp) and the launch plan (csrc/fo_scene_plan.hpp brake_ladder_verdict_*) built with the host C++
compiler, as tests/test_hidden_brake_verdict_cpu.py builds csrc/fo_hidden_verdict.hpp, against the plain statement
tests/ref_hidden_brake_ladder_verdict.py; the validation of PlanningStep(hidden_ladder_verdict=); the library's symbols."""
import itertools
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import ref_hidden_brake_ladder_verdict as LV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

# the driver walks the brake starts of ONE trajectory as a lane of the kernel does over its rounds: a key and the per-class ranks per
# start with a manoeuvre, their maxima, then lane 0's verdict and fold
DRIVER = r"""
#include <cstdio>
#include "fo_scene_plan.hpp"
#include "fo_hidden_ladder_verdict.hpp"
static double rows[8][FO_NC];
static const int BS[6] = {1, 2, 3, 5, 8, 31};
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'C') {          // C -> FO_C_SAFE FO_C_RES0 FO_C_RES1 FO_NC NOT_FINITE rows bound
      printf("%d %d %d %d %d %d %zu\n", FO_C_SAFE, FO_C_RES0, FO_C_RES1, FO_NC, FO_HIDDEN_VERDICT_NOT_FINITE, BRAKE_LADDER_ROWS_BYTES,
             brake_ladder_verdict_lds_bound());
    } else if (what == 'R') {   // R i, sixteen costs: row i for later V lines
      int i;
      if (scanf("%d", &i) != 1 || i < 0 || i >= 8) return 1;
      for (int c = 0; c < FO_NC; ++c) if (scanf("%lf", rows[i] + c) != 1) return 1;
      printf("ok\n");
    } else if (what == 'V') {   // V C L B ends finite safe row a_limit, three levels, ra[3], blk[3], req[3][3] -> need at blocking user decel need_of[3] safe + the sixteen
      int C, L, B, ends, finite, safe_in, row;
      double a_limit, levels[3];
      int ra[3], blk[3], req[3][3];
      if (scanf("%d %d %d %d %d %d %d %lf %lf %lf %lf", &C, &L, &B, &ends, &finite, &safe_in, &row, &a_limit, levels, levels + 1, levels + 2) != 11) return 1;
      for (int b = 0; b < 3; ++b) if (scanf("%d", ra + b) != 1) return 1;
      for (int b = 0; b < 3; ++b) if (scanf("%d", blk + b) != 1) return 1;
      for (int c = 0; c < 3; ++c) for (int b = 0; b < 3; ++b) if (scanf("%d", &req[c][b]) != 1) return 1;
      int32_t key = FO_HIDDEN_LADDER_NO_KEY, need_of[3] = {-1, -1, -1};
      for (int b = 0; b < B; ++b)
        if (b < ends) {
          for (int c = 0; c < C; ++c) need_of[c] = fo_hidden_ladder_max(need_of[c], fo_hidden_ladder_rank(req[c][b], L));
          key = fo_hidden_ladder_max(key, fo_hidden_ladder_key(fo_hidden_ladder_rank(ra[b], L), b, blk[b]));
        }
      fo_hidden_ladder_verdict_t r = fo_hidden_ladder_verdict_of(key, L, finite != 0);
      const int nl = r.need >= 0 && r.need < L ? r.need : 0;
      r.decel = fo_hidden_ladder_decel(r.need, L, levels[nl]);
      printf("%d %d %d %d %.17g %d %d %d", r.need, r.at, r.blocking, r.user, r.decel, need_of[0], need_of[1], need_of[2]);
      if (row >= 0) {           // (row < 0: steps 1 - 6 alone)
        double cost[FO_NC];
        for (int i = 0; i < FO_NC; ++i) cost[i] = rows[row][i];
        uint8_t safe = (uint8_t)safe_in;
        fo_hidden_ladder_verdict_fold(r, L, a_limit, cost, &safe);
        printf(" %d", (int)safe);
        for (int i = 0; i < FO_NC; ++i) printf(" %.17g", cost[i]);
      }
      printf("\n");
    } else if (what == 'K') {   // K rank b blocking -> the key
      int rank, b, blocking;
      if (scanf("%d %d %d", &rank, &b, &blocking) != 3) return 1;
      printf("%d\n", fo_hidden_ladder_key(rank, b, blocking));
    } else if (what == 'P') {   // P T K M -> for L = 1 .. 64, B in {1, 2, 3, 5, 8, 31, T} (those <= T; else zeros), at the most classes C <= 8 that
                                // T and L admit (C T <= 896, 4 C T + 8 L <= 3584): C width group per_block blocks lds
      int T, K, M;
      if (scanf("%d %d %d", &T, &K, &M) != 3) return 1;
      for (int L = 1; L <= 64; ++L) {
        int C = 8;
        while (C > 1 && (C * T > BRAKE_USERS_MAX_TABLE || 4 * C * T + 8 * L > BRAKE_LADDER_USERS_MAX_ARG_BYTES)) --C;
        for (int i = 0; i < 7; ++i) {
          const int B = i < 6 ? BS[i] : T;
          if (B > T) { printf("0 0 0 0 0 0 "); continue; }
          printf("%d %d %d %d %d %zu ", C, brake_ladder_users_width(L), brake_ladder_verdict_group(L, B), brake_ladder_verdict_per_block(T, K, L, B),
                 brake_ladder_verdict_blocks(M, T, K, L, B), brake_ladder_verdict_lds_bytes(T, K, C, L, B));
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
    d = tmp_path_factory.mktemp("hidden_ladder_verdict")
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
ROWS["clean"][0][LV.C_SAFE] = 1.0
ROWS["unsafe"][0][LV.C_SAFE] = 0.0
LEVELS = (0.5, 2.0, 6.5)


def _limits(L):
    """0, just below, at and just above each level, and +inf"""
    out = [0.0, math.inf]
    for a in LEVELS[:L]:
        out += [np.nextafter(a, -np.inf), a, np.nextafter(a, np.inf)]
    return [float(a) for a in out]


@needs_cxx
def test_the_header_names_the_columns_the_checker_names(ask):
    from frenetix_occlusion import _native as N
    got = [int(v) for v in ask(["C"])[0]]
    assert got[:5] == [LV.C_SAFE, LV.C_RES0, LV.C_RES1, LV.NC, LV.NOT_FINITE] == [N.COST["safe"], 14, 15, N.NC, N.HIDDEN_VERDICT_NOT_FINITE]


@needs_cxx
def test_the_key_orders_rank_then_the_earlier_start(ask):
    """the header's key is monotone in (rank, -b) whatever the masks: a larger rank wins against any start and mask, at equal rank the
    earlier start wins against any mask -- over the corners rank 0 / 64, b = 0 / 253, masks 0 / 255"""
    ranks, starts = (0, 1, 63, 64), (0, 1, 252, 253)
    cases = [(r, b, k) for r in ranks for b in starts for k in (0, 255)]
    key = {c: int(g[0]) for c, g in zip(cases, ask([f"K {r} {b} {k}" for r, b, k in cases]))}
    assert all(0 <= v < 2 ** 31 for v in key.values()) and min(key.values()) > -1      # every key beats "no key" (-1)
    for r in ranks:
        for b0, b1 in zip(starts, starts[1:]):
            assert key[r, b0, 0] > key[r, b1, 255], (r, b0, b1)
    for r0, r1 in zip(ranks, ranks[1:]):
        assert key[r1, 253, 0] > key[r0, 0, 255], (r0, r1)


def _v_line(C_, L, B, ends, finite, safe, row, a_limit, ra, blk, req):
    pad = lambda v, fill=0: list(v) + [fill] * (3 - len(v))
    flat = [x for r in pad([pad(r) for r in req], [0, 0, 0]) for x in r]
    return (f"V {C_} {L} {B} {ends} {finite} {safe} {row} {a_limit!r} " + " ".join(repr(a) for a in LEVELS) + " "
            + " ".join(str(v) for v in pad(ra) + pad(blk) + flat))


@needs_cxx
def test_steps_1_to_6_exhaustively_against_the_checker(ask):
    """C <= 3, B <= 3, L <= 3: every required_all vector in {-1 .. L-1}^B x every vector of blocking masks (3 bits a start: the masks of
    C < 3 are among them, the key does not know C) x every ends <= B; not finite x every vector x every ends; every required vector of
    every class in every class position x every ends (the classes share no state: while one runs through every vector the others
    rotate).  need, at, blocking, user, decel and need_of are the checker's"""
    cases = []
    n = 0
    for L, B in itertools.product((1, 2, 3), (1, 2, 3)):
        vecs = list(itertools.product(range(-1, L), repeat=B))
        for ra in vecs:
            for ends in range(B + 1):
                for blk in itertools.product(range(8), repeat=B):
                    n += 1
                    cases.append((3, L, B, ends, 1, ra, blk, [vecs[(n + 7 * c) % len(vecs)] for c in range(3)]))
                cases.append((3, L, B, ends, 0, ra, (7,) * B, [vecs[(n + 7 * c) % len(vecs)] for c in range(3)]))
        for C_ in (1, 2, 3):
            for c, rq in itertools.product(range(C_), vecs):
                for ends in range(B + 1):
                    n += 1
                    cases.append((C_, L, B, ends, 1, vecs[n % len(vecs)], (0,) * B, [rq if k == c else vecs[(n + 5 * k) % len(vecs)] for k in range(C_)]))
    got_all = ask([_v_line(C_, L, B, ends, finite, 1, -1, math.inf, ra, blk, req) for C_, L, B, ends, finite, ra, blk, req in cases])
    kinds = set()
    for (C_, L, B, ends, finite, ra, blk, req), got in zip(cases, got_all):
        need, at, blocking, user, decel, need_of = LV.fold_one(ra, blk, req, ends, LEVELS[:L], bool(finite))
        want = [str(need), str(at), str(blocking), str(user), repr(decel).replace("inf", "inf")] + [str(v) for v in need_of] + ["-1"] * (3 - C_)
        if got[:4] != want[:4] or float(got[4]) != decel or got[5:8] != want[5:8]:
            raise AssertionError(((C_, L, B, ends, finite, ra, blk, req), got, want))
        kinds.add((need - L if need >= L else min(need, 0), user))
    assert {(0, -2), (-1, -1), (0, -1), (0, 0), (0, 1), (0, 2)} <= kinds and len(cases) > 200000


@needs_cxx
def test_fold_exhaustively_against_the_checker(ask):
    """step 7 with the steps before it, L <= 3: every need in {-1 .. L}, finite or not, every blocking mask of three users, a_limit at 0,
    just below, at and just above each level and +inf, over a clean, an unsafe and a poisoned cost row.  The header is the checker;
    and what the definition promises of any such row"""
    order = list(ROWS)
    lines = [f"R {i} " + " ".join(repr(v) for v in ROWS[name][0]) for i, name in enumerate(order)]
    cases = []
    for L in (1, 2, 3):
        for need, finite, mask, a_limit, row in itertools.product(range(-1, L + 1), (0, 1), range(8), _limits(L), order):
            ra, ends = ([need if need < L else -1, 0], 1) if need >= 0 else ([0, 0], 0)
            cases.append((3, L, 2, ends, finite, row, a_limit, ra, [mask, 7 - mask], [[0, 0], [-1, 0], [L - 1, 0]]))
    for C_, L, B, ends, finite, row, a_limit, ra, blk, req in cases:
        lines.append(_v_line(C_, L, B, ends, finite, ROWS[row][1], order.index(row), a_limit, ra, blk, req))
    got_all = ask(lines)[3:]
    seen = set()
    for (C_, L, B, ends, finite, row, a_limit, ra, blk, req), got in zip(cases, got_all):
        at_case = (C_, L, B, ends, finite, row, a_limit, ra, blk, req)
        cost, safe = ROWS[row]
        levels = LEVELS[:L]
        need, at, blocking, user, decel, need_of = LV.fold_one(ra, blk, req, ends, levels, bool(finite))
        want_row, want_safe = LV.fold_row(cost, safe, need, user, decel, L, a_limit)
        g = [int(v) for v in got[:4]] + [float(got[4])] + [int(v) for v in got[5:9]]
        g_row = [float(v) for v in got[9:]]
        assert g[:5] == [need, at, blocking, user, decel] and g[5:5 + C_] == need_of and g[8] == want_safe, at_case
        assert all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(g_row, want_row)), at_case
        # the definition's own promises, not via the checker
        g_need, g_at, g_blk, g_user, g_decel, g_safe = g[0], g[1], g[2], g[3], g[4], g[8]
        if not finite:
            assert (g_need, g_at, g_blk, g_user, g_decel) == (L, 0, 0, -2, math.inf), at_case                 # fails closed
        elif ends == 0:
            assert (g_need, g_at, g_blk, g_user, g_decel) == (-1, -1, 0, -1, 0.0), at_case                    # nothing asked
        else:
            assert g_need == (ra[0] if ra[0] >= 0 else L) and g_at == 0 and g_blk == blk[0], at_case
            assert g_user == ([c for c in range(3) if g_blk >> c & 1] or [-1])[0], at_case
            assert g_decel == (math.inf if g_need == L else levels[g_need]), at_case                          # bit-equal to levels[need]
        lost = g_need == L or g_decel > a_limit
        assert g_safe == (0 if lost else safe) and g_safe <= safe, at_case                                    # safety is only ever taken away
        if a_limit == math.inf:
            assert lost == (g_need == L), at_case
        for col in range(16):
            if col not in (LV.C_SAFE, LV.C_RES0, LV.C_RES1):
                assert (math.isnan(cost[col]) and math.isnan(g_row[col])) or cost[col] == g_row[col], at_case   # NaN rows keep their NaNs
        assert g_row[LV.C_RES0] == g_decel and g_row[LV.C_RES1] == float(g_user), at_case
        assert g_row[LV.C_SAFE] == (0.0 if lost else cost[LV.C_SAFE]), at_case
        seen.add((g_user, g_safe, row))
    assert {(-2, 0, "clean"), (-1, 1, "clean"), (0, 0, "clean"), (2, 1, "clean"), (-1, 0, "poisoned"), (1, 0, "poisoned")} <= seen


@needs_cxx
def test_the_key_of_the_header_is_the_documented_one(ask):
    cases = [(r, b, k) for r in (0, 1, 23, 64) for b in (0, 1, 30, 253) for k in (0, 1, 0x80, 0xff)]
    got = ask([f"K {r} {b} {k}" for r, b, k in cases])
    assert [int(g[0]) for g in got] == [r << 16 | (255 - b) << 8 | k for r, b, k in cases]


# ------------------------------------------------------------------------------------------------ the plan
def expected_plan(T, K, C, L, B, M):
    """(Lp, G, per_block, blocks, lds_bytes): the Python restatement of csrc/fo_scene_plan.hpp's brake_ladder_verdict_* functions"""
    Lp = 1 << (L - 1).bit_length()
    G = min(256, Lp * (1 << (B - 1).bit_length()))
    per_traj = T * (48 + 4 * K)
    per = max(1, min(256 // G, 32768 // per_traj))
    return Lp, G, per, -(-M // per), per * per_traj + 4 * C * T + 4 * (C + 1) * 4


def most_classes(T, L):
    """the largest C in [1, 8] that one call admits at this T and L: C T <= 896 thresholds and 4 C T + 8 L <= 3584 bytes of argument (C = 1
    always fits: 4 * 254 + 8 * 64 = 1528)"""
    return max(c for c in range(1, 9) if c == 1 or (c * T <= 896 and 4 * c * T + 8 * L <= 3584))


PLAN_STARTS = (1, 2, 3, 5, 8, 31)
# (T, K, L, B) over T in [1, 254], K in {1, 2, 3}, L in [1, 64], B in {1, 2, 3, 5, 8, 31} where B <= T, and B = T
PLAN_SHAPES = 3 * 64 * sum(1 + sum(b <= T for b in PLAN_STARTS) for T in range(1, 255))


@needs_cxx
def test_plan_over_every_shape(ask):
    """EVERY (T, K, L, B), T in [1, 254], K in {1, 2, 3}, L in [1, 64], B in {1, 2, 3, 5, 8, 31, T} (B <= T), none left out -- each at the
    most classes a call admits there (the lanes and the grid do not depend on C; LDS grows with it): the plan is its formula, the lanes
    cover every (b, l), LDS within the bound, per_block >= 1, G a power of two >= Lp"""
    rows_bytes, bound = (int(v) for v in ask(["C"])[0][5:7])
    assert rows_bytes == 32768 and bound == 32768 + 3584 + 9 * 4 * 4 <= 65536
    assert most_classes(254, 64) == 3 and most_classes(112, 1) == 7 and most_classes(112, 57) == 6 and most_classes(100, 48) == 8 and most_classes(100, 49) == 7
    shapes = [(T, K) for T in range(1, 255) for K in (1, 2, 3)]
    lines = [f"P {T} {K} {1000 + T}" for T, K in shapes]
    groups, pers, classes, n = set(), set(), set(), 0
    for (T, K), got in zip(shapes, ask(lines)):
        vals = np.array(got, dtype=np.int64).reshape(64, 7, 6)
        M = 1000 + T
        for i, B in enumerate(PLAN_STARTS + (T,)):
            if B > T:
                assert not vals[:, i].any()
                continue
            for L in range(1, 65):
                C_, Lp, G, per, blocks, lds = (int(v) for v in vals[L - 1, i])
                at = (T, K, L, B)
                assert C_ == most_classes(T, L) and 4 * C_ * T + 8 * L <= 3584 and C_ * T <= 896, at
                assert (Lp, G, per, blocks, lds) == expected_plan(T, K, C_, L, B, M), at
                assert G & (G - 1) == 0 and Lp <= G <= 256 and L <= Lp < 2 * L, at
                assert per >= 1 and per * G <= 256, at                          # every trajectory of the workgroup has its G lanes ...
                assert -(-(B * Lp) // G) * G >= B * Lp, at                      # ... which reach every (b, l) in ceil(B Lp / G) rounds
                assert blocks * per >= M > (blocks - 1) * per, at
                assert lds <= bound and (per == 1 or per * T * (48 + 4 * K) <= rows_bytes), at
                groups.add(G)
                pers.add(per)
                classes.add(C_)
                n += 1
    assert n == PLAN_SHAPES == 332928                               # 1 734 (T, B) pairs x 64 ladders x 3 map counts: none skipped
    assert groups == {1, 2, 4, 8, 16, 32, 64, 128, 256} and {1, 2, 17, 256} <= pers and classes == {3, 4, 5, 6, 7, 8}
    # the bench's shapes: 23 levels at B = 5 and B = 31 are one trajectory per workgroup; L = 2, B = 1 is capped by the rows, not the lanes
    assert expected_plan(31, 2, 3, 23, 5, 10000)[1:4] == (256, 1, 10000) and expected_plan(31, 2, 3, 23, 31, 10000)[1:4] == (256, 1, 10000)
    assert expected_plan(31, 3, 3, 2, 1, 100)[1:3] == (2, 17) and 128 * 31 * 60 > rows_bytes


# ------------------------------------------------------------------------------------------------ the checker by hand
def test_the_checker_on_a_hand_case():
    """a self-check of the CHECKER alone (it runs no product code): three brake starts, ladder 0.5 / 2 / 6.5: start 1 needs level 2 and is blocked below by user 1; start 2 has no level at all but
    lies beyond a candidate of two samples"""
    ra, blk, req = [0, 2, -1], [0, 0b10, 0b01], [[0, 1, -1], [0, 2, 0]]
    assert LV.fold_one(ra, blk, req, 2, LEVELS) == (2, 1, 0b10, 1, 6.5, [1, 2])
    assert LV.fold_one(ra, blk, req, 3, LEVELS) == (3, 2, 0b01, 0, math.inf, [3, 2])
    assert LV.fold_one(ra, blk, req, 0, LEVELS) == (-1, -1, 0, -1, 0.0, [-1, -1])
    assert LV.fold_one(ra, blk, req, 1, LEVELS, finite=False) == (3, 0, 0, -2, math.inf, [0, 0])
    assert LV.fold_one([1, 1, 1], [4, 2, 1], [[1, 1, 1]], 3, LEVELS)[:4] == (1, 0, 4, 2)          # a tie stays with the first start
    row, safe = LV.fold_row(ROWS["clean"][0], 1, 2, 1, 6.5, 3, 6.5)
    assert safe == 1 and row[LV.C_RES0] == 6.5 and row[LV.C_RES1] == 1.0 and row[LV.C_SAFE] == 1.0
    row, safe = LV.fold_row(ROWS["clean"][0], 1, 2, 1, 6.5, 3, 6.0)
    assert safe == 0 and row[LV.C_SAFE] == 0.0
    assert LV.fold_row(ROWS["clean"][0], 1, 3, 0, math.inf, 3, math.inf)[1] == 0                    # "no level" loses safety at any limit
    out = LV.verdict([ra, ra], [blk, blk], [[r, r] for r in req], [[-1, 4], [0, 0]], LEVELS, 3, 3, lens=[2, 7], finite=[1, 1])
    assert out["need"].tolist() == [2, 3] and out["at"].tolist() == [1, 2] and out["need_of"].tolist() == [[1, 3], [2, 2]]
    assert out["first"].tolist() == [[-1, 4], [0, 0]] and out["decel"].tolist() == [6.5, math.inf]


# ------------------------------------------------------------------------------------------------ the planning step's validation
def test_planning_step_refuses_before_it_allocates():
    """hidden_ladder_verdict= is validated before the step touches the device: stand-ins without one show the refusals"""
    from frenetix_occlusion.step import PlanningStep, hidden_ladder_verdict_options
    ctx = object()
    stage = SimpleNamespace(ctx=ctx)
    good = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, levels=[1.0, 2.0], starts=5, a_limit=8.0)
    hv = dict(vehicle=(4.5, 1.8, 1.4), users=((2.0, "road", "any"),), dt=0.1, a_brake=8.0, starts=5, commit_min=5)
    step = lambda **kw: PlanningStep(stage, stage, stage, None, None, None, None, **kw)
    with pytest.raises(ValueError, match="same two reserved cost columns"):
        step(hidden_verdict=hv, hidden_ladder_verdict=good)
    for bad in (dict(users=good["users"]), {k: v for k, v in good.items() if k != "a_limit"}, dict(good, a_brake=8.0), dict(good, commit_min=1),
                {k: v for k, v in good.items() if k != "levels"}, 5, "levels"):
        with pytest.raises(ValueError, match="hidden_ladder_verdict"):
            step(hidden_ladder_verdict=bad)
    with pytest.raises(ValueError, match=r"missing: \['a_limit', 'levels'\]"):
        hidden_ladder_verdict_options(None, {k: v for k, v in good.items() if k not in ("a_limit", "levels")})
    with pytest.raises(ValueError, match=r"unknown: \['a_brake'\]"):
        hidden_ladder_verdict_options(None, dict(good, a_brake=1.0))
    assert hidden_ladder_verdict_options(None, None) is None and hidden_ladder_verdict_options(hv, None) is None
    got = hidden_ladder_verdict_options(None, dict(good, margin=0.5, inflate=0.1, lengths=[1, 2]))
    assert got == dict(good, margin=0.5, inflate=0.1, lengths=[1, 2]) and got is not good


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_entry_and_keeps_the_abi():
    import ctypes as C
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import sensor_model as SM
    lib = N.load()
    assert "fo_scene_hidden_brake_ladder_verdict" in N.EXPORTS and hasattr(lib, "fo_scene_hidden_brake_ladder_verdict")
    assert lib.fo_abi_version() == 12
    # the ladder-users inputs word for word (its nine output pointers left out), then a_limit, finite, cost, safe and seven outputs
    assert C.sizeof(N.HiddenBrakeLadderVerdict) == C.sizeof(N.HiddenBrakeLadderUsers) - 9 * 8 + 8 + 3 * 8 + 7 * 8
    names = [f[0] for f in N.HiddenBrakeLadderUsers._fields_]
    assert [f[0] for f in N.HiddenBrakeLadderVerdict._fields_][:names.index("d_required")] == names[:names.index("d_required")]
    assert SM.SensorModel.hidden_brake_ladder_verdict is not None and SM.HiddenBrakeLadderVerdict is not None
