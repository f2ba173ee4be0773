"""The host decisions of the scene stage (csrc/fo_scene_plan.hpp) on the CPU: a driver of a few lines around the header is
built with the host C++ compiler -- the header is host-only integer arithmetic -- and asked over stdin.  The form rules are
held to their independent Python restatement tests/scene_forms.expected_form (which the GPU form tests use to say what a
scene is meant to exercise), the integer square root to math.isqrt, and the reaches derived from it to the formulas of
tests/ref_occlusion_memory_road.py and tests/ref_hidden_reach_road.py."""
import itertools
import math
import os
import shutil
import subprocess

import pytest

import ref_hidden_reach_road as RR
import ref_occlusion_memory_road as OMR
import scene_forms as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include <cstdio>
#include "fo_hip.h"
#include "fo_scene_plan.hpp"
int main() {
  char what;
  long long v;
  while (scanf(" %c", &what) == 1) {
    if (what == 'F') {          // F E O forced cells -> waves two_launch
      int E, O, forced, cells;
      if (scanf("%d %d %d %d", &E, &O, &forced, &cells) != 4) return 1;
      printf("%d %d\n", ray_waves(E, O, forced != 0), (int)compact_two_launches(cells));
    } else if (what == 'V') {   // V n_rays -> rays per thread
      if (scanf("%lld", &v) != 1) return 1;
      printf("%d\n", fv_rays_per_thread((int)v));
    } else if (what == 'S') {   // S v -> isqrt
      if (scanf("%lld", &v) != 1) return 1;
      printf("%lld\n", (long long)isqrt(v));
    } else if (what == 'R') {   // R r2 -> h L n bands small
      if (scanf("%lld", &v) != 1) return 1;
      const int L = road_reach((int)v);
      printf("%d %d %d %d %d\n", reach_cells((int)v), L, road_steps(L), reach_bands(L), (int)omr_small(road_steps(L)));
    } else if (what == 'C') {   // C -> the constants
      printf("%d %d %d %d %d %d %d\n", FO_HIDDEN_REACH_MAX_HALO, FO_OCCLUSION_MEMORY_MAX_HALO, SCENE_CHUNK, COMPACT_ONE_LAUNCH,
             FV_THREADS, HRR_BAND, OMR_SMALL_N);
    } else {
      return 1;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_plan")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(d / "driver.cpp"), "-o", exe])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [[int(v) for v in ln.split()] for ln in out[:-1]]
    return ask


@pytest.fixture(scope="module")
def caps(plan):
    reach_cap, memory_cap, chunk, one_launch, fv_threads, band, small_n = plan(["C"])[0]
    # the constants the Python restatements carry on their own
    assert (chunk, one_launch) == (F.CHUNK, F.ONE_LAUNCH_BLOCKS) and fv_threads == 256 and band == 12 * 16 and small_n == 16
    return reach_cap, memory_cap


def test_form_rules_equal_their_python_restatement(plan):
    E = (0, 1, 4032, 4033, 4096, 4097, 4160)
    O = (0, 16, 17)
    cells = (1, 256, 2048 * 256, 2048 * 256 + 1, 725 ** 2, 901 ** 2)
    cases = list(itertools.product(E, O, (0, 1), (0, 1), cells))
    got = plan(["F %d %d %d %d" % (e, o, forced, c) for e, o, forced, skip, c in cases])
    forms = set()
    for (e, o, forced, skip, c), (waves, two) in zip(cases, got):
        # SKIP is no decision of the plan: the form follows the presence of the table (launch_rays / launch_settle)
        assert (waves, bool(skip), bool(two)) == F.expected_form(e, o, skip, c, forced), (e, o, forced, skip, c)
        forms.add((waves, two))
    assert forms == {(1, 0), (1, 1), (5, 0), (5, 1)}


def test_rays_per_thread_of_the_future_visibility(plan):
    assert [r[0] for r in plan(["V %d" % n for n in (4, 256, 257, 512, 513, 768)])] == [1, 1, 2, 2, 3, 3]


def test_the_integer_square_root_is_exact_around_every_square(plan, caps):
    top = 13 * (caps[0] + 1)
    values = [v for k in range(1, top + 1) for v in (k * k - 1, k * k, k * k + 1)]
    assert [r[0] for r in plan(["S %d" % v for v in values])] == [math.isqrt(v) for v in values]


def test_reaches_derived_from_a_squared_radius(plan, caps):
    """h = isqrt(r2), L = isqrt(169 r2) (ref_hidden_reach_road.reach_units, ref_occlusion_memory_road.reach_units),
    n = L // 12 (ref_occlusion_memory_road.halo), max(1, ceil(L / 192)) band launches (B = 12 x 16), and the
    road occlusion memory's small form up to n = 16"""
    reach_cap, memory_cap = caps
    r2s = sorted({0, 1, 2, 3, 4} | {v for k in range(1, reach_cap + 2) for v in (k * k - 1, k * k)})
    assert r2s[-1] == (reach_cap + 1) ** 2            # the first refused reach included: the largest accepted one is just below it
    got = plan(["R %d" % r2 for r2 in r2s])
    units = RR.reach_units(r2s)
    for r2, L_ref, (h, L, n, bands, small) in zip(r2s, units, got):
        assert h == math.isqrt(r2) and L == int(L_ref), r2
        assert bands == max(1, -(-L // 192)), r2
        if r2 <= memory_cap ** 2:                     # what the occlusion memory's arming call accepts
            assert L == OMR.reach_units(r2) and n == OMR.halo(r2) and small == int(n <= 16), r2
    assert {b for *_, b, _ in got} >= {1, 2, 18}      # no reach, more than one band, the 18 bands of the longest reach
