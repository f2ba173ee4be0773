"""The sweep's launch plan (csrc/fo_sweep_plan.hpp: plan_sweep, max_chunk_cells, max_chunk_rows) on the CPU: a driver of a
few lines around the header is built with the host C++ compiler -- the header is host-only integer arithmetic -- and asked
for the plan of a grid of batch shapes and knob settings.  Checked: the chunks cover the agents exactly once, the grid,
the precedence of the agents-per-wave settings, the taper cases of tests/test_sweep_gate_gpu.py, fo_sweep_reserve's worst
case against the planner, and launch geometries recorded on the MI355X."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

DRIVER = r"""
#include <cstdio>
#include "fo_sweep_plan.hpp"
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'R') {   // R max_M max_T max_A -> cells rows
      int m, t, a;
      if (scanf("%d %d %d", &m, &t, &a) != 3) return 1;
      printf("%zu %zu\n", max_chunk_cells(m, a), max_chunk_rows(a));
      continue;
    }
    int M, T, A, Ta, tuned, force, fg, ht;
    SweepKnobs k;
    if (scanf("%d %d %d %d %d %d %d %d %d %d %d %lf %lf %lf", &M, &T, &A, &Ta, &tuned, &force, &fg, &k.apw, &k.split, &k.split_apw,
              &ht, &k.taper[0], &k.taper[1], &k.taper[2]) != 14) return 1;
    k.force_generic = fg != 0;
    k.has_taper = ht != 0;
    const SweepPlan p = plan_sweep(M, T, A, Ta, tuned, force, k);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)p.use_queue, (int)p.split, p.wpb, p.apw, p.n_chunks, p.ph_n[0],
           p.ph_n[1], p.ph_n[2], p.ph_a[0], p.ph_a[1], p.ph_a[2], p.ph_a[3], p.Mp, p.n_tiles, p.grid, p.block);
  }
  return 0;
}
"""
FIELDS = ("use_queue", "split", "wpb", "apw", "n_chunks", "n0", "n1", "n2", "a0", "a1", "a2", "a3", "Mp", "n_tiles", "grid", "block")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-I" + CSRC, str(d / "driver.cpp"), "-o", exe])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(lines) + 1
        return [[int(v) for v in ln.split()] for ln in out[:-1]]
    return ask


def knobs_of(env):
    """the FO_SWEEP_* environment as read_knobs (fo_sweep.hip) hands it to the planner: -1 / 0 = not set"""
    k = {"fg": int(env.get("FO_SWEEP_GENERIC", "0")[:1] == "1"), "apw": int(env.get("FO_SWEEP_APW", -1)), "split": -1,
         "split_apw": int(env.get("FO_SWEEP_SPLIT_APW", -1)), "ht": 0, "f": [1.0, 0.0, 0.0]}
    if "FO_SWEEP_SPLIT" in env:
        k["split"] = int(env["FO_SWEEP_SPLIT"][:1] == "1")
    if "FO_SWEEP_TAPER" in env:
        k["ht"] = 1
        for i, v in enumerate(env["FO_SWEEP_TAPER"].split(",")[:3]):
            k["f"][i] = float(v)
    return k


def query(M, T, A, Ta, env=None, tuned=0, force=0):
    k = knobs_of(env or {})
    return "P %d %d %d %d %d %d %d %d %d %d %d %r %r %r" % (M, T, A, Ta, tuned, force, k["fg"], k["apw"], k["split"], k["split_apw"],
                                                            k["ht"], *k["f"])


def plans(planner, queries):
    return [dict(zip(FIELDS, row)) for row in planner(queries)]


def chunk_ranges(p):
    """[first agent, one past the last) of every chunk: the chunk table as fo_prep_traj.hpp fills it from (n0..n2, a0..a3, wpb),
    read the way the kernels read it -- the horizon-split form takes agents [c apw, (c + 1) apw) without the table"""
    if p["split"]:
        return [(c * p["apw"], (c + 1) * p["apw"]) for c in range(p["n_chunks"])]
    n0, n1, n2, a0, a1, a2, a3, wpb = (p[k] for k in ("n0", "n1", "n2", "a0", "a1", "a2", "a3", "wpb"))
    out = []
    for c in range(p["n_chunks"]):
        if c < n0:
            ap, k0 = a0, c * a0
        elif c < n0 + n1:
            ap, k0 = a1, n0 * a0 + (c - n0) * a1
        elif c < n0 + n1 + n2:
            ap, k0 = a2, n0 * a0 + n1 * a1 + (c - n0 - n1) * a2
        else:
            ap, k0 = a3, n0 * a0 + n1 * a1 + n2 * a2 + (c - n0 - n1 - n2) * a3
        out.append((k0 * wpb, k0 * wpb + wpb * ap))     # wave w: [k0 wpb + w ap, + ap)
    return out


N_TILES = (1, 2, 47, 48, 64, 97, 155, 157)
AGENTS = (0, 1, 3, 4, 5, 31, 32, 63, 129, 255, 256, 257, 1000)
HORIZONS = (2, 31, 32, 33, 60, 300)
KNOB_SETS = ([{}, {"FO_SWEEP_GENERIC": "1"}, {"FO_SWEEP_SPLIT": "0"}, {"FO_SWEEP_SPLIT": "1"}, {"FO_SWEEP_SPLIT_APW": "2"},
              {"FO_SWEEP_TAPER": "0"}, {"FO_SWEEP_TAPER": "0.5,0.3,0.1"}] +
             [{"FO_SWEEP_APW": str(a)} for a in (1, 2, 4, 8)] + [{"FO_SWEEP_APW": str(a), "FO_SWEEP_TAPER": "0"} for a in (1, 2, 4, 8)])


def shapes():
    for nt, A, T in itertools.product(N_TILES, AGENTS, HORIZONS):
        for Ta in sorted({31, T, T + 5}):
            yield 64 * nt - (nt % 3) * 21, T, A, Ta     # (ragged last tiles as well: 64 nt, 64 nt - 21, 64 nt - 42)


def test_chunks_cover_the_agents_once_and_the_grid_follows(planner):
    cases = [(s, env) for s in shapes() for env in KNOB_SETS]
    got = plans(planner, [query(*s, env=env) for s, env in cases])
    kernels = set()
    for ((M, T, A, Ta), env), p in zip(cases, got):
        why = (M, T, A, Ta, env, p)
        assert p["n_tiles"] == (M + 63) // 64 and p["Mp"] == 64 * p["n_tiles"], why
        reach = T <= Ta + 255 or A == 0
        assert p["use_queue"] == int(reach and "FO_SWEEP_GENERIC" not in env), why
        assert p["wpb"] == 4 and p["block"] == 256, why
        if p["split"]:
            assert p["use_queue"] and T <= 32, why
        rng = chunk_ranges(p)
        assert len(rng) == p["n_chunks"], why
        assert p["n0"] >= 0 and p["n1"] >= 0 and p["n2"] >= 0 and p["n0"] + p["n1"] + p["n2"] <= p["n_chunks"], why
        at = 0
        for lo, hi in rng:          # disjoint, ascending, no hole
            assert lo == at and hi > lo, why
            at = hi
        if A == 0:
            assert rng == [], why
        else:                       # exactly [0, A) up to the padding of the last chunk
            assert rng[-1][0] < A <= at, why
        assert p["grid"] == 8 * ((p["n_tiles"] + 7) // 8) * p["n_chunks"], why
        kernels.add((p["use_queue"], p["split"], p["n1"] + p["n2"] > 0))
    # the matrix meets the generic kernel (T = 300 against Ta = 31 crosses the row reach), the split, plain and tapered forms
    assert kernels == {(0, 0, False), (1, 1, False), (1, 0, False), (1, 0, True)}, kernels
    by = {(s, tuple(sorted(env.items()))): p for (s, env), p in zip(cases, got)}
    assert by[((43, 300, 32, 31), ())]["use_queue"] == 0 and by[((43, 300, 32, 300), ())]["use_queue"] == 1


def test_list_offsets_beyond_4_gb_take_the_generic_kernel(planner):
    # (T - 1) M pairs of float64 per agent: 16 bytes each, below 2^32
    a, b = plans(planner, [query(2 ** 28 // 30, 31, 4, 31), query(2 ** 28 // 30 + 1, 31, 4, 31)])
    assert (2 ** 28 // 30) * 30 * 16 < 2 ** 32 <= (2 ** 28 // 30 + 1) * 30 * 16
    assert a["use_queue"] == 1 and b["use_queue"] == 0


def test_agents_per_wave_precedence(planner):
    M, T, A, Ta = 10000, 31, 256, 31
    static, tuned, forced, env, both = plans(planner, [
        query(M, T, A, Ta), query(M, T, A, Ta, tuned=2), query(M, T, A, Ta, tuned=2, force=1),
        query(M, T, A, Ta, {"FO_SWEEP_APW": "8"}, tuned=2, force=1), query(M, T, A, Ta, {"FO_SWEEP_APW": "8"}, tuned=2)])
    # (static: 157 tiles x ceil(256 / 32) chunks x 4 waves = 5 024 < 8 192 at 8 agents per wave, 10 048 at 4)
    assert (static["apw"], tuned["apw"], forced["apw"], env["apw"], both["apw"]) == (4, 2, 1, 8, 8)
    out_of_range = plans(planner, [query(M, T, A, Ta, {"FO_SWEEP_APW": v}, tuned=4) for v in ("0", "65", "-3")])
    assert [p["apw"] for p in out_of_range] == [4, 4, 4]
    # the horizon-split form: one agent per workgroup whatever the other settings say, unless FO_SWEEP_SPLIT_APW speaks
    M, A = 2000, 32
    sp = plans(planner, [query(M, T, A, Ta), query(M, T, A, Ta, tuned=4, force=2), query(M, T, A, Ta, {"FO_SWEEP_APW": "8"}),
                         query(M, T, A, Ta, {"FO_SWEEP_SPLIT_APW": "3"}, tuned=4),
                         query(M, T, A, Ta, {"FO_SWEEP_SPLIT_APW": "17"}), query(M, T, A, Ta, {"FO_SWEEP_SPLIT": "0"}, tuned=4),
                         query(10000, T, 256, Ta, {"FO_SWEEP_SPLIT": "1"}, tuned=4), query(M, 33, A, 33, {"FO_SWEEP_SPLIT": "1"})])
    assert [(p["split"], p["apw"]) for p in sp] == [(1, 1), (1, 1), (1, 1), (1, 3), (1, 1), (0, 4), (1, 1), (0, 1)]
    assert sp[0]["n_chunks"] == 32 and sp[3]["n_chunks"] == 11


# tests/test_sweep_gate_gpu.py::TAPER_CASES (that test adds FO_SWEEP_SPLIT=0) -- the same table, read off the plan
def test_the_taper_cases_of_the_gate_test_plan_as_its_table_says(planner):
    import ast
    src = open(os.path.join(ROOT, "tests", "test_sweep_gate_gpu.py")).read()
    tree = ast.parse(src)
    table = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "TAPER_CASES")
    assert len(table) == 5
    got = plans(planner, [query(M, 31, A, 31, {**env, "FO_SWEEP_SPLIT": "0"}) for M, A, env, _ in table])
    for (M, A, env, tapered), p in zip(table, got):
        untapered = p["n_tiles"] * ((A + 4 * p["apw"] - 1) // (4 * p["apw"]))     # the gate test's own criterion
        assert (p["apw"] >= 2 and p["grid"] != untapered) == tapered, (M, A, env, p)
        assert (p["n1"] + p["n2"] > 0 or p["a3"] != p["a0"]) == tapered, (M, A, env, p)
        if "FO_SWEEP_APW" in env:
            assert p["apw"] == int(env["FO_SWEEP_APW"])


def test_reserve_covers_every_plan_within_its_sizes(planner):
    """fo_sweep_reserve(max_M, max_T, max_A) sets aside max_chunk_cells x NPS x TILE doubles of partial rows and max_chunk_rows
    chunk-table rows; a plan needs n_tiles x (n_chunks + 1) cells and n_chunks + 1 rows.  No knob set.  (max_T is no input of the
    bound: a batch may be shorter than it, so max_T = 33 must still hold the horizon-split plan of 43 x 4 agents x 2 samples.)"""
    maxima = [(64 * nt, T, A) for nt in (1, 2, 47, 48, 97, 157) for T in (2, 31, 32, 33, 60, 300) for A in (0, 1, 5, 32, 63, 257, 1000)]
    res = planner(["R %d %d %d" % m for m in maxima])
    batch = [s for s in shapes() if s[3] in (31, s[1])]
    got = plans(planner, [query(*s) for s in batch])
    checked = 0
    for (mM, mT, mA), (cells, rows) in zip(maxima, res):
        for (M, T, A, Ta), p in zip(batch, got):
            if M <= mM and T <= mT and A <= mA:
                assert p["n_tiles"] * (p["n_chunks"] + 1) <= cells, ((mM, mT, mA), (M, T, A, Ta), p, cells)
                assert p["n_chunks"] + 1 <= rows, ((mM, mT, mA), (M, T, A, Ta), p, rows)
                checked += 1
    assert checked > 10000      # (the loops above met something)


# (grid, block, agents per wave) as fo_sweep_last_launch reported them on an MI355X at revision 88640cd, the last one whose
# sweep_run planned in line: bench.py's headline batch and small step in the three output modes, the taper cases, and a
# wider net of shapes and knobs.  No autotuned entry.  Integers: equal or wrong.
# (M, A, T, Ta, environment, (grid, block, agents per wave));  the comment names the output mode of the recorded run
RECORDED = [
    (10000, 256, 31, 31, {}, (3520, 256, 4)),    # full
    (10000, 256, 31, 31, {}, (3520, 256, 4)),    # pair
    (10000, 256, 31, 31, {}, (3520, 256, 4)),    # reduced
    (2000, 32, 31, 31, {}, (1024, 256, 1)),    # full
    (2000, 32, 31, 31, {}, (1024, 256, 1)),    # pair
    (2000, 32, 31, 31, {}, (1024, 256, 1)),    # reduced
    (4095, 255, 31, 31, {"FO_SWEEP_SPLIT": "0"}, (2368, 256, 2)),    # pair
    (4095, 255, 31, 31, {}, (2368, 256, 2)),    # reduced
    (4097, 257, 31, 31, {"FO_SWEEP_SPLIT": "0"}, (2736, 256, 2)),    # pair
    (4097, 257, 31, 31, {}, (2736, 256, 2)),    # reduced
    (6143, 255, 31, 31, {"FO_SWEEP_APW": "8", "FO_SWEEP_SPLIT": "0"}, (2304, 256, 8)),    # pair
    (6143, 255, 31, 31, {"FO_SWEEP_APW": "8"}, (2304, 256, 8)),    # reduced
    (9857, 129, 31, 31, {"FO_SWEEP_APW": "8", "FO_SWEEP_SPLIT": "0"}, (1920, 256, 8)),    # pair
    (9857, 129, 31, 31, {"FO_SWEEP_APW": "8"}, (1920, 256, 8)),    # reduced
    (4095, 255, 31, 31, {"FO_SWEEP_TAPER": "0", "FO_SWEEP_SPLIT": "0"}, (2048, 256, 2)),    # pair
    (4095, 255, 31, 31, {"FO_SWEEP_TAPER": "0"}, (2048, 256, 2)),    # reduced
    (64, 1, 31, 31, {}, (8, 256, 1)),    # reduced
    (64, 3, 31, 31, {}, (24, 256, 1)),    # reduced
    (128, 5, 31, 31, {}, (40, 256, 1)),    # reduced
    (3000, 31, 31, 31, {}, (1488, 256, 1)),    # reduced
    (3008, 63, 31, 31, {}, (3024, 256, 1)),    # reduced
    (3072, 129, 33, 33, {}, (1584, 256, 1)),    # reduced
    (4096, 255, 60, 60, {}, (2368, 256, 2)),    # reduced
    (6208, 1000, 31, 31, {}, (7384, 256, 8)),    # reduced
    (9920, 256, 31, 36, {}, (3520, 256, 4)),    # reduced
    (10048, 257, 32, 32, {}, (3680, 256, 4)),    # reduced
    (640, 32, 300, 31, {}, (128, 256, 1)),    # reduced
    (640, 32, 300, 300, {}, (128, 256, 1)),    # reduced
    (64, 32, 2, 31, {}, (256, 256, 1)),    # reduced
    (2000, 32, 31, 31, {"FO_SWEEP_SPLIT": "0"}, (256, 256, 1)),    # reduced
    (2000, 32, 31, 31, {"FO_SWEEP_SPLIT_APW": "2"}, (512, 256, 2)),    # reduced
    (2000, 32, 31, 31, {"FO_SWEEP_GENERIC": "1"}, (256, 256, 1)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_GENERIC": "1"}, (2560, 256, 4)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_SPLIT": "1"}, (40960, 256, 1)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_TAPER": "0.5,0.3,0.1"}, (4960, 256, 4)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_APW": "1"}, (10240, 256, 1)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_APW": "2"}, (5920, 256, 2)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_APW": "4"}, (3520, 256, 4)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_APW": "8"}, (3360, 256, 8)),    # reduced
    (10000, 256, 31, 31, {"FO_SWEEP_APW": "8", "FO_SWEEP_TAPER": "0"}, (1280, 256, 8)),    # reduced
    (2000, 32, 31, 31, {"FO_SWEEP_APW": "4"}, (1024, 256, 1)),    # reduced
    (2000, 32, 31, 31, {"FO_SWEEP_APW": "4", "FO_SWEEP_SPLIT": "0"}, (64, 256, 4)),    # reduced
]


def test_plans_equal_the_launches_recorded_before_the_planner_moved(planner):
    assert len(RECORDED) >= 11
    got = plans(planner, [query(M, T, A, Ta, env) for M, A, T, Ta, env, _ in RECORDED])
    for (M, A, T, Ta, env, launch), p in zip(RECORDED, got):
        assert (p["grid"], p["block"], p["apw"]) == launch, (M, A, T, Ta, env, p)
