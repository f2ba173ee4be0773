"""The host side of the hidden-traffic impact verdict by approach angle (DESIGN.md §5.10 "Impact verdict by approach angle"), without a
GPU: what a move byte says about a heading, by the builder's own predicate (scenario.lane_move_raster); the approach cosine and the
closing speed (csrc/fo_hidden_approach.hpp) built with the host C++ compiler -- as tests/test_hidden_impact_cpu.py builds
csrc/fo_hidden_impact.hpp -- against the plain statement tests/ref_hidden_impact_lanes.py bit for bit and against the reference's own
harm (tests/golden/hidden_impact_lanes.npz); the condition the device tests rest on -- no open choice of the start or of the user in any
of their raw-entry scenes -- by the checkers alone; the library's symbol and the Python layer's options."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import hidden_impact_cases as IC
import hidden_impact_lanes_cases as LC
import ref_hidden_impact as RI
import ref_hidden_impact_lanes as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
TOL = 1e-9                                          # the project's stated float tolerance (README, "GPU vs oracle")
SLACKS = (0.0, 0.2, math.pi / 2.0, math.pi)

DRIVER = r"""
#include <cstdio>
#include "fo_hidden_approach.hpp"
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'K') {          // K byte -> the mask of its central directions
      unsigned b;
      if (scanf("%u", &b) != 1) return 1;
      printf("%u\n", fo_hidden_approach_central(b));
    } else if (what == 'A') {   // A byte bound ct st cos_h sin_h u s -> cm w (hexadecimal floats: every bit)
      unsigned b;
      int bound;
      double ct, st, ch, sh, u, s;
      if (scanf("%u %d %la %la %la %la %la %la", &b, &bound, &ct, &st, &ch, &sh, &u, &s) != 8) return 1;
      const double cm = fo_hidden_approach_cosine(b, bound != 0, ct, st, ch, sh);
      printf("%a %a\n", cm, fo_hidden_approach_closing(u, s, cm));
    } else if (what == 'L') {   // L p_const p_speed w -> the logistic
      double a, b, w;
      if (scanf("%la %la %la", &a, &b, &w) != 3) return 1;
      printf("%a\n", fo_hidden_impact_logistic(a, b, w));
    } else {
      return 1;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("hidden_impact_lanes")
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
    return np.load(os.path.join(ROOT, "tests", "golden", "hidden_impact_lanes.npz"))


def _x(v):
    return float(v).hex()


def _f(s):
    return float.fromhex(s)


# ------------------------------------------------------------------------------------------------ what a byte says about a heading
def _bytes_of(yaws):
    """the move bytes of cells whose only lanelet has the headings ``yaws``, by scenario.lane_move_raster itself"""
    from frenetix_occlusion.scenario import lane_move_raster
    yaws = np.asarray(yaws, dtype=np.float64)
    n = len(yaws)
    return lane_move_raster(None, 0.0, 0.0, 1.0, n, 1, cells=[(0, 1, 0, n, np.arange(n), yaws)])[0]


def _sweep_headings():
    grid = np.deg2rad(np.arange(0, 72000) * 0.01)                                       # a 0.01 deg grid over two turns
    edges = [math.radians(22.5 * j) for j in range(-16, 33)]                            # every multiple of 22.5 deg
    near = []
    for e in edges:
        lo = hi = e
        for _ in range(10):                                                             # ten ulps either side of each
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            near += [float(lo), float(hi)]
    return np.concatenate((grid, np.array(edges), np.array(near)))


def _angle_between(a, b):
    return abs((a - b + math.pi) % (2.0 * math.pi) - math.pi)


def test_a_central_direction_lies_within_22_5_degrees_of_the_generating_heading():
    """the sector claim over the builder's own predicate: every heading of a fine sweep -- a 0.01 deg grid over two turns, every multiple
    of 22.5 deg and ten ulps either side of each -- lies within 22.5 deg of a central direction of the byte it generates, or that byte has
    no central direction at all (the float borderline at odd multiples of 22.5 deg, two bits), which is priced head-on"""
    yaws = _sweep_headings()
    assert len(yaws) > 72000
    bytes_ = _bytes_of(yaws)
    none = 0
    for yaw, b in zip(yaws.tolist(), bytes_.tolist()):
        ks = RL.central(b)
        if not ks:
            none += 1
            assert bin(b).count("1") <= 2, (yaw, b)
            continue
        assert min(_angle_between(yaw, k * math.pi / 4.0) for k in ks) <= math.pi / 8.0 + 1e-12, (math.degrees(yaw), b)
    print(f"{len(yaws)} headings: {none} give a byte without a central direction")
    assert none <= 64                                                                   # a borderline, not a habit
    # a 90 deg crossing of two lanelets: the union widens the sector, which still holds both headings
    both = int(_bytes_of([0.0])[0]) | int(_bytes_of([math.pi / 2.0])[0])
    assert RL.central(both) == [0, 1, 2] and RL.central(0xFF) == list(range(8)) and RL.central(0) == [] and RL.central(0b00000110) == []


# ------------------------------------------------------------------------------------------------ steps 3 - 4: the header is the checker
def _ego_headings():
    """64 unit headings: the 8 lattice ones, 1e-6 rad either side of each sector edge at every slack's h < pi as seen from theta + pi,
    and seeded ones"""
    th = [k * math.pi / 4.0 for k in range(8)]
    for slack in SLACKS[:3]:
        h = RL.BASE + slack
        for k in (0, 3, 5):
            for side in (-1.0, 1.0):
                edge = k * math.pi / 4.0 + side * h - math.pi                            # theta + pi sits on the sector's edge
                th += [edge - 1e-6, edge + 1e-6]
    rng = np.random.default_rng(20240923)
    th += rng.uniform(-math.pi, math.pi, 64 - len(th)).tolist()
    assert len(th) == 64
    return th


@needs_cxx
def test_cosine_and_closing_speed_are_the_checkers_bit_for_bit(ask):
    """all 256 bytes x 64 ego headings x slacks {0, 0.2, pi / 2, pi}, lane-bound or not: cm and w of the header are the checker's in every
    bit; w <= u + s always, w == u + s bit for bit where cm == 1.0; a byte without a central direction, a free class and h >= pi are
    head-on"""
    heads = _ego_headings()
    rng = np.random.default_rng(7)
    cases, lines = [], []
    for slack in SLACKS:
        cos_h, sin_h = RL.host_h(slack)
        for byte in range(256):
            for n, th in enumerate(heads):
                ct, st = math.cos(th), math.sin(th)
                bound = (byte + n) % 5 != 0
                u, s = float(rng.uniform(0.0, 16.0)), (2.0, 7.0, 13.9)[(byte + n) % 3]
                cases.append((slack, byte, bound, ct, st, cos_h, sin_h, u, s))
                lines.append(f"A {byte} {int(bound)} {_x(ct)} {_x(st)} {_x(cos_h)} {_x(sin_h)} {_x(u)} {_x(s)}")
    got = ask(lines)
    below = head_on = 0
    for case, g in zip(cases, got):
        slack, byte, bound, ct, st, cos_h, sin_h, u, s = case
        cm, w = RL.cosine(byte, bound, ct, st, cos_h, sin_h), None
        w = RL.closing(u, s, cm)
        assert (_f(g[0]).hex(), _f(g[1]).hex()) == (cm.hex(), w.hex()), case
        assert w <= u + s and -1.0 - 1e-15 <= cm <= 1.0, case
        if cm == 1.0:
            head_on += 1
            assert w.hex() == (u + s).hex(), case
        else:
            below += 1
            assert bound and RL.central(byte) and slack < math.pi, case
        if not bound or not RL.central(byte) or slack >= math.pi:
            assert cm == 1.0, case
    assert below > 10000 and head_on > 10000
    assert [int(g[0]) for g in ask([f"K {b}" for b in range(256)])] == [sum(1 << k for k in RL.central(b)) for b in range(256)]


def test_the_cosine_is_the_greatest_over_the_sectors():
    """the checker's step 3 against a dense scan of cos(yaw - theta + pi) over the headings H of the byte"""
    rng = np.random.default_rng(11)
    for _ in range(400):
        byte, th, slack = int(rng.integers(0, 256)), float(rng.uniform(-math.pi, math.pi)), float(rng.choice([0.0, 0.2, 1.0]))
        ks = RL.central(byte)
        if not ks:
            continue
        h = RL.BASE + slack
        yaws = np.concatenate([k * math.pi / 4.0 + np.linspace(-h, h, 2001) for k in ks] + [[th + math.pi] if any(
            _angle_between(th + math.pi, k * math.pi / 4.0) <= h for k in ks) else []])
        want = float(np.cos(yaws - th + math.pi).max())
        got = RL.cosine(byte, True, math.cos(th), math.sin(th), *RL.host_h(slack))
        assert abs(got - want) <= 1e-12, (byte, th, slack, got, want)


# ------------------------------------------------------------------------------------------------ the reference's own harm
def _stage_harm(ask, golden, block):
    rows = np.array([RI.row(str(k), l, w, float(golden["ego_mass"])) for k, (l, w) in zip(golden["kinds"], golden["dims"])])
    n = len(golden[f"{block}_kind"])
    lines = []
    for i in range(n):
        th, slack = float(golden[f"{block}_theta"][i]), float(golden[f"{block}_slack"][i])
        cos_h, sin_h = RL.host_h(slack)
        lines.append(f"A {int(golden[f'{block}_byte'][i])} 1 {_x(math.cos(th))} {_x(math.sin(th))} {_x(cos_h)} {_x(sin_h)} "
                     f"{_x(golden[f'{block}_v_ego'][i])} {_x(golden[f'{block}_v_obs'][i])}")
    cw = [(_f(g[0]), _f(g[1])) for g in ask(lines)]
    lines = []
    for i, (_, w) in enumerate(cw):
        r = rows[golden[f"{block}_kind"][i]]
        lines += [f"L {_x(r[0])} {_x(r[1])} {_x(w)}", f"L {_x(r[2])} {_x(r[3])} {_x(w)}"]
    harm = np.array([_f(g[0]) for g in ask(lines)]).reshape(-1, 2)
    return np.array(cw), harm


@needs_cxx
def test_the_stage_attains_the_references_harm_at_the_bound(ask, golden):
    """the reference's unmodified get_harm with the user's yaw at the maximiser over the byte's headings -- a side approach, the same
    direction, a sector that holds theta + pi, unions of sectors, non-lattice ego headings, a slack -- for Car, Bicycle, Pedestrian and Truck
    x ego speeds {0.5, 3, 8, 15} x user speeds {2.0, 7.0, 13.9}: the row's logistics at step 4's w give its harms to 1e-9"""
    assert [str(k) for k in golden["kinds"]] == ["Car", "Bicycle", "Pedestrian", "Truck"]
    assert sorted(set(golden["bound_v_ego"].tolist())) == [0.5, 3.0, 8.0, 15.0] and sorted(set(golden["bound_v_obs"].tolist())) == [2.0, 7.0, 13.9]
    combos = {(t, b, s) for t, b, s in zip(golden["bound_theta"].tolist(), golden["bound_byte"].tolist(), golden["bound_slack"].tolist())}
    assert len(combos) >= 6 and len(golden["bound_kind"]) == 4 * 4 * 3 * len(combos)
    assert np.array_equal(golden["coeff"], np.array(list(RI.COEFF.values())))
    cw, harm = _stage_harm(ask, golden, "bound")
    # the recorded yaw is the maximiser: its own cosine is the stage's
    own = np.cos(golden["bound_yaw"] - golden["bound_theta"] + math.pi)
    assert np.abs(own - cw[:, 0]).max() <= 1e-12
    worst_o, worst_e = np.abs(harm[:, 0] - golden["bound_obst_harm"]).max(), np.abs(harm[:, 1] - golden["bound_ego_harm"]).max()
    print(f"stage against the reference at the bound: worst |obstacle harm| difference {worst_o:.3e}, ego {worst_e:.3e}; "
          f"cosines {sorted(set(np.round(cw[:, 0], 4).tolist()))}")
    assert worst_o <= TOL and worst_e <= TOL
    cs = cw[:, 0]
    assert (cs == 1.0).any() and (cs < -0.9).any() and ((cs > 0.3) & (cs < 0.5)).any()   # head-on, from behind, from the side
    head_on = np.array([RI.logistic(*RI.row(str(golden["kinds"][k]), *golden["dims"][k], float(golden["ego_mass"]))[:2], float(ve) + float(vo))
                        for k, ve, vo in zip(golden["bound_kind"], golden["bound_v_ego"], golden["bound_v_obs"])])
    assert (golden["bound_obst_harm"] <= head_on + 1e-12).all() and (head_on - golden["bound_obst_harm"]).max() > 1e-3


@needs_cxx
def test_no_recorded_reference_harm_exceeds_the_stage(ask, golden):
    """256 pairs per type, the user's yaw uniform inside the headings of its byte, random positions and speeds: the reference's harm never
    exceeds the stage's by more than 1e-12"""
    assert all((golden["rand_kind"] == k).sum() == 256 for k in range(4))
    h = RL.BASE + golden["rand_slack"]
    inside = [min(_angle_between(y, k * math.pi / 4.0) for k in RL.central(int(b))) <= hh + 1e-12
              for y, b, hh in zip(golden["rand_yaw"].tolist(), golden["rand_byte"].tolist(), h.tolist())]
    assert all(inside)
    cw, harm = _stage_harm(ask, golden, "rand")
    excess_o, excess_e = (golden["rand_obst_harm"] - harm[:, 0]).max(), (golden["rand_ego_harm"] - harm[:, 1]).max()
    print(f"random pairs: largest excess of the reference's obstacle harm over the stage's {excess_o:.3e}, of its ego harm {excess_e:.3e}; "
          f"{int((cw[:, 0] < 1.0).sum())} of {len(cw)} below head-on")
    assert excess_o <= 1e-12 and excess_e <= 1e-12
    assert (cw[:, 0] < 1.0).sum() > 500 and (harm[:, 0] - golden["rand_obst_harm"]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ the condition of the device tests
def test_no_open_choice_in_any_raw_entry_scene_of_the_device_tests():
    """the condition tests/test_hidden_impact_lanes_gpu.py compares ``at`` and ``user`` exactly under: in every raw-entry scene of its
    checker test no two starts of a class have closing speeds within 4 ulp unless they are the same number, and no two classes have
    harms within 1e-9 unless they come from the same row and w; and the scenes bite: lane-bound classes are priced below head-on"""
    import ref_hidden_brake_users as BU
    SC = IC.SC
    road = SC.road_raster()
    users_out = {}
    below = hits = 0
    for name, C_, K, tab, mask, slack, B in LC.RAW_CASES:
        sc, keys, qmins, thr, map_of, r2_caps, rows, speed_of = LC.raw_scene(name, C_, K)
        if (name, C_, K) not in users_out:
            users_out[name, C_, K] = BU.brake_users(keys, sc.win, road, qmins, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW,
                                                    SC.WB, sc.a_brake, sc.dt, thr, map_of, sc.lens)
        bf, stop, _, first = users_out[name, C_, K]
        cos_h, sin_h = RL.host_h(slack)
        harm, user, clos, at, cosn, n_open, by_start = RL.impact_lanes(
            keys, sc.win, road, LC.table(tab), SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB, sc.a_brake, sc.dt, thr,
            map_of, B, rows, speed_of, mask, cos_h, sin_h, bf, stop, first, sc.lens)
        assert n_open == 0 and RL.close_starts(by_start) == 0, (name, C_, K, tab, mask, slack, B)
        # never above head-on, and head-on where the class is free
        _, _, speed, at0, _ = RI.impact(bf, stop, first, sc.v, sc.a_brake, sc.dt, B, rows, speed_of, sc.lens)
        head_on = np.where(at0 >= 0, speed + np.asarray(speed_of)[:, None], 0.0)
        assert (clos <= head_on).all() and ((at >= 0) == (at0 >= 0)).all()
        for c in range(C_):
            if not mask >> c & 1:
                assert clos[c].tobytes() == head_on[c].tobytes() and np.array_equal(at[c], at0[c]) and (cosn[c] == 1.0).all()
        below += int((clos < head_on).sum())
        hits += int((at >= 0).sum())
    print(f"{len(LC.RAW_CASES)} raw-entry cases: {hits} (class, trajectory) pairs with a hit, {below} priced below head-on")
    assert hits > 100 and below > 30


# ------------------------------------------------------------------------------------------------ the library and the Python layer
def test_library_exports_the_entry_and_keeps_the_abi():
    from frenetix_occlusion import _native as N
    import ctypes as C
    lib = N.load()
    assert "fo_scene_hidden_brake_impact_lanes" in N.EXPORTS and hasattr(lib, "fo_scene_hidden_brake_impact_lanes")
    assert lib.fo_abi_version() == 12
    # the head-on structure with d_closing for d_speed, and: dir_mask (padded), cos_h, sin_h, d_cosine
    assert C.sizeof(N.HiddenBrakeImpactLanes) == C.sizeof(N.HiddenBrakeImpact) + 4 * 8
    assert N.HiddenBrakeImpactLanes.d_closing.offset == N.HiddenBrakeImpact.d_speed.offset
    ctx_free = N.HiddenBrakeImpactLanes()
    assert ctx_free.dir_mask == 0


def test_stage_options_take_the_two_keywords():
    from frenetix_occlusion.step import hidden_stage_options
    iv = dict(vehicle=(4.5, 1.8, 1.4), ego_mass=1200.0, users=((2.0, "road", "any"),), kinds=(("Pedestrian", 0.4, 0.6),), dt=0.1, a_brake=8.0,
              starts=5, harm_limit=0.1)
    got = hidden_stage_options(None, None, dict(iv, approach="lanes", heading_slack=0.2))[1]
    assert got == dict(iv, approach="lanes", heading_slack=0.2)
    with pytest.raises(ValueError, match="hidden_impact_verdict"):
        hidden_stage_options(None, None, dict(iv, angle="lanes"))


def test_the_result_names_closing_speed_where_there_is_no_impact_speed():
    import torch
    from frenetix_occlusion.hidden_traffic import HiddenBrakeImpact
    z = torch.zeros((1, 2), dtype=torch.float64)
    at = torch.tensor([[0, -1]], dtype=torch.int32)
    user = torch.tensor([0, -1], dtype=torch.int32)
    lanes = HiddenBrakeImpact(z.T.clone(), user, None, at, at, at, np.zeros((1, 4)), np.array([2.0]), (), 0.1,
                              closing=torch.tensor([[5.0, 0.0]], dtype=torch.float64), cosine=torch.tensor([[0.5, 1.0]], dtype=torch.float64),
                              approach="lanes")
    with pytest.raises(ValueError, match="closing_speed"):
        lanes.impact_speed()
    assert lanes.closing_speed().tolist() == [5.0, 0.0] and lanes.approach_cosine().tolist() == [0.5, 1.0]
    assert lanes.closing_speed(0).tolist() == [5.0, 0.0]
    head = HiddenBrakeImpact(z.T.clone(), user, torch.tensor([[3.0, 0.0]], dtype=torch.float64), at, at, at, np.zeros((1, 4)), np.array([2.0]), (), 0.1)
    assert head.closing is None and head.approach == "head_on"
    assert head.impact_speed().tolist() == [3.0, 0.0] and head.closing_speed().tolist() == [5.0, 0.0] and head.approach_cosine().tolist() == [1.0, 1.0]
