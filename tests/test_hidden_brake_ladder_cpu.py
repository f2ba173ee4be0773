"""Hidden-traffic brake ladder on the CPU (DESIGN.md §5.10 "Brake ladder"): the checker tests/ref_hidden_brake_ladder.py is held to
hand cases whose results are written down, to tests/ref_hidden_brake.py level by level (the tie), to the reference's own ladder
and speed rows (tests/golden/brake_ladder.npz) and to conditions on the scenes the device test reuses; the host layer runs on CPU
tensors with a stand-in for the native call; the launch plan is built alone with the host compiler."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_ladder_scenes as LS
import hidden_brake_scenes as SC
import ref_hidden_brake as B
import ref_hidden_brake_ladder as L
import ref_hidden_reach as HR
import test_hidden_brake_cpu as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. hand cases
# The road of tests/test_hidden_brake_cpu.py: 5 x 60 cells of 1 m, hidden traffic has reached every cell from column 30 on (A = 0)
# and never reaches the others; the ego (1.8 m x 0.8 m about its reference point, heading east in row 2) touches reached road iff
# x >= 29.6.  dt = 0.5 s.
def _hand(x0, v, levels, starts=None, lens=None, A=BC.H_A):
    v = np.asarray(v, dtype=np.float64)[None]
    T = v.shape[1]
    x = x0 + np.concatenate(([0.0], np.cumsum(v[0, :-1] * BC.H_DT)))[None]
    y = np.full((1, T), 2.5)
    head = np.zeros((1, T, 2))
    head[..., 0] = 1.0
    arc = SC.travelled_arc(x, y)
    lens = None if lens is None else np.array([lens], dtype=np.int32)
    _, first, _ = HR.trajectories(A, BC.H_WIN, BC.H_ROAD, BC.H_ORIGIN, BC.H_CS, x, y, head, BC.H_HL, BC.H_HW, BC.H_WB, lens)
    nb = T if starts is None else starts
    bf, st, req, lu, cm = L.ladder(A, BC.H_WIN, BC.H_ROAD, first, BC.H_ORIGIN, BC.H_CS, x, y, head, arc, v, BC.H_HL, BC.H_HW, BC.H_WB, levels,
                                   nb, BC.H_DT, lens)
    return SimpleNamespace(first=int(first[0]), bf=bf[0], st=st[0], req=req[0].tolist(), lu=lu[0].tolist(), cm=cm[0].tolist())


def test_straight_run_towards_a_hidden_stretch():
    """8 m/s from x = 0.5 (4 m a step), the ladder 2, 3.5, 4, 8 m/s^2.  be.py's discrete profile: from b the speeds are
    vn(i) = max(8 - a (i - b) 0.5, 0), held over a step, the braking ego is at x_b + sum vn(i) 0.5.
      b = 5 (x = 20.5, 9.1 m short of 29.6): at 3.5 the steps are 4, 3.125, 2.25 -- 29.875 at sample 8, still moving (it stands at 10):
        just NOT clear; at 4 they are 4, 3, 2, 1 -- 29.5 moving, 30.5 only at its stop sample 9: just clear.  required = 2.
      b = 4 (x = 16.5): at 2 the ego is at 31.5 at sample 9 and moves; at 3.5 it comes to rest after 11.25 m, at 27.75.  required = 1.
      b <= 3: at 2 it is at 29 at the last sample: clear within the horizon.  b = 6 (x = 24.5): only 8 stops it (28.5, then 30.5 at its
      stop).  b = 7 (x = 28.5): 32.5 at the next sample whatever the level.  b >= 8: the candidate itself is in the stretch"""
    r = _hand(0.5, [8.0] * 10, [2.0, 3.5, 4.0, 8.0])
    assert r.first == 8
    assert r.req == [0, 0, 0, 0, 1, 2, 3, -1, -1, -1]
    assert r.lu == [-1, -1, -1, -1, 0, 1, 2, 3, 3, 3]
    assert r.cm == [4, 5, 6, 7]
    assert r.bf[5].tolist() == [8, 8, 9, -1] and r.st[5].tolist() == [10, 10, 9, 7]
    # level 4.0 is the existing hand case test_fast_candidate_cannot_stop of tests/test_hidden_brake_cpu.py
    assert r.bf[:, 2].tolist() == [-1, -1, -1, -1, -1, 9, 8, 8, 9, -1] and r.st[:, 2].tolist() == [4, 5, 6, 7, 8, 9, 10, 10, 10, 10]
    # fewer brake starts: the rows are cut, commit keeps what lies below B
    r = _hand(0.5, [8.0] * 10, [2.0, 3.5, 4.0, 8.0], starts=6)
    assert r.req == [0, 0, 0, 0, 1, 2] and r.lu == [-1, -1, -1, -1, 0, 1] and r.cm == [4, 5, -1, -1]


def test_level_zero_never_stops_and_a_huge_level_stands_at_once():
    """a level of 0.0: vn is v[b] for ever, stop = Lm, the braking ego is the candidate.  A huge level: vn(b) = v[b] by definition
    (the speed is held over the step that begins at b), vn(b + 1) = 0 -- the ego covers the candidate's own next step and stands
    from b + 1 on: stop = b + 1 (stop = b only where v[b] = 0), a hit at or after it is a standing ego's and does not count; so
    nothing but the candidate's own first makes the huge level unclear"""
    r = _hand(0.5, [8.0] * 10, [0.0, 1e9])
    assert r.st[:, 0].tolist() == [10] * 10 and r.bf[:, 0].tolist() == [8] * 8 + [9, -1]
    assert r.st[:, 1].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    assert r.bf[:, 1].tolist() == [-1, -1, -1, -1, -1, -1, -1, 8, 9, -1]      # b = 7: 32.5 at sample 8 = its stop
    assert r.req == [1] * 8 + [-1, -1] and r.lu == [0] * 8 + [1, 1] and r.cm == [0, 8]
    r = _hand(10.5, [0.0] * 5, [0.0, 1e9])                                    # a standing candidate stands at b at every level
    assert r.st.tolist() == [[b, b] for b in range(5)] and r.req == [0] * 5 and r.lu == [-1] * 5 and r.cm == [-1, -1]


def test_the_candidates_own_first_blocks_every_level():
    """2 m/s from x = 28.5 (1 m a step): the candidate is in the stretch from sample 2 on (x = 30.5), and no deceleration helps
    from there.  Before that: at 0.5 m/s^2 the ego still rolls into it (from b = 0: 29.5, then 30.375 at sample 2); at 8 m/s^2 and
    beyond it stands after the candidate's own next step -- from b = 0 at 29.5, from b = 1 at 30.5, reached AT its stop sample 2,
    which is a standing ego's conflict and does not count"""
    r = _hand(28.5, [2.0] * 6, [0.5, 8.0, 1e9])
    assert r.first == 2
    assert r.req == [1, 1, -1, -1, -1, -1] and r.lu == [0, 0, 2, 2, 2, 2]
    assert r.bf[0].tolist() == [2, -1, -1] and r.st[0].tolist() == [6, 1, 1]
    assert r.bf[1].tolist() == [2, 2, 2] and r.st[1].tolist() == [6, 2, 2]
    assert r.cm == [0, 2, 2]


def test_ragged_lengths_mark_no_manoeuvre():
    r = _hand(10.5, [8.0] * 6, [1.0, 4.0], lens=2)
    assert r.req == [0, 0, -1, -1, -1, -1] and r.lu == [-1] * 6
    assert r.st.tolist() == [[2, 2], [2, 2]] + [[-1, -1]] * 4 and (r.bf == -1).all() and r.cm == [-1, -1]
    r = _hand(10.5, [8.0] * 6, [1.0, 4.0], lens=0)
    assert r.req == [-1] * 6 and r.lu == [-1] * 6 and r.cm == [-1, -1]


def test_a_harder_brake_can_be_less_safe():
    """hidden traffic reaches the columns 20 and 21 at sample 4 and nothing else ever (the ego touches them iff 19.6 <= x <= 22.4).
    8 m/s from x = 10.5, brake start 0.  Without braking the ego is at 18.5 at sample 2 and at 22.5 at sample 3: it has passed.  At
    3 m/s^2 the speeds are 8, 6.5, 5, 3.5, 2, 0.5, 0: 14.5, 17.75, 20.25 (sample 3: inside, not yet reached), 22.0 at sample 4 --
    inside, reached, and moving until sample 6.  At 8 m/s^2 it stands at 16.5.  unclear = no, YES, no: the first clear level lies
    below an unclear one, which a bisection would not see"""
    A = np.full((5, 60), 255, dtype=np.uint8)
    A[:, 20:22] = 4
    r = _hand(10.5, [8.0] * 10, [0.0, 3.0, 8.0], A=A)
    assert r.first == -1
    assert r.bf[0].tolist() == [-1, 4, -1] and r.st[0].tolist() == [10, 6, 2]
    assert r.req[0] == 0 and r.lu[0] == 1 and r.req[0] < r.lu[0]
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import HiddenBrakeLadder
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32))
    hl = HiddenBrakeLadder(None, t(r.bf[None]), t(r.st[None]), t([r.cm]), t([r.req]), t([r.lu]), np.array([0.0, 3.0, 8.0]), None, 0.5)
    assert hl.monotone()[0, 0].item() is False and hl.required_deceleration()[0, 0].item() == 0.0


# ------------------------------------------------------------------------------------------------ 2. the tie, and the scenes
TIE_SCENES = [LS.CONDITION_SCENES[0] + (23, None), LS.CONDITION_SCENES[1] + (23, None), LS.CONDITION_SCENES[4] + (23, None)] + \
             [s for s in LS.SHAPE_SCENES if s[2] in (31, 33) and s[5] <= 17]


def test_checker_equals_the_brake_clearances_checker_level_by_level():
    """slice k is ref_hidden_brake.brake at a_brake = levels[k] for b < B; commit[:, k] is its commit where that is < B, else -1"""
    cut = 0
    for spec in TIE_SCENES:
        sc, A, first, ref = LS.checked(spec)
        bf, st, cm = L.from_single_calls(A, sc.win, sc.road, first, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB,
                                         sc.levels, sc.starts, sc.dt, sc.lens)
        assert np.array_equal(ref[0], bf) and np.array_equal(ref[1], st) and np.array_equal(ref[4], cm), spec
        if sc.starts < sc.T:
            full = B.brake(A, sc.win, sc.road, first, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB, float(sc.levels[0]),
                           sc.dt, sc.lens)[2]
            cut += int(((full >= sc.starts) & (ref[4][:, 0] == -1)).sum())
    assert cut > 0                                              # some commit beyond B was turned into -1


def _counts(specs):
    tot = {}
    for spec in specs:
        sc, A, first, ref = LS.checked(spec)
        bf, st, req, lu, cm = ref
        assert bf.shape == st.shape == (sc.M, sc.starts, len(sc.levels)) and req.shape == lu.shape == (sc.M, sc.starts)
        assert cm.shape == (sc.M, len(sc.levels)) and all(a.dtype == np.int32 for a in ref)
        assert ((req >= -1) & (req < len(sc.levels)) & (lu >= -1) & (lu < len(sc.levels))).all() and ((req != lu) | (req == -1)).all()
        for k, n in L.classes(req, lu, first, sc.lens, sc.T).items():
            tot[k] = tot.get(k, 0) + int(n)
    return tot


def test_condition_scenes_are_not_degenerate():
    """the six scenes on the ladder 0.5 .. 11.5 from every brake start, by the checker alone: interior answers, unblocked pairs
    without a clear level, pairs that are clear throughout and non-monotone pairs all occur (135 / 118 / 637 / 4 when this was
    written)"""
    n = _counts(LS.CONDITION_SCENES)
    print(n)
    assert n["interior"] >= 100 and n["none_clear"] >= 50 and n["all_clear"] >= 100 and n["non_monotone"] >= 1
    assert n["no_manoeuvre"] > 0 and n["blocked"] > 0


def test_shape_scenes_are_not_degenerate_and_sit_on_the_plans_edges():
    """the scenes that vary K and B: the same four kinds occur among them, every K, B and T the device test is to see is there,
    and M takes the three values around EVERY trajectories-per-workgroup edge the plan gives: 256, 128, 64, 32, 16, 8, 4, 2 and
    (M = 1 and 2) 1 -- all nine group sizes G = 1 .. 256 run on the device"""
    n = _counts(LS.SHAPE_SCENES)
    print(n)
    assert n["interior"] >= 50 and n["none_clear"] >= 20 and n["all_clear"] >= 100 and n["non_monotone"] >= 1 and n["no_manoeuvre"] > 0
    assert {s[5] for s in LS.SHAPE_SCENES} >= {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64}
    assert {s[2] for s in LS.SHAPE_SCENES} == {1, 2, 31, 33, 64, 65, 254}
    for T in (1, 2, 31, 33, 64, 65, 254):                       # B = T at every horizon, B = 1 and a middle value on the longer ones
        assert T in {s[6] for s in LS.SHAPE_SCENES if s[2] == T}, T
    assert any(s[6] == 1 < s[2] for s in LS.SHAPE_SCENES) and all(any(1 < s[6] < T for s in LS.SHAPE_SCENES if s[2] == T) for T in (31, 33, 64, 65, 254))
    families = {}
    for s in LS.SHAPE_SCENES:
        families.setdefault(s[2:3] + s[5:], set()).add(s[1])
    edges = {fam: LS.expected_plan(*fam)[2] for fam in families}
    around = {fam for fam, Ms in families.items() if {edges[fam] - 1, edges[fam], edges[fam] + 1} - {0} <= Ms}
    assert {edges[f] for f in around} == {256, 128, 64, 32, 16, 8, 4, 2, 1}, sorted(edges[f] for f in around)      # (edge 1: M = 1 and 2)
    assert {LS.expected_plan(*f)[1] for f in families} == {1, 2, 4, 8, 16, 32, 64, 128, 256}   # every G: parts of a wave, one, two, four waves
    assert any(s[4] for s in LS.SHAPE_SCENES)                   # ragged: hidden_brake_scenes.fan puts 0, 1 and 2 first


# ------------------------------------------------------------------------------------------------ 3. the reference's own ladder
def test_ladder_and_speed_rows_are_the_references():
    """tests/golden/brake_ladder.npz (written by tests/golden/gen_brake_ladder.py): the reference's unmodified
    ``BE._calc_deceleration_trajectory(traj, break_time_step=b, deceleration=[lo, hi])``.  Its deceleration vector is
    ``reference_deceleration_ladder(lo, hi)`` bit for bit, and the speed row of every level is the checker's profile (``speed``, the
    statement of ``hb_speed``) bit for bit -- at levels and speeds that are not dyadic"""
    from frenetix_occlusion.hidden_traffic import reference_deceleration_ladder
    from frenetix_occlusion import sensor_model
    assert sensor_model.reference_deceleration_ladder is reference_deceleration_ladder
    g = np.load(os.path.join(ROOT, "tests", "golden", "brake_ladder.npz"))
    dt, v = float(g["dt"]), g["v"]
    T = v.shape[1]
    sizes, stopped, moving = set(), 0, 0
    ends = np.cumsum(g["levels"])
    for i, (lo, hi, n, b) in enumerate(zip(g["case_lo"], g["case_hi"], g["case_traj"], g["case_b"])):
        decel, v_new = g["decel"][ends[i] - g["levels"][i]:ends[i]], g["v_new"][ends[i] - g["levels"][i]:ends[i]]
        mine = reference_deceleration_ladder(float(lo), float(hi))
        assert mine.dtype == np.float64 and mine.tobytes() == decel.tobytes(), (lo, hi)
        sizes.add(len(decel))
        n, b = int(n), int(b)
        for k, a in enumerate(decel.tolist()):
            vn = np.array([B.speed(float(v[n, b]), a, dt, j, b) for j in range(b, T)])
            assert vn.tobytes() == v_new[k, b:].tobytes() and np.array_equal(v_new[k, :b], v[n, :b]), (i, k)
            st = B.stop_sample(float(v[n, b]), a, dt, b, T)
            assert st == next((j for j in range(b, T) if v_new[k, j] == 0.0), T)
            stopped += st < T
            moving += st == T
    assert sizes == {1, 30, 111} and stopped > 20 and moving > 20      # (as the pin of brake_manoeuvre.npz asks)
    assert len(reference_deceleration_ladder(0.5, 11.6)) == 111 and reference_deceleration_ladder(0.0, 3.0)[3] == 3 * 0.1 != 0.3


# ------------------------------------------------------------------------------------------------ 4. the host layer
def test_derived_tables_on_a_hand_table():
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import HiddenBrakeLadder
    from frenetix_occlusion.sensor_model import HiddenBrakeLadder as exported
    assert exported is HiddenBrakeLadder
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.int32))
    #           clear at once | interior, monotone | interior, NOT monotone | no level clear | no manoeuvre
    required = [[0, 2, 1, -1, -1]]
    last_unclear = [[-1, 1, 2, 2, -1]]
    z = t(np.zeros((1, 5, 3)))
    hl = HiddenBrakeLadder(None, z, z + 1, t([[0, 1, 2]]), t(required), t(last_unclear), np.array([0.5, 4.0, 11.5]), None, 0.1)
    rd = hl.required_deceleration()
    assert rd.dtype == torch.float64 and tuple(rd.shape) == (1, 5)
    assert rd[0, :3].tolist() == [0.5, 11.5, 4.0] and rd[0, 3].item() == float("inf") and np.isnan(rd[0, 4].item())
    btn = hl.brake_threat_number(11.5)
    assert btn[0, :3].tolist() == [0.5 / 11.5, 1.0, 4.0 / 11.5] and btn[0, 3].item() == float("inf") and np.isnan(btn[0, 4].item())
    assert hl.monotone().dtype == torch.bool and hl.monotone()[0].tolist() == [True, True, False, True, True]
    bf, st, cm = hl.level(1)
    assert tuple(bf.shape) == tuple(st.shape) == (1, 5) and (st == 1).all() and cm.tolist() == [1]


def test_refusals_come_after_hidden_reachs(monkeypatch):
    torch = pytest.importorskip("torch")
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import hidden_traffic
    from frenetix_occlusion.sensor_model import SensorModel
    assert SensorModel.__dict__["hidden_brake_ladder"] is hidden_traffic.hidden_brake_ladder     # the module function itself, no wrapper
    monkeypatch.setattr(N, "current_stream", lambda index=None: None)
    z = np.zeros((2, 31))
    kw = dict(vehicle=SC.VEH, v_max=8.0, dt=0.1)
    sm = BC._cpu_model(torch)
    call = lambda sm, v=z, **k: SensorModel.hidden_brake_ladder(sm, z, z, z, v, **{**kw, **k})
    # hidden_reach's refusals first, in its words -- with v, the ladder and starts wrong as well
    with pytest.raises(ValueError, match=r"^hidden_reach: metric 'manhattan'"):
        call(sm, np.zeros((2, 30)), decelerations=[], starts=0, metric="manhattan", lengths=np.zeros(3))
    with pytest.raises(ValueError, match=r"^hidden_reach: lengths must be \[M\]$"):
        call(sm, np.zeros((2, 30)), decelerations=[], starts=0, lengths=np.zeros(3))
    none = SimpleNamespace(window=None, cell_size=SC.CS)
    with pytest.raises(RuntimeError, match=r"^hidden_reach needs the cell classes of a previous launch\(\)$"):
        call(none, decelerations=[], starts=0)
    assert sm.ctx.calls == []
    # then its own: v, the ladder, its order, starts
    with pytest.raises(ValueError, match=r"^hidden_brake_ladder: v must be \[M, T\]$"):
        call(sm, np.zeros((2, 30)), decelerations=[], starts=0)
    many = np.linspace(0.0, 13.0, 65)
    for bad in ([], None, 4.0, [1.0, -0.5], [float("nan")], [1.0, float("inf")], many, ["a"], "123", b"12", np.array([[1.0], [2.0]]),
                np.ones((1, 3)), np.float64(2.0)):
        with pytest.raises(ValueError, match=r"^hidden_brake_ladder: decelerations must hold 1 \.\. 64 finite values >= 0$"):
            call(sm, decelerations=bad, starts=0)
    for bad in ([2.0, 1.0], [1.0, 1.0], [0.5, 4.0, 4.0]):
        with pytest.raises(ValueError, match=r"^hidden_brake_ladder: decelerations must be strictly ascending"):
            call(sm, decelerations=bad, starts=0)
    for bad in (0, 32, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"^hidden_brake_ladder: starts = .*, an integer in \[1, T = 31\] or None$"):
            call(sm, decelerations=[1.0, 2.0], starts=bad)
    assert "fo_scene_hidden_brake_ladder" not in sm.ctx.calls and set(sm.ctx.calls) == {"fo_scene_hidden_reach"}
    # a good call: the forecast's entry, then the ladder's, on the forecast's own device inputs
    sm = BC._cpu_model(torch)
    x = np.cumsum(np.full((2, 31), 0.5), axis=1)
    out = SensorModel.hidden_brake_ladder(sm, x, z, z, np.full((2, 31), 5.0), decelerations=many[:64], starts=np.int64(7), metric="road",
                                          lengths=np.array([31, 7]), **kw)
    assert sm.ctx.calls == ["fo_scene_hidden_reach_road", "fo_scene_hidden_brake_ladder"]
    assert isinstance(out, hidden_traffic.HiddenBrakeLadder) and out.reach.metric == "road" and out.dt == 0.1
    assert out.decelerations.dtype == np.float64 and np.array_equal(out.decelerations, many[:64])
    assert tuple(out.brake_first.shape) == tuple(out.stop.shape) == (2, 7, 64) and tuple(out.commit.shape) == (2, 64)
    assert tuple(out.required.shape) == tuple(out.last_unclear.shape) == (2, 7)
    assert all(getattr(out, k).dtype == torch.int32 for k in ("brake_first", "stop", "commit", "required", "last_unclear"))
    assert np.array_equal(out.arc.numpy(), hidden_traffic.travelled_arc(x, z)) and out.lengths.tolist() == [31, 7]
    assert sm._hr_inputs[0].data_ptr() != 0 and sm._hbl_inputs[1] is out.arc
    out = SensorModel.hidden_brake_ladder(sm, x, z, z, np.full((2, 31), 5.0), decelerations=(3.0,), **kw)      # starts=None: T
    assert tuple(out.brake_first.shape) == (2, 31, 1)


def test_native_mirror_matches_the_header():
    from frenetix_occlusion import _native as N
    assert "fo_scene_hidden_brake_ladder" in N.EXPORTS and N.HIDDEN_BRAKE_MAX_LEVELS == 64
    names = [f[0] for f in N.HiddenBrakeLadder._fields_]
    assert names == ["base", "d_v", "d_arc", "h_levels", "K", "B", "dt", "d_brake_first", "d_stop", "d_required", "d_last_unclear", "d_commit"]
    assert N.HiddenBrakeLadder.base.size == C.sizeof(N.HiddenReach) and N.HiddenBrakeLadder.dt.size == 8
    assert N.HiddenBrakeLadder.K.size == N.HiddenBrakeLadder.B.size == 4 and N.HiddenBrakeLadder.dt.offset % 8 == 0
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        header = f.read()
    assert "#define FO_HIDDEN_BRAKE_MAX_LEVELS 64" in header
    body = header[header.index("fo_hidden_reach_t base;", header.index("BRAKE LADDER")):header.index("} fo_hidden_brake_ladder_t;")]
    order = [body.index(n) for n in ("d_v;", "d_arc;", "h_levels;", "int32_t K;", "int32_t B;", "double dt;", "*d_brake_first, *d_stop;",
                                     "*d_required, *d_last_unclear;", "d_commit;")]
    assert order == sorted(order)
    assert "int fo_scene_hidden_brake_ladder(fo_ctx *ctx, const fo_hidden_brake_ladder_t *p, void *stream);" in header


def test_interface_defaults():
    pytest.importorskip("torch")
    from frenetix_occlusion.interface import FOInterface
    seen = {}

    def hidden_brake_ladder(x, y, theta, v, **kw):
        seen.clear()
        seen.update(kw, x=x, v=v)
        return "result"
    vp = SimpleNamespace(length=4.508, width=1.61, wb_rear_axle=1.4227, mass=1093.3, a_max=11.5)
    fo = SimpleNamespace(timestep=3, sensor_model=SimpleNamespace(window=object(), hidden_brake_ladder=hidden_brake_ladder),
                         occlusion_memory={"v_max": 13.9, "margin": 0.7}, vehicle_params=vp, dt=0.1)
    traj = {k: np.full((2, 5), i, dtype=np.float64) for i, k in enumerate(("x", "y", "theta", "v", "a"))}
    assert FOInterface.hidden_brake_ladder(fo, traj) == "result"
    assert seen["decelerations"] == [0.5 * k for k in range(1, 24)] and seen["starts"] is None
    assert seen["v_max"] == 13.9 and seen["margin"] == 0.7 and seen["dt"] == 0.1
    assert seen["vehicle"] == (4.508, 1.61, 1.4227) and seen["metric"] == "euclid" and seen["flow"] == "any" and seen["inflate"] == 0.0
    assert seen["v"] is traj["v"] and seen["x"] is traj["x"]
    FOInterface.hidden_brake_ladder(fo, traj, decelerations=[1.0, 2.0], starts=3, v_max=5.0, margin=0.0, inflate=0.2, metric="road", flow="lanes")
    assert (seen["decelerations"], seen["starts"], seen["v_max"], seen["margin"], seen["inflate"], seen["metric"], seen["flow"]) == \
        ([1.0, 2.0], 3, 5.0, 0.0, 0.2, "road", "lanes")
    vp.a_max = 8.2                                              # not on the 0.5 grid: a_max itself is appended
    FOInterface.hidden_brake_ladder(fo, traj)
    assert seen["decelerations"] == [0.5 * k for k in range(1, 17)] + [8.2]
    vp.a_max = 0.3
    FOInterface.hidden_brake_ladder(fo, traj)
    assert seen["decelerations"] == [0.3]
    vp.a_max = 32.0                                             # 64 levels: the longest default ladder
    FOInterface.hidden_brake_ladder(fo, traj)
    assert len(seen["decelerations"]) == 64 and seen["decelerations"][-1] == 32.0
    for a_max in (32.2, 32.5, 1e9):
        vp.a_max = a_max
        with pytest.raises(ValueError, match=r"^hidden_brake_ladder: the default ladder .* has more than 64 levels"):
            FOInterface.hidden_brake_ladder(fo, traj)
    fo.timestep = None
    with pytest.raises(RuntimeError, match="^hidden_brake_ladder needs a previous evaluate_scenario$"):
        FOInterface.hidden_brake_ladder(fo, traj)


# ------------------------------------------------------------------------------------------------ 5. the launch plan
_PLAN_DRIVER = r"""
#include <cstdio>
#include "fo_hip.h"
#include "fo_scene_plan.hpp"
int main() {
  long long M, T, K, B;
  printf("%d %d %d %d\n", HB_THREADS, BRAKE_LADDER_MAX_LEVELS, FO_HIDDEN_BRAKE_MAX_LEVELS, BRAKE_LADDER_ROWS_BYTES);
  // every (T, K, B) a call can have: the largest LDS size, and whether the plan ever breaks one of its own rules
  size_t worst = 0;
  long long broken = 0, n = 0;
  for (int t = 1; t <= FO_HIDDEN_REACH_MAX_HALO && t <= 254; ++t)
    for (int k = 1; k <= FO_HIDDEN_BRAKE_MAX_LEVELS; ++k)
      for (int b = 1; b <= t; ++b, ++n) {
        const int Kp = brake_ladder_width(k), G = brake_ladder_group(t, k, b), per = brake_ladder_per_block(t, k, b);
        const size_t lds = brake_ladder_lds_bytes(t, k, b);
        worst = lds > worst ? lds : worst;
        broken += !(Kp >= k && Kp <= 64 && (Kp & (Kp - 1)) == 0 && G >= Kp && G <= HB_THREADS && (G & (G - 1)) == 0 && per * G == HB_THREADS &&
                    lds == (size_t)per * 48 * t + 1024 && (per == 1 || (size_t)per * 48 * t <= (size_t)BRAKE_LADDER_ROWS_BYTES));
      }
  printf("%zu %lld %lld\n", worst, broken, n);
  while (scanf("%lld %lld %lld %lld", &M, &T, &K, &B) == 4)
    printf("%d %d %d %d %zu\n", brake_ladder_width((int)K), brake_ladder_group((int)T, (int)K, (int)B), brake_ladder_per_block((int)T, (int)K, (int)B),
           brake_ladder_blocks((int)M, (int)T, (int)K, (int)B), brake_ladder_lds_bytes((int)T, (int)K, (int)B));
  return 0;
}
"""


def test_launch_plan(tmp_path):
    """the host functions of csrc/fo_scene_plan.hpp behind the launch (built alone with the host compiler) against their Python
    restatement tests/hidden_brake_ladder_scenes.expected_plan at the switch points: K around every power of two, B Kp around every
    power of two up to 256, T around every horizon at which the 32 KB of rows halve the trajectories of a workgroup (48 T per <=
    32 768: T = 2 | 3, 5 | 6, 10 | 11, 21 | 22, 42 | 43, 85 | 86, 170 | 171).  The LDS size of EVERY (T, K, B) in range is derived,
    not sampled: a workgroup with more than one trajectory keeps its rows within 32 KB, one trajectory needs 48 T <= 12 192 bytes,
    the commit rows add 1 KB -- at most 33 792 bytes, far below the 64 KB a workgroup may take; the driver walks all 2 072 640
    combinations and reports the largest size and any broken rule"""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "driver.cpp").write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "driver")
    csrc = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"), "-o", exe])
    Ts = (1, 2, 3, 5, 6, 10, 11, 21, 22, 31, 33, 42, 43, 64, 65, 85, 86, 170, 171, 254)
    Ks = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
    asked = []
    for T in Ts:
        for K in Ks:
            Kp = LS.expected_plan(T, K, 1)[0]
            Bs = {1, T, (T + 1) // 2} | {b for g in (64, 128, 256) for b in (g // Kp - 1, g // Kp, g // Kp + 1)}
            for Bn in sorted(b for b in Bs if 1 <= b <= T):
                per = LS.expected_plan(T, K, Bn)[2]
                asked += [(M, T, K, Bn) for M in sorted({0, 1, per - 1, per, per + 1, 10000, 2 ** 31 - 1} - {-1})]
    out = subprocess.run([exe], input="\n".join("%d %d %d %d" % q for q in asked) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [256, 64, 64, 32768]
    worst, broken, n = (int(v) for v in out[1].split())
    assert n == sum(64 * T for T in range(1, 255)) == 2072640 and broken == 0
    # the same maximum by the restatement, over the classes the plan distinguishes: T, Kp and min(B Kp, 256) rounded up to a power of two
    derived = max(LS.expected_plan(T, Kp, Bn)[3] for T in range(1, 255) for Kp in (1, 2, 4, 8, 16, 32, 64)
                  for Bn in sorted({min(2 ** e, T) for e in range(9)}))
    assert worst == derived == 4 * 48 * 170 + 1024 and worst <= 32768 + 1024 <= 64 * 1024
    groups = set()
    for (M, T, K, Bn), line in zip(asked, out[2:]):
        Kp, G, per, lds = LS.expected_plan(T, K, Bn)
        assert [int(v) for v in line.split()] == [Kp, G, per, -(-M // per), lds], (M, T, K, Bn)
        groups.add((G, per * 48 * T > 32768))
    assert {g for g, _ in groups} == {1, 2, 4, 8, 16, 32, 64, 128, 256} and not any(over for g, over in groups if g < 256)
    # the brake kernel's rule alone would have asked for megabytes here; the scenes of the device test sit on these edges
    assert LS.expected_plan(254, 1, 1)[1:] == (128, 2, 2 * 48 * 254 + 1024) and LS.expected_plan(31, 4, 1)[1:3] == (16, 16)
