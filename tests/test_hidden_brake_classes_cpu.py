"""Hidden-traffic brake clearance by classes on the CPU (DESIGN.md §5.10 "Brake clearance by classes"): the checker
tests/ref_hidden_brake_classes.py is held to the tie -- per class it is tests/ref_hidden_brake.py on that class's arrival map --,
to conditions that keep the scenes from being degenerate, to monotony in the speed and to hand cases whose results are written
down; the host layer runs on CPU tensors, the ctypes mirror and the launch plan are held to the header and to csrc by a host
compiler.  Every comparison is between integers and exact."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_classes_scenes as CS
import hidden_brake_scenes as SC
import ref_hidden_brake as B
import ref_hidden_brake_classes as BCL
import ref_hidden_clearance as HC
import ref_hidden_reach as HR
import test_hidden_brake_cpu as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = [spec for spec in SC.RANDOM_SCENES if spec[2] >= 31]
_cache = {}


def solved(spec):
    """the scene of ``spec`` with the classes checker's outputs and, per class, ref_hidden_brake's on that class's arrival map --
    computed once, shared by the tests below, never changed"""
    if spec not in _cache:
        sc = CS.class_scene(spec)
        got = BCL.brake_classes(sc.key, sc.win, sc.road, sc.qmin, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB,
                                sc.a_brake, sc.dt, sc.thr, sc.lens)
        per_class = []
        for table in sc.tables:
            sc.r2 = table
            A, _, first = SC.arrival_and_first(sc)
            per_class.append(B.brake(A, sc.win, sc.road, first, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB,
                                     sc.a_brake, sc.dt, sc.lens) + (first,))
        _cache[spec] = (sc, got, per_class)
    return _cache[spec]


# ------------------------------------------------------------------------------------------------ 1. the tie on the checkers
def test_speeds_of_the_scenes():
    assert CS.speeds_for(31) == (1.5, 4.0, 8.0) and CS.speeds_for(1) == (1.5, 4.0, 8.0)
    s = CS.speeds_for(254)
    assert s[2] == 24.0 / 25.3 and s[0] < s[1] < s[2]
    assert {spec[3] for spec in LONG} == {0, 1, 2} and len(LONG) == 18


@pytest.mark.parametrize("spec", LONG, ids=lambda s: "-".join(str(v) for v in s))
def test_checker_equals_the_brake_checker_per_class(spec):
    """the scenes of tests/hidden_brake_scenes.RANDOM_SCENES with T >= 31 -- between them all three forecasts -- with the speeds
    (1.5, 4.0, 8.0): row c of every output is ref_hidden_brake.brake on the arrival map of class c, first the forecast's own"""
    sc, (bf, st, commit, first), per_class = solved(spec)
    assert bf.shape == (3, sc.M, sc.T) and st.shape == (sc.M, sc.T) and commit.shape == first.shape == (3, sc.M)
    assert all(a.dtype == np.int32 for a in (bf, st, commit, first))
    for c, (bf_c, st_c, commit_c, first_c) in enumerate(per_class):
        assert np.array_equal(bf[c], bf_c), (c, np.argwhere(bf[c] != bf_c)[:4].tolist())
        assert np.array_equal(st, st_c), c
        assert np.array_equal(commit[c], commit_c), (c, np.argwhere(commit[c] != commit_c)[:4].tolist())
        assert np.array_equal(first[c], first_c), c
        assert np.array_equal(first[c], HC.reach_from_qmin(sc.qmin, sc.tables[c])[1]), c


def test_scenes_are_not_degenerate():
    """by the checker alone: in scene (35, 70, 31, road, ragged) commit differs between the slowest and the fastest class for at
    least 20 candidates, and at least 10 are fail-safe against the slowest class and not against the fastest (28 and 18 when the
    scenes were written); over the first nine scenes some candidate of every kind is there"""
    _, (_, _, commit, _), _ = solved((35, 70, 31, 1, True))
    differ, safe_slow = int((commit[0] != commit[2]).sum()), int(((commit[0] == -1) & (commit[2] >= 0)).sum())
    print("scene 35:", differ, safe_slow)
    assert differ >= 20 and safe_slow >= 10
    total = [0, 0]
    for spec in LONG[:9]:
        commit = solved(spec)[1][2]
        total[0] += int((commit[0] != commit[2]).sum())
        total[1] += int(((commit[0] == -1) & (commit[2] >= 0)).sum())
    print("first nine scenes:", total)
    assert total[0] >= 20 and total[1] >= 10


@pytest.mark.parametrize("spec", LONG[:9], ids=lambda s: "-".join(str(v) for v in s))
def test_monotone_in_the_speed(spec):
    """for v_a <= v_b: commit_a >= 0 implies 0 <= commit_b <= commit_a, and where both brake_first are >= 0 the faster class is hit
    no later (a faster road user reaches every cell no later: thr_a <= thr_b entry by entry)"""
    sc, (bf, _, commit, first), _ = solved(spec)
    assert (sc.thr[:-1] <= sc.thr[1:]).all()
    for a in range(2):
        b = a + 1
        lost = commit[a] >= 0
        assert ((commit[b][lost] >= 0) & (commit[b][lost] <= commit[a][lost])).all()
        both = (bf[a] >= 0) & (bf[b] >= 0)
        assert (bf[b][both] <= bf[a][both]).all()
        assert ((bf[a] < 0) | (bf[b] >= 0)).all()
        assert ((first[a] < 0) | ((first[b] >= 0) & (first[b] <= first[a]))).all()


# ------------------------------------------------------------------------------------------------ 2. hand cases
# A road of 5 x 60 cells of 1 m, all of it inside the window and seen, but for the stretch from column 40 on, which is hidden.  No
# margin, dt = 0.5 s: a road user of up to v m/s may be D cells in front of the stretch at sample j iff D <= 0.5 v j, and the cell of
# column 40 - D has the key 169 D^2.  The ego is a box of 1.8 m x 0.8 m about its reference point (wb = 0) in row 2, heading east: at
# x = k + 0.5 it holds exactly the cell of column k.
H_ORIGIN, H_CS, H_DT = (0.0, 0.0), 1.0, 0.5
H_ROAD = np.ones((5, 60), dtype=np.uint8)
H_WIN = (0, 0, 60, 5)
H_CLS = np.full((5, 60), 3, dtype=np.uint8)
H_CLS[:, 40:] = 5
H_HL, H_HW, H_WB = 0.9, 0.4, 0.0


def _hand(x0, v, a_brake, speeds, lens=None):
    """one trajectory along the road from x0 with the speeds v (held over a step) against the classes ``speeds``; r2_cap is the end of
    the fastest table exactly.  Returns (first [C], brake_first [C][T], stop [T], commit [C]) as lists"""
    v = np.asarray(v, dtype=np.float64)[None]
    T = v.shape[1]
    x = x0 + np.concatenate(([0.0], np.cumsum(v[0, :-1] * H_DT)))[None]
    y = np.full((1, T), 2.5)
    head = np.zeros((1, T, 2))
    head[..., 0] = 1.0
    arc = SC.travelled_arc(x, y)
    lens = None if lens is None else np.array([lens], dtype=np.int32)
    tables = CS.reach_tables(speeds, T, H_DT, 0.0, H_CS)
    thr = CS.thresholds(tables)
    r2_cap = max(int(t[-1]) for t in tables)
    assert thr.max() == 169 * r2_cap                             # the fastest table ends exactly at the cap
    key = HC.key_map(H_CLS, H_WIN, H_ROAD, r2_cap)[0]
    qmin = HC.clearance(key, H_WIN, H_ROAD, H_ORIGIN, H_CS, x, y, head, H_HL, H_HW, H_WB, lens)
    bf, st, commit, first = BCL.brake_classes(key, H_WIN, H_ROAD, qmin, H_ORIGIN, H_CS, x, y, head, arc, v, H_HL, H_HW, H_WB, a_brake, H_DT,
                                              thr, lens)
    for c, table in enumerate(tables):                           # the tie, on the hand case too
        A = HR.arrival_map(H_CLS, H_WIN, H_ROAD, table)[0]
        _, f, _ = HR.trajectories(A, H_WIN, H_ROAD, H_ORIGIN, H_CS, x, y, head, H_HL, H_HW, H_WB, lens)
        ref = B.brake(A, H_WIN, H_ROAD, f, H_ORIGIN, H_CS, x, y, head, arc, v, H_HL, H_HW, H_WB, a_brake, H_DT, lens)
        assert np.array_equal(bf[c], ref[0]) and np.array_equal(st, ref[1]) and np.array_equal(commit[c], ref[2]) and first[c, 0] == f[0]
    return first[:, 0].tolist(), bf[:, 0].tolist(), st[0].tolist(), commit[:, 0].tolist()


def test_key_of_the_hand_road():
    key = HC.key_map(H_CLS, H_WIN, H_ROAD, 36 * 36)[0]
    assert key[2, 40:].tolist() == [0] * 20 and key[2, 4:40].tolist() == [169 * (40 - k) ** 2 for k in range(4, 40)]
    assert (key[:, :4] == HC.NONE).all()                         # farther than the cap of 36 cells


def test_fast_medium_and_slow_class_by_hand():
    """8 m/s from x = 0.5 (4 m a step: column 4 k at sample k), braking at 4 m/s^2: 4, 7, 9 m beyond x_b while it moves, standing 10 m
    beyond it from sample b + 4.
    8 m/s hidden (4 cells a sample): the candidate is met when 40 - 4 k <= 4 k, first = 5.  From b = 2 the ego stands in column 18 at
    sample 6 and is met there at that very sample (22 <= 24): at its stop, not counted.  From b = 3 it is in column 21 at sample 6,
    still moving (19 <= 24): commit = 3.
    4 m/s hidden (2 cells a sample): first = 7 (12 <= 14).  From b = 4 it stands in column 26 from sample 8 and is met there at 8
    (14 <= 16): not counted.  From b = 5 it is in column 27 at sample 7, moving (13 <= 14): commit = 5.
    0.5 m/s hidden: 2.25 cells within the horizon, the candidate ends 4 cells short: nothing"""
    first, bf, st, commit = _hand(0.5, [8.0] * 10, 4.0, (8.0, 4.0, 0.5))
    assert st == [4, 5, 6, 7, 8, 9, 10, 10, 10, 10]
    assert first == [5, 7, -1] and commit == [3, 5, -1]
    assert bf[0] == [8, 7, 6, 6, 5, 6, 7, 8, 9, -1]
    assert bf[1] == [-1, -1, -1, 9, 8, 7, 7, 8, 9, -1]
    assert bf[2] == [-1] * 10


def test_equal_unsorted_and_zero_speeds():
    """the rows come in the order of the speeds given, equal speeds give equal rows, and a hidden road user that does not move (v = 0,
    no margin) is met only inside the hidden stretch itself"""
    first, bf, st, commit = _hand(0.5, [8.0] * 10, 4.0, (4.0, 8.0, 0.0, 4.0, 0.5))
    assert first == [7, 5, -1, 7, -1] and commit == [5, 3, -1, 5, -1]
    assert bf[0] == bf[3] == [-1, -1, -1, 9, 8, 7, 7, 8, 9, -1] and bf[1] == [8, 7, 6, 6, 5, 6, 7, 8, 9, -1]
    assert bf[2] == bf[4] == [-1] * 10
    # from x = 33.5 at 4 m/s (2 m a step: columns 33, 35, 37, 39, 41, 43), braking at 8 m/s^2: it stands at b + 1, one step on.
    # v = 0 meets the candidate in column 41 at sample 4; the manoeuvre from b = 3 stands exactly there from its stop sample on: not
    # counted, commit is first's.  2 m/s (one cell a sample) meets the candidate in column 39 at sample 3 (1 <= 3); the manoeuvres from
    # b = 0, 1, 2 stand in columns 35, 37, 39 and are met at samples 5, 3, 3 -- all standing
    first, bf, st, commit = _hand(33.5, [4.0] * 6, 8.0, (0.0, 2.0))
    assert st == [1, 2, 3, 4, 5, 6]
    assert first == [4, 3] and commit == [4, 3]
    assert bf[0] == [-1, -1, -1, 4, 5, -1] and bf[1][:3] == [5, 3, 3]
    # a candidate that stands inside the stretch: every class, the motionless one included, has it now
    first, bf, st, commit = _hand(41.5, [0.0] * 4, 3.0, (0.0, 8.0))
    assert first == [0, 0] and commit == [0, 0] and st == [0, 1, 2, 3] and bf[0] == bf[1] == [1, 2, 3, -1]


def test_ragged_lengths_by_hand():
    speeds = (8.0, 0.5)
    v = [8.0] * 6
    assert _hand(41.5, v, 4.0, speeds, lens=0) == ([-1, -1], [[-1] * 6] * 2, [-1] * 6, [-1, -1])
    assert _hand(41.5, v, 4.0, speeds, lens=1) == ([0, 0], [[-1] * 6] * 2, [1] + [-1] * 5, [0, 0])
    # two samples from x = 36.5: sample 0 is 4 cells short for either class, the one pose (sample 1, x = 40.5) lies inside the stretch
    first, bf, st, commit = _hand(36.5, v, 4.0, speeds, lens=2)
    assert bf == [[1, -1, -1, -1, -1, -1]] * 2 and st == [2, 2, -1, -1, -1, -1] and first == [1, 1] and commit == [0, 0]


# ------------------------------------------------------------------------------------------------ 3. the host layer
def test_thresholds_are_169_times_the_reach_tables():
    pytest.importorskip("torch")
    from frenetix_occlusion import sensor_model
    from frenetix_occlusion.hidden_traffic import hidden_brake_thresholds, hidden_reach_r2
    assert sensor_model.hidden_brake_thresholds is hidden_brake_thresholds
    speeds = (8.0, 0.0, 1.5, 13.9)
    thr = hidden_brake_thresholds(speeds, 0.1, 0.7, 0.5, 31)
    assert isinstance(thr, np.ndarray) and thr.dtype == np.int32 and thr.shape == (4, 31) and thr.flags["C_CONTIGUOUS"]
    for c, v in enumerate(speeds):
        assert np.array_equal(thr[c].astype(np.int64), 169 * hidden_reach_r2(v, 0.1, 0.7, 0.5, 31).astype(np.int64))
        assert np.array_equal(thr[c].astype(np.int64), 169 * HR.reach_table(v, 0.1, 0.7, 0.5, 31))
    assert (np.diff(thr.astype(np.int64), axis=1) >= 0).all() and (thr >= 0).all()
    assert hidden_brake_thresholds((2.0,), 0.1, 0.0, 0.5, 1).tolist() == [[0]]


def test_critical_speed_and_decided_until():
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import HiddenBrake, HiddenBrakeClasses
    from frenetix_occlusion.sensor_model import HiddenBrakeClasses as exported
    assert exported is HiddenBrakeClasses
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.int32))
    stop = [[2, 3, 4, 5, 5, 5], [3, 4, 5, 6, 6, 6], [6] * 6, [2, 3, 4, 4, -1, -1], [-1] * 6]
    lengths = t([6, 6, 9, 4, -2])
    commit = [[-1, 3, -1, 0, -1], [-1, 2, 5, 0, -1], [-1, 0, -1, 0, -1]]       # speeds in the order given: 4, 1.5, 8
    bf = torch.zeros((3, 5, 6), dtype=torch.int32)
    out = HiddenBrakeClasses(None, (4.0, 1.5, 8.0), np.zeros((3, 6), dtype=np.int32), bf, t(stop), t(commit), t(commit), None, 4.0, 0.1, lengths)
    vc = out.critical_speed()
    assert vc.dtype == torch.float64 and vc.tolist() == [float("inf"), 1.5, 1.5, 1.5, float("inf")]
    assert out.decided_until().tolist() == HiddenBrake(None, bf[0], t(stop), t(commit[0]), None, 4.0, 0.1, lengths).decided_until().tolist() \
        == [6, 3, 0, 2, 0]
    one = HiddenBrakeClasses(None, (7.0,), np.zeros((1, 6), dtype=np.int32), bf[:1], t(stop), t(commit[:1]), t(commit[:1]), None, 4.0, 0.1)
    assert one.critical_speed().tolist() == [float("inf"), 7.0, float("inf"), 7.0, float("inf")]
    assert one.decided_until().tolist() == [6, 3, 0, 6, 6]       # no lengths: Lm = T, only the rows whose stop reaches 6 are open


def test_refusals_in_their_order(monkeypatch):
    torch = pytest.importorskip("torch")
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import hidden_traffic
    from frenetix_occlusion.sensor_model import SensorModel
    assert SensorModel.__dict__["hidden_brake_classes"] is hidden_traffic.hidden_brake_classes
    assert (N.HIDDEN_BRAKE_MAX_CLASSES, N.HIDDEN_BRAKE_MAX_TABLE) == (8, 896)
    monkeypatch.setattr(N, "current_stream", lambda index=None: None)
    z = np.zeros((2, 31))
    kw = dict(vehicle=SC.VEH, dt=0.1)
    sm = BC._cpu_model(torch)
    bad_v = np.zeros((2, 30))
    # its own refusals first, before the model is looked at: the speeds, then the size of the table -- with everything else wrong too
    none = SimpleNamespace(window=None, cell_size=SC.CS)
    for speeds in ((), (1.0,) * 9, (1.0, -0.5), (float("nan"),), (1.0, float("inf")), None):
        with pytest.raises(ValueError, match=r"^hidden_brake_classes: speeds must hold 1 \.\. 8 finite values >= 0$"):
            SensorModel.hidden_brake_classes(none, z, z, z, bad_v, speeds=speeds, a_brake=-1.0, metric="manhattan", **kw)
    long = np.zeros((2, 113))
    with pytest.raises(ValueError, match=r"^hidden_brake_classes: 8 speeds x 113 samples = 904 thresholds, at most 896 are possible"):
        SensorModel.hidden_brake_classes(none, long, long, long, bad_v, speeds=(1.0,) * 8, a_brake=-1.0, metric="manhattan", **kw)
    # then the clearance's, in its words
    with pytest.raises(ValueError, match=r"^hidden_clearance: metric 'manhattan'"):
        SensorModel.hidden_brake_classes(sm, z, z, z, bad_v, speeds=(1.0, 2.0), a_brake=-1.0, metric="manhattan", **kw)
    with pytest.raises(RuntimeError, match=r"^hidden_clearance needs the cell classes of a previous launch\(\)$"):
        SensorModel.hidden_brake_classes(none, z, z, z, bad_v, speeds=(1.0, 2.0), a_brake=-1.0, **kw)
    with pytest.raises(ValueError, match=r"^hidden_clearance: lengths must be \[M\]$"):
        SensorModel.hidden_brake_classes(sm, z, z, z, bad_v, speeds=(1.0, 2.0), a_brake=-1.0, lengths=np.zeros(3), **kw)
    assert sm.ctx.calls == []
    # then v before a_brake, after the clearance ran
    with pytest.raises(ValueError, match=r"^hidden_brake_classes: v must be \[M, T\]$"):
        SensorModel.hidden_brake_classes(sm, z, z, z, bad_v, speeds=(1.0, 2.0), a_brake=-1.0, **kw)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^hidden_brake_classes: a_brake >= 0 and finite$"):
            SensorModel.hidden_brake_classes(sm, z, z, z, z, speeds=(1.0, 2.0), a_brake=bad, **kw)
    assert "fo_scene_hidden_brake_classes" not in sm.ctx.calls and set(sm.ctx.calls) == {"fo_scene_hidden_clearance"}
    # a good call: the clearance at the fastest speed, then the one entry, on the clearance's own device inputs; 8 x 112 is accepted
    sm = BC._cpu_model(torch)
    x = np.cumsum(np.full((2, 112), 0.05), axis=1)
    z = np.zeros((2, 112))
    speeds = (4.0, 0.5, 2.0, 0.0, 1.0, 1.0, 3.0, 0.25)
    out = SensorModel.hidden_brake_classes(sm, x, z, z, np.full((2, 112), 0.5), speeds=speeds, a_brake=0.0, metric="road",
                                           lengths=np.array([112, 7]), **kw)
    assert sm.ctx.calls == ["fo_scene_hidden_clearance", "fo_scene_hidden_brake_classes"]
    assert isinstance(out, hidden_traffic.HiddenBrakeClasses) and out.speeds == speeds and (out.a_brake, out.dt) == (0.0, 0.1)
    assert out.clearance.metric == "road" and out.clearance.r2_cap == int(hidden_traffic.hidden_reach_r2(4.0, 0.1, out.clearance.margin, SC.CS, 112)[-1])
    assert np.array_equal(out.thr, hidden_traffic.hidden_brake_thresholds(speeds, 0.1, out.clearance.margin, SC.CS, 112))
    assert int(out.thr.max()) == 169 * out.clearance.r2_cap
    assert tuple(out.brake_first.shape) == (8, 2, 112) and tuple(out.stop.shape) == (2, 112)
    assert tuple(out.commit.shape) == tuple(out.first.shape) == (8, 2)
    assert out.brake_first.dtype == out.stop.dtype == out.commit.dtype == out.first.dtype == torch.int32
    assert np.array_equal(out.arc.numpy(), hidden_traffic.travelled_arc(x, z)) and out.lengths.tolist() == [112, 7]
    assert sm._hc_inputs[0].data_ptr() != 0 and sm._hbc_inputs[1] is out.arc
    # flow="lanes" goes to the flow clearance; heading= is handed on
    sm = BC._cpu_model(torch)
    sm.lane_moves = object()
    out2 = SensorModel.hidden_brake_classes(sm, x, z, None, z, speeds=(1.0,), a_brake=2.0, metric="road", flow="lanes", heading=out.clearance.heading, **kw)
    assert sm.ctx.calls == ["fo_scene_hidden_clearance_flow", "fo_scene_hidden_brake_classes"] and out2.clearance.flow == "lanes"


def test_interface_defaults():
    pytest.importorskip("torch")
    import inspect
    from frenetix_occlusion.interface import FOInterface
    from frenetix_occlusion.sensor_model import SensorModel
    assert list(inspect.signature(FOInterface.hidden_brake_classes).parameters) == \
        ["self", "trajectories", "speeds", "a_brake", "margin", "inflate", "metric", "flow"]
    sig = inspect.signature(SensorModel.hidden_brake_classes)
    assert list(sig.parameters) == ["self", "x", "y", "theta", "v", "vehicle", "speeds", "dt", "a_brake", "margin", "inflate", "lengths",
                                    "metric", "flow", "heading"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[5:])
    seen = {}

    def hidden_brake_classes(x, y, theta, v, **kw):
        seen.update(kw, x=x, v=v)
        return "result"
    vp = SimpleNamespace(length=4.508, width=1.61, wb_rear_axle=1.4227, mass=1093.3, a_max=11.5)
    fo = SimpleNamespace(timestep=3, sensor_model=SimpleNamespace(window=object(), hidden_brake_classes=hidden_brake_classes),
                         occlusion_memory={"v_max": 13.9, "margin": 0.7}, vehicle_params=vp, dt=0.1)
    traj = {k: np.full((2, 5), i, dtype=np.float64) for i, k in enumerate(("x", "y", "theta", "v", "a"))}
    assert FOInterface.hidden_brake_classes(fo, traj, (2.0, 7.0)) == "result"
    assert seen["a_brake"] == 11.5 and seen["speeds"] == (2.0, 7.0) and seen["margin"] == 0.7 and seen["dt"] == 0.1
    assert seen["vehicle"] == (4.508, 1.61, 1.4227) and seen["metric"] == "euclid" and seen["flow"] == "any" and seen["inflate"] == 0.0
    assert seen["v"] is traj["v"] and seen["x"] is traj["x"] and "v_max" not in seen
    FOInterface.hidden_brake_classes(fo, traj, [13.9], a_brake=4.0, margin=0.0, inflate=0.2, metric="road", flow="lanes")
    assert (seen["a_brake"], seen["speeds"], seen["margin"], seen["inflate"], seen["metric"], seen["flow"]) == (4.0, [13.9], 0.0, 0.2, "road", "lanes")
    fo.timestep = None
    with pytest.raises(RuntimeError, match="^hidden_brake_classes needs a previous evaluate_scenario$"):
        FOInterface.hidden_brake_classes(fo, traj, (2.0,))


# ------------------------------------------------------------------------------------------------ 4. the C side, by a host compiler
def _cc(names):
    return next((c for c in names if shutil.which(c)), None)


def test_native_mirror_has_the_layout_of_the_header(tmp_path):
    """size and the offset of every member of fo_hidden_brake_classes_t against what a C compiler makes of include/fo_hip.h; the two
    constants; the entry is declared and exported"""
    from frenetix_occlusion import _native as N
    cc = _cc(("gcc", "cc", "clang"))
    if cc is None:
        pytest.skip("no host C compiler")
    fields = [n for n, *_ in N.HiddenBrakeClasses._fields_]
    assert fields == ["M", "T", "d_x", "d_y", "d_heading", "d_len_or_null", "hl", "hw", "wb", "win_ix0", "win_iy0", "win_nx", "win_ny",
                      "r2_cap", "C", "d_key", "d_qmin", "d_v", "d_arc", "a_brake", "dt", "h_thr", "d_brake_first", "d_stop", "d_commit",
                      "d_first"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fo_hip.h"', 'int main(void) {',
             'printf("%zu %d %d\\n", sizeof(fo_hidden_brake_classes_t), FO_HIDDEN_BRAKE_MAX_CLASSES, FO_HIDDEN_BRAKE_MAX_TABLE);']
    lines += ['printf("%%zu\\n", offsetof(fo_hidden_brake_classes_t, %s));' % f for f in fields]
    lines += ['return 0; }']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", str(tmp_path / "layout.c"), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:3] == [C.sizeof(N.HiddenBrakeClasses), N.HIDDEN_BRAKE_MAX_CLASSES, N.HIDDEN_BRAKE_MAX_TABLE]
    assert out[3:] == [getattr(N.HiddenBrakeClasses, f).offset for f in fields]
    assert "fo_scene_hidden_brake_classes" in N.EXPORTS
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        assert "int fo_scene_hidden_brake_classes(fo_ctx *ctx, const fo_hidden_brake_classes_t *p, void *stream);" in f.read()


_PLAN_DRIVER = r"""
#include <cstdio>
#include "fo_hip.h"
#include "fo_scene_plan.hpp"
int main() {
  long long M, T, C;
  while (scanf("%lld %lld %lld", &M, &T, &C) == 3)
    printf("%d %d %zu %zu\n", brake_classes_width((int)C), brake_classes_blocks((int)M, (int)T), brake_classes_lds_bytes((int)T, (int)C),
           brake_lds_bytes((int)T));
  return 0;
}
"""


def test_launch_plan(tmp_path):
    """the host functions of csrc/fo_scene_plan.hpp behind the launch, built alone with the host compiler: the grid of the brake
    kernel, its six rows plus one int32 row per trajectory plus the table in LDS -- never more than 64 KB --, the compile-time class
    count the power of two >= C"""
    cxx = _cc(("g++", "c++", "clang++"))
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "driver.cpp").write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "driver")
    csrc = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"), "-o", exe])
    asked = [(M, T, C) for T in (1, 2, 3, 31, 32, 33, 64, 65, 112, 128, 254) for C in range(1, 9) if C * T <= 896
             for M in (1, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257, 10000, 2 ** 31 - 1)]
    assert (1, 112, 8) in asked and (1, 128, 7) in asked and (1, 254, 3) in asked and (1, 254, 4) not in asked
    out = subprocess.run([exe], input="\n".join("%d %d %d" % a for a in asked) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    worst = 0
    for (M, T, C), line in zip(asked, out):
        G = 1
        while G < min(T, 64):
            G *= 2
        per = 256 // G
        width = next(w for w in (1, 2, 4, 8) if w >= C)
        lds = per * T * (6 * 8 + 4) + C * T * 4
        assert [int(v) for v in line.split()] == [width, -(-M // per), lds, per * 6 * T * 8], (M, T, C)
        worst = max(worst, lds)
    assert worst == 4 * 254 * 52 + 3 * 254 * 4 and worst <= 64 * 1024
