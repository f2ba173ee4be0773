"""Hidden-traffic brake clearance on the CPU (DESIGN.md §5.10 "Brake clearance"): the checker tests/ref_hidden_brake.py is held
to hand cases whose results are written down, to the shipped forecast (with no deceleration and exact arithmetic the braking ego
is the candidate itself), to the reference's own ``BE._calc_deceleration_trajectory`` (tests/golden/brake_manoeuvre.npz) and to
conditions on the random scenes the device test reuses; the host layer runs on CPU tensors."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_scenes as SC
import ref_hidden_brake as B
import ref_hidden_reach as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. hand cases
# A road of 5 x 60 cells of 1 m, all of it inside the window; hidden traffic has reached every cell from column 30 on (A = 0) and
# never reaches the others (A = 255).  The ego is a box of 1.8 m x 0.8 m about its reference point (wb = 0) in row 2, heading east:
# it holds the cell centres within 0.9 m of x, so it touches reached road iff x + 0.9 >= 30.5, i.e. x >= 29.6.  dt = 0.5 s.
H_ORIGIN, H_CS, H_DT = (0.0, 0.0), 1.0, 0.5
H_ROAD = np.ones((5, 60), dtype=np.uint8)
H_WIN = (0, 0, 60, 5)
H_A = np.full((5, 60), 255, dtype=np.uint8)
H_A[:, 30:] = 0
H_HL, H_HW, H_WB = 0.9, 0.4, 0.0


def _hand(x0, v, a_brake, lens=None, A=H_A):
    """one trajectory along the road from x0 with the speeds v (held over a step): the checker's rows and the forecast's first"""
    v = np.asarray(v, dtype=np.float64)[None]
    T = v.shape[1]
    x = x0 + np.concatenate(([0.0], np.cumsum(v[0, :-1] * H_DT)))[None]
    y = np.full((1, T), 2.5)
    head = np.zeros((1, T, 2))
    head[..., 0] = 1.0
    arc = SC.travelled_arc(x, y)
    lens = None if lens is None else np.array([lens], dtype=np.int32)
    _, first, _ = HR.trajectories(A, H_WIN, H_ROAD, H_ORIGIN, H_CS, x, y, head, H_HL, H_HW, H_WB, lens)
    bf, st, commit = B.brake(A, H_WIN, H_ROAD, first, H_ORIGIN, H_CS, x, y, head, arc, v, H_HL, H_HW, H_WB, a_brake, H_DT, lens)
    return int(first[0]), bf[0].tolist(), st[0].tolist(), int(commit[0])


def test_slow_candidate_stops_short():
    """2 m/s from x = 10.5: at 17.5 after 8 samples, far from the hidden stretch; at 2 m/s^2 it stands two samples after b"""
    first, bf, st, commit = _hand(10.5, [2.0] * 8, 2.0)
    assert first == -1 and bf == [-1] * 8 and commit == -1
    assert st == [2, 3, 4, 5, 6, 7, 8, 8]                       # (8 = not within the horizon)


def test_fast_candidate_cannot_stop():
    """8 m/s from x = 0.5 (4 m a step), 4 m/s^2: the speeds after b are 8, 6, 4, 2, 0, so the braking ego is 4, 7, 9 m beyond x_b
    while it moves and stands 10 m beyond it from sample b + 4.  Its own first hit is sample 8 (x = 32.5).  From b = 5 (x = 20.5) it
    reaches 29.5 moving and 30.5 only standing, at its stop sample 9: that does not count.  From b = 6 (x = 24.5) it is at 31.5 at
    sample 8, still moving: commit = 6"""
    first, bf, st, commit = _hand(0.5, [8.0] * 10, 4.0)
    assert first == 8
    assert st == [4, 5, 6, 7, 8, 9, 10, 10, 10, 10]
    assert bf == [-1, -1, -1, -1, -1, 9, 8, 8, 9, -1]
    assert commit == 6


def test_the_candidates_own_first_decides():
    """2 m/s from x = 28.5, 8 m/s^2: every manoeuvre stands at b + 1 on the candidate's own next sample, so no moving ego ever meets
    reached road; the candidate itself does at sample 2 (x = 30.5)"""
    first, bf, st, commit = _hand(28.5, [2.0] * 6, 8.0)
    assert first == 2 and st == [1, 2, 3, 4, 5, 6]
    assert bf == [-1, 2, 3, 4, 5, -1]                           # from b = 0 it stands at 29.5: clear; later ones are hit AT their stop
    assert commit == 2


def test_standing_start():
    """a candidate that stands: clear of the stretch it is fail-safe for ever, inside it commit = 0; every arc entry is 0, so every
    pose is a repeated sample (xhi == xlo) and takes sample idx - 1 = 0"""
    first, bf, st, commit = _hand(10.5, [0.0] * 5, 3.0)
    assert (first, bf, st, commit) == (-1, [-1] * 5, [0, 1, 2, 3, 4], -1)
    first, bf, st, commit = _hand(31.5, [0.0] * 5, 3.0)
    assert (first, st, commit) == (0, [0, 1, 2, 3, 4], 0)
    assert bf == [1, 2, 3, 4, -1]                               # the standing ego is hit, strictly after its stop: not counted


def test_no_deceleration_is_the_candidate_itself():
    first, bf, st, commit = _hand(0.5, [8.0] * 10, 0.0)
    assert first == 8 and st == [10] * 10
    assert bf == [8] * 8 + [9, -1]
    assert commit == 0                                          # whenever it "brakes" it still drives into the stretch


def test_repeated_samples():
    """three samples at rest at x = 20.5, then 4 m/s (2 m a step): arc = 0, 0, 0, 0, 2, 4, 6, 8, 10, 12.  From b = 0 .. 2 the speed
    is 0: the pose is sample 0 (the segment with xhi == xlo).  From b = 3 at 2 m/s^2 the speeds are 4, 3, 2, 1, 0: 2, 3.5, 4.5, 5 m
    beyond 20.5, standing from sample 7 at 25.5.  From b = 7 (x = 28.5): 30.5 at sample 8, moving"""
    first, bf, st, commit = _hand(20.5, [0.0] * 3 + [4.0] * 7, 2.0)
    assert first == 8                                           # x_8 = 30.5
    assert st == [0, 1, 2, 7, 8, 9, 10, 10, 10, 10]
    # b = 4 (22.5): 24.5, 26, 27, 27.5 -- clear; b = 5 (24.5): 26.5, 28, 29 (+ 29.5 standing) -- clear; b = 6 (26.5): 28.5, 30 at 8
    assert bf == [-1, -1, -1, -1, -1, -1, 8, 8, 9, -1]
    assert commit == 6


def test_ragged_lengths_of_0_1_and_2():
    v = [8.0] * 6
    assert _hand(31.5, v, 4.0, lens=0) == (-1, [-1] * 6, [-1] * 6, -1)
    assert _hand(31.5, v, 4.0, lens=1) == (0, [-1] * 6, [1] + [-1] * 5, 0)        # its own first; no pose; moving at the end
    assert _hand(10.5, v, 4.0, lens=1) == (-1, [-1] * 6, [1] + [-1] * 5, -1)
    # two samples: one pose, the segment index clamped to 1 = Lm - 1; from x = 26.5 the pose at sample 1 is 30.5
    assert _hand(26.5, v, 4.0, lens=2) == (1, [1, -1, -1, -1, -1, -1], [2, 2, -1, -1, -1, -1], 0)
    assert _hand(10.5, v, 4.0, lens=2) == (-1, [-1] * 6, [2, 2, -1, -1, -1, -1], -1)
    assert _hand(26.5, [0.0] * 6, 4.0, lens=2) == (-1, [-1] * 6, [0, 1, -1, -1, -1, -1], -1)


def test_clamp_at_the_end_of_the_path():
    """a candidate that drives 8 m in two steps and then stands at x = 28.5 (arc ends at 8): kept at 8 m/s (a_brake = 0) from b = 0
    it would be 12, 16, .. m along -- beyond its path; the manoeuvre is clamped to the path's end, so it never gets nearer than
    28.5 and never touches the stretch.  One metre farther on (29.6 <= 29.5 + ...) the end of the path itself is inside"""
    first, bf, st, commit = _hand(20.5, [8.0, 8.0, 0.0, 0.0, 0.0, 0.0], 0.0)
    assert first == -1 and st == [6, 6, 2, 3, 4, 5] and bf == [-1] * 6 and commit == -1
    poses = list(B.manoeuvre([20.5, 24.5, 28.5, 28.5, 28.5, 28.5], [2.5] * 6, [[1.0, 0.0]] * 6, [0.0, 4.0, 8.0, 8.0, 8.0, 8.0], 8.0, 6, 0, 0.0, H_DT))
    assert [p[1] for p in poses] == [24.5, 28.5, 28.5, 28.5, 28.5] and [p[6] for p in poses] == [4.0, 8.0, 8.0, 8.0, 8.0]
    assert [p[5] for p in poses] == [1, 2, 2, 2, 2]             # the first index with arc >= 8 is 2, for ever
    first, bf, st, commit = _hand(22.5, [8.0, 8.0, 0.0, 0.0, 0.0, 0.0], 0.0)      # ends at 30.5
    assert first == 2 and bf == [2, 2, 3, 4, 5, -1] and st == [6, 6, 2, 3, 4, 5] and commit == 0


# ------------------------------------------------------------------------------------------------ 2. the tie to the forecast
def dyadic_fan(win, T, dt=0.125):
    """straight trajectories along the road, either way, at constant speeds whose step v dt is a multiple of 1 / 8 m, from starts
    that are multiples of 1 / 8 m: every x, every v dt and every arc entry is exact in binary and arc[i + 1] - arc[i] == v dt"""
    rows = []
    for n, v in enumerate([0.0, 1.0, 2.0, 5.0, 8.0, 11.0, 14.0, 3.0]):
        for sign in (1.0, -1.0):
            x0 = SC.ORIGIN[0] + (win[0] + 6 + 9 * n) * SC.CS + 0.125
            rows.append((x0, -1.75 if sign > 0 else 1.625, sign, v))
    M = len(rows)
    k = np.arange(T, dtype=np.float64)
    x = np.stack([x0 + sign * (k * (v * dt)) for x0, _, sign, v in rows])
    y = np.stack([np.full(T, y0) for _, y0, _, _ in rows])
    head = np.zeros((M, T, 2))
    head[..., 0] = np.array([sign for _, _, sign, _ in rows])[:, None]
    v = np.stack([np.full(T, v) for _, _, _, v in rows])
    arc = SC.travelled_arc(x, y)
    assert all(np.array_equal(arc[m], k * (rows[m][3] * dt)) for m in range(M))
    return x, y, head, v, arc


def first_hit_after(cells):
    """per (m, b) the first sample i > b with cells[m][i] > 0, -1 = none"""
    M, T = cells.shape
    out = np.full((M, T), -1, dtype=np.int32)
    for m in range(M):
        for b in range(T):
            later = np.nonzero(cells[m, b + 1:] > 0)[0]
            if len(later):
                out[m, b] = b + 1 + later[0]
    return out


def test_without_deceleration_the_braking_ego_is_the_candidate():
    """constant speed, a_brake = 0, exact arithmetic: every brake pose is the candidate's own sample, so brake_first[m][b] is the
    first later sample with cells > 0 of the shipped forecast's checker"""
    dt, T = 0.125, 32
    sc = SC.scene(5, 0, T, entry=0, win=SC.WINDOWS[0])
    A = HR.arrival_map(sc.cls, sc.win, sc.road, HR.reach_table(8.0, dt, math.sqrt(2.0) * SC.CS, SC.CS, T))[0]
    x, y, head, v, arc = dyadic_fan(sc.win, T, dt)
    for m in range(len(x)):
        for b in (0, 7, 30):
            for i, xn, yn, c, s, idx, _ in B.manoeuvre(x[m].tolist(), y[m].tolist(), head[m].tolist(), arc[m].tolist(), v[m, b], T, b, 0.0, dt):
                assert (xn, yn, c, s) == (x[m, i], y[m, i], head[m, i, 0], head[m, i, 1]) and (idx == i or v[m, 0] == 0.0)
    cells, first, _ = HR.trajectories(A, sc.win, sc.road, SC.ORIGIN, SC.CS, x, y, head, SC.HL, SC.HW, SC.WB)
    bf, st, commit = B.brake(A, sc.win, sc.road, first, SC.ORIGIN, SC.CS, x, y, head, arc, v, SC.HL, SC.HW, SC.WB, 0.0, dt)
    assert np.array_equal(bf, first_hit_after(cells))
    assert (cells > 0).any() and (bf >= 0).any() and (bf < 0).any()
    assert np.array_equal(st, np.where(v > 0.0, T, np.arange(T)[None, :]))


# ------------------------------------------------------------------------------------------------ 3. the reference's own manoeuvre
def test_resampling_rule_is_the_references():
    """tests/golden/brake_manoeuvre.npz (written by tests/golden/gen_brake_manoeuvre.py): the reference's unmodified
    ``BE._calc_deceleration_trajectory(traj, break_time_step=b, deceleration=[a])``.  The inputs are dyadic, so that ``cumsum(v dt)``
    IS the chord length: the reference's running sum from 0 and this definition's sum from the anchor ``arc[b]`` then coincide
    exactly, which is what makes a bit-for-bit pin possible -- on inputs that round the two sums may differ in the last bits"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "brake_manoeuvre.npz"))
    dt = float(g["dt"])
    x, y, v = g["x"], g["y"], g["v"]
    T = x.shape[1]
    arc = SC.travelled_arc(x, y)
    head = np.stack((np.cos(g["theta"]), np.sin(g["theta"])), -1)
    stopped = moving = 0
    for n, b, a, x_new, y_new, v_new in zip(g["case_traj"], g["case_b"], g["case_a"], g["x_new"], g["y_new"], g["v_new"]):
        n, b, a = int(n), int(b), float(a)
        assert np.array_equal(arc[n], np.insert(np.cumsum(v[n] * dt), 0, 0)[:-1])      # the precondition of the pin
        poses = list(B.manoeuvre(x[n].tolist(), y[n].tolist(), head[n].tolist(), arc[n].tolist(), float(v[n, b]), T, b, a, dt))
        assert [p[0] for p in poses] == list(range(b + 1, T))
        assert np.array([p[1] for p in poses]).tobytes() == x_new[b + 1:].tobytes(), (n, b, a)
        assert np.array([p[2] for p in poses]).tobytes() == y_new[b + 1:].tobytes(), (n, b, a)
        vn = np.array([B.speed(float(v[n, b]), a, dt, i, b) for i in range(b, T)])
        assert vn.tobytes() == v_new[b:].tobytes() and np.array_equal(v_new[:b], v[n, :b])
        st = B.stop_sample(float(v[n, b]), a, dt, b, T)
        assert (st < T) == bool((v_new[b:] == 0.0).any()) and (st == T or v_new[st] == 0.0 and (v_new[b:st] > 0.0).all())
        stopped += st < T
        moving += st == T
    assert stopped > 20 and moving > 20


# ------------------------------------------------------------------------------------------------ 4. the random scenes
def test_random_scenes_are_not_degenerate():
    """the scenes tests/test_hidden_brake_gpu.py runs on the device, by the checker alone: of the candidates with a full horizon
    (T >= 31) at least a fifth are fail-safe throughout (commit = -1), at least a fifth lose it later on (commit > 0), some have
    lost it now (commit = 0), and some manoeuvres are hit only strictly after they stand, which does not count"""
    n = dict(none=0, later=0, now=0, after_stop=0, M=0, ragged_out=0)
    for spec in SC.RANDOM_SCENES:
        sc = SC.scene(*spec)
        A, _, first = SC.arrival_and_first(sc)
        stats = {}
        bf, st, commit = B.brake(A, sc.win, sc.road, first, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB,
                                 sc.a_brake, sc.dt, sc.lens, stats)
        assert bf.shape == st.shape == (sc.M, sc.T) and commit.shape == (sc.M,)
        assert ((bf == -1) | (bf > np.arange(sc.T)[None, :])).all() and (bf < sc.T).all()
        if sc.T >= 31:
            n["none"] += int((commit < 0).sum())
            n["later"] += int((commit > 0).sum())
            n["now"] += int((commit == 0).sum())
            n["after_stop"] += stats["after_stop"]
            n["M"] += sc.M
        n["ragged_out"] += int((st == -1).sum())
    print(n)
    assert 5 * n["none"] >= n["M"] and 5 * n["later"] >= n["M"] and n["now"] >= 1 and n["after_stop"] >= 1 and n["ragged_out"] > 0


# ------------------------------------------------------------------------------------------------ 5. the host layer
def test_travelled_arc_numpy_and_torch():
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import travelled_arc
    from frenetix_occlusion import sensor_model
    assert sensor_model.travelled_arc is travelled_arc
    rng = np.random.default_rng(7)
    x, y = np.cumsum(rng.uniform(0.0, 1.5, (9, 31)), axis=1), np.cumsum(rng.uniform(-0.3, 0.3, (9, 31)), axis=1)
    host = travelled_arc(x, y)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and host.shape == (9, 31)
    for m in range(9):                                          # be.py's formula, row by row
        assert np.array_equal(host[m], np.insert(np.cumsum(np.sqrt(np.diff(x[m]) ** 2 + np.diff(y[m]) ** 2)), 0, 0))
    dev = travelled_arc(torch.as_tensor(x), torch.as_tensor(y))
    assert torch.is_tensor(dev) and dev.dtype == torch.float64 and tuple(dev.shape) == (9, 31)
    ulp = np.spacing(np.maximum(host, 1e-300))
    assert (np.abs(dev.numpy() - host) <= 4 * ulp).all()
    xd, yd, _, _, arc = dyadic_fan(SC.WINDOWS[0], 32)
    assert np.array_equal(travelled_arc(torch.as_tensor(xd), torch.as_tensor(yd)).numpy(), arc) and np.array_equal(travelled_arc(xd, yd), arc)
    e = np.zeros((0, 5))
    assert travelled_arc(e, e).shape == (0, 5) and tuple(travelled_arc(torch.as_tensor(e), torch.as_tensor(e)).shape) == (0, 5)
    one = np.zeros((3, 1))
    assert np.array_equal(travelled_arc(one, one), one)


def test_decided_until():
    torch = pytest.importorskip("torch")
    from frenetix_occlusion.hidden_traffic import HiddenBrake
    from frenetix_occlusion.sensor_model import HiddenBrake as exported
    assert exported is HiddenBrake
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.int32))
    #        stands in time from every b | open from b = 3 | open from 0 | ragged, Lm = 4: open from b = 2 | Lm = 0
    stop = [[2, 3, 4, 5, 5, 5], [3, 4, 5, 6, 6, 6], [6] * 6, [2, 3, 4, 4, -1, -1], [-1] * 6]
    hb = HiddenBrake(None, t(stop), t(stop), t([0] * 5), None, 4.0, 0.1, t([6, 6, 9, 4, -2]))
    out = hb.decided_until()
    assert out.dtype == torch.int32 and out.tolist() == [6, 3, 0, 2, 0]
    hb = HiddenBrake(None, t(stop[:3]), t(stop[:3]), t([0] * 3), None, 4.0, 0.1)     # no lengths: Lm = T
    assert hb.decided_until().tolist() == [6, 3, 0]


class _Ctx:
    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append(name)


def _cpu_model(torch):
    """what hidden_reach and hidden_brake read of a SensorModel, on CPU tensors; the context records the entries it is asked for"""
    from frenetix_occlusion.cell_window import CellWindow
    w = CellWindow(SC.ORIGIN[0], SC.ORIGIN[1], SC.CS, 0, 0, 20, 10)
    om = SimpleNamespace(hidden_on_device=lambda w: None, hidden_vehicles_on_device=lambda w: None)
    return SimpleNamespace(window=w, cell_size=SC.CS, device=torch.device("cpu"), _om=om, _dev_index=0, ctx=_Ctx(), lane_moves=None,
                           cell_class=torch.zeros((10, 20), dtype=torch.uint8), raster_origin=SC.ORIGIN)


def test_refusals_come_after_hidden_reachs(monkeypatch):
    torch = pytest.importorskip("torch")
    from frenetix_occlusion import _native as N
    from frenetix_occlusion import hidden_traffic
    from frenetix_occlusion.sensor_model import SensorModel
    assert SensorModel.__dict__["hidden_brake"] is hidden_traffic.hidden_brake     # the module function itself, no wrapper
    monkeypatch.setattr(N, "current_stream", lambda index=None: None)
    z = np.zeros((2, 31))
    kw = dict(vehicle=SC.VEH, v_max=8.0, dt=0.1)
    sm = _cpu_model(torch)
    # hidden_reach's refusals first, in its words: a bad metric, bad lengths -- with v and a_brake wrong as well
    with pytest.raises(ValueError, match=r"^hidden_reach: metric 'manhattan'"):
        SensorModel.hidden_brake(sm, z, z, z, np.zeros((2, 30)), a_brake=-1.0, metric="manhattan", lengths=np.zeros(3), **kw)
    with pytest.raises(ValueError, match=r"^hidden_reach: lengths must be \[M\]$"):
        SensorModel.hidden_brake(sm, z, z, z, np.zeros((2, 30)), a_brake=-1.0, lengths=np.zeros(3), **kw)
    none = SimpleNamespace(window=None, cell_size=SC.CS)
    with pytest.raises(RuntimeError, match=r"^hidden_reach needs the cell classes of a previous launch\(\)$"):
        SensorModel.hidden_brake(none, z, z, z, np.zeros((2, 30)), a_brake=-1.0, **kw)
    assert sm.ctx.calls == []
    # then its own, v before a_brake
    with pytest.raises(ValueError, match=r"^hidden_brake: v must be \[M, T\]$"):
        SensorModel.hidden_brake(sm, z, z, z, np.zeros((2, 30)), a_brake=-1.0, **kw)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^hidden_brake: a_brake >= 0 and finite$"):
            SensorModel.hidden_brake(sm, z, z, z, z, a_brake=bad, **kw)
    assert "fo_scene_hidden_brake" not in sm.ctx.calls
    # a good call: the forecast's entry, then the brake entry, on the forecast's own device inputs
    sm = _cpu_model(torch)
    x = np.cumsum(np.full((2, 31), 0.5), axis=1)
    out = SensorModel.hidden_brake(sm, x, z, z, np.full((2, 31), 5.0), a_brake=0.0, metric="road", lengths=np.array([31, 7]), **kw)
    assert sm.ctx.calls == ["fo_scene_hidden_reach_road", "fo_scene_hidden_brake"]
    assert isinstance(out, hidden_traffic.HiddenBrake) and out.reach.metric == "road" and (out.a_brake, out.dt) == (0.0, 0.1)
    assert tuple(out.brake_first.shape) == tuple(out.stop.shape) == (2, 31) and tuple(out.commit.shape) == (2,)
    assert out.brake_first.dtype == out.stop.dtype == out.commit.dtype == torch.int32
    assert np.array_equal(out.arc.numpy(), hidden_traffic.travelled_arc(x, z)) and out.lengths.tolist() == [31, 7]
    assert sm._hr_inputs[0].data_ptr() != 0 and sm._hb_inputs[1] is out.arc


def test_native_mirror_matches_the_header():
    from frenetix_occlusion import _native as N
    assert "fo_scene_hidden_brake" in N.EXPORTS
    names = [f[0] for f in N.HiddenBrake._fields_]
    assert names == ["base", "d_v", "d_arc", "a_brake", "dt", "d_brake_first", "d_stop", "d_commit"]
    assert N.HiddenBrake.base.size == C.sizeof(N.HiddenReach) and N.HiddenBrake.a_brake.size == 8
    with open(os.path.join(ROOT, "include", "fo_hip.h")) as f:
        header = f.read()
    body = header[header.index("fo_hidden_reach_t base;", header.index("BRAKE CLEARANCE")):header.index("} fo_hidden_brake_t;")]
    order = [body.index(n) for n in ("d_v;", "d_arc;", "a_brake, dt;", "*d_brake_first, *d_stop;", "d_commit;")]
    assert order == sorted(order)
    assert "int fo_scene_hidden_brake(fo_ctx *ctx, const fo_hidden_brake_t *p, void *stream);" in header


def test_interface_defaults():
    pytest.importorskip("torch")
    from frenetix_occlusion.interface import FOInterface
    seen = {}

    def hidden_brake(x, y, theta, v, **kw):
        seen.update(kw, x=x, v=v)
        return "result"
    vp = SimpleNamespace(length=4.508, width=1.61, wb_rear_axle=1.4227, mass=1093.3, a_max=11.5)
    fo = SimpleNamespace(timestep=3, sensor_model=SimpleNamespace(window=object(), hidden_brake=hidden_brake),
                         occlusion_memory={"v_max": 13.9, "margin": 0.7}, vehicle_params=vp, dt=0.1)
    traj = {k: np.full((2, 5), i, dtype=np.float64) for i, k in enumerate(("x", "y", "theta", "v", "a"))}
    assert FOInterface.hidden_brake(fo, traj) == "result"
    assert seen["a_brake"] == 11.5 and seen["v_max"] == 13.9 and seen["margin"] == 0.7 and seen["dt"] == 0.1
    assert seen["vehicle"] == (4.508, 1.61, 1.4227) and seen["metric"] == "euclid" and seen["flow"] == "any" and seen["inflate"] == 0.0
    assert seen["v"] is traj["v"] and seen["x"] is traj["x"]
    FOInterface.hidden_brake(fo, traj, a_brake=4.0, v_max=5.0, margin=0.0, inflate=0.2, metric="road", flow="lanes")
    assert (seen["a_brake"], seen["v_max"], seen["margin"], seen["inflate"], seen["metric"], seen["flow"]) == (4.0, 5.0, 0.0, 0.2, "road", "lanes")
    fo.timestep = None
    with pytest.raises(RuntimeError, match="^hidden_brake needs a previous evaluate_scenario$"):
        FOInterface.hidden_brake(fo, traj)


# ------------------------------------------------------------------------------------------------ 6. the launch plan
_PLAN_DRIVER = r"""
#include <cstdio>
#include "fo_hip.h"
#include "fo_scene_plan.hpp"
int main() {
  long long M, T;
  printf("%d\n", HB_THREADS);
  while (scanf("%lld %lld", &M, &T) == 2)
    printf("%d %d %d %zu\n", brake_group((int)T), brake_per_block((int)T), brake_blocks((int)M, (int)T), brake_lds_bytes((int)T));
  return 0;
}
"""


def test_launch_plan(tmp_path):
    """the host functions of csrc/fo_scene_plan.hpp behind the launch (built alone with the host compiler): a lane per brake start,
    G = the power of two >= min(T, 64) lanes and six rows of T float64 in LDS per trajectory, 256 / G trajectories per workgroup --
    the M edges of tests/hidden_brake_scenes.RANDOM_SCENES are these -- and never more than 48 KB of LDS"""
    import shutil
    import subprocess
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "driver.cpp").write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "driver")
    csrc = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"), "-o", exe])
    asked = [(M, T) for T in (1, 2, 3, 31, 32, 33, 64, 65, 254) for M in (0, 1, 3, 4, 5, 7, 8, 9, 127, 128, 129, 255, 256, 257, 10000, 2 ** 31 - 1)]
    out = subprocess.run([exe], input="\n".join(f"{M} {T}" for M, T in asked) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(out[0]) == 256
    for (M, T), line in zip(asked, out[1:]):
        G = 1
        while G < min(T, 64):
            G *= 2
        per = 256 // G
        assert [int(v) for v in line.split()] == [G, per, -(-M // per), per * 6 * T * 8], (M, T)
        assert per * 6 * T * 8 <= 48 * 1024 + 768
    per_block = {1: 256, 2: 128, 31: 8, 32: 8, 33: 4, 64: 4, 65: 4, 254: 4}
    for T, per in per_block.items():       # the scenes take the three values of M around each edge (the long horizon: one value)
        Ms = {spec[1] for spec in SC.RANDOM_SCENES if spec[2] == T}
        assert {per - 1, per, per + 1} <= Ms or T == 254, T
