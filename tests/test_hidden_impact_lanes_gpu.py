"""Hidden-traffic impact verdict by approach angle on the device (fo_scene_hidden_brake_impact_lanes, SensorModel.hidden_brake_impact(
approach="lanes"), PlanningStep(hidden_impact_verdict=dict(approach="lanes")); DESIGN.md §5.10 "Impact verdict by approach angle"): the tie
to fo_scene_hidden_brake_impact of the same library on the same device inputs wherever nothing is known, the plain statement
tests/ref_hidden_impact_lanes.py on hand-built move tables, a hand case with the numbers written out, the edges of the hit cells, a real
scene, the fold, the step, the pre-filled outputs, the refusals.  Integers, closing speeds and cosines are compared with ``==`` (float64
without contraction, which the host reproduces bit for bit: tests/test_hidden_impact_lanes_cpu.py), harms to 1e-9, the start and the user
exactly -- the scenes hold no open choice (the same file).  Every test runs under a time limit of its own that ends the process; no test
provokes a fault."""
import ctypes as C
import faulthandler
import math
from types import SimpleNamespace

import numpy as np
import pytest

import hidden_brake_scenes as SC
import hidden_brake_users_scenes as US
import hidden_impact_cases as IC
import hidden_impact_lanes_cases as LC
import ref_hidden_impact as RI
import ref_hidden_impact_lanes as RL
import ref_hidden_reach_flow as RF
import rule_refusal_cases as RC
import test_hidden_brake_users_gpu as UG
import test_hidden_brake_verdict_gpu as VG
import test_hidden_impact_gpu as IG
import test_hidden_reach_flow_gpu as FG
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_np = T._np
HL, HW, WB = SC.HL, SC.HW, SC.WB
INT_OUTPUTS, F64_OUTPUTS = ("user", "at", "commit", "first"), ("harm", "closing", "cosine")
OUTPUTS = F64_OUTPUTS + INT_OUTPUTS
SHARED = ("harm", "user", "at", "commit", "first")      # the outputs the entry shares with fo_scene_hidden_brake_impact
STEP_LIMIT = 240
TOL = 1e-9
PATTERN, PAT_I32, PAT_F64 = IG.PATTERN, IG.PAT_I32, IG.PAT_F64
LANE_USERS = ((1.5, "road", "any"), (4.0, "road", "lanes"), (6.0, "road", "lanes"))     # of the step tests: a pedestrian, two lane-bound users
STEP_KINDS = IG.STEP_KINDS


@pytest.fixture(autouse=True)
def _time_limit(request):
    faulthandler.dump_traceback_later(getattr(request.module, request.function.__name__ + "_limit", STEP_LIMIT), exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ------------------------------------------------------------------------------------------------ the raw entry
def _raw_lanes(torch, sm, win, r2_caps, keys, qmins, x, y, head, v, arc, a_brake, dt, thr, map_of, B, rows, speed_of, dir_mask, slack=0.0,
               harm_limit=math.inf, lens=None, finite=None, cost=None, safe=None, alias=(), hl=HL, hw=HW, wb=WB, drop=(), drop_map=(), **over):
    """fo_scene_hidden_brake_impact_lanes on maps and trajectories of the test's own, against the move table the context holds; every
    byte of the output buffers is pre-filled with PATTERN.  The arguments as tests/test_hidden_impact_gpu._raw_impact's, and ``dir_mask``,
    ``slack`` (cos_h and sin_h are the host's of 22.5 deg + slack).  Returns (rc, message, outputs)"""
    from frenetix_occlusion import _native as N
    dev = sm.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    M, Tn = x.shape
    thr = np.ascontiguousarray(thr, dtype=np.int32)
    Cn, Kn = thr.shape[0], len(keys)
    tx, ty, th, tv, ta = (up(a, np.float64) for a in (x, y, head, v, arc))
    dk, dq, tl, tf = [up(k, np.int32) for k in keys], [up(q, np.int32) for q in qmins], up(lens, np.int32), up(finite, np.uint8)
    if alias:
        dk[alias[0]] = dk[alias[1]]
    tc, ts = up(cost, np.float64), up(safe, np.uint8)
    trow, tsp = up(np.asarray(rows, dtype=np.float64).reshape(Cn, 4), np.float64), up(np.asarray(speed_of, dtype=np.float64), np.float64)

    def filled(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(PATTERN)
        return t
    out = SimpleNamespace(harm=filled((M, 2), torch.float64), user=filled((M,), torch.int32), closing=filled((Cn, M), torch.float64),
                          cosine=filled((Cn, M), torch.float64), at=filled((Cn, M), torch.int32), commit=filled((Cn, M), torch.int32),
                          first=filled((Cn, M), torch.int32))
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    pad = lambda vals, n, fill: (list(vals) + [fill] * n)[:n]
    ptrs = dict(d_key=pad([p(t) for t in dk], 3, None), d_qmin=pad([p(t) for t in dq], 3, None))
    for name, k in drop_map:
        ptrs[name][k] = None
    cos_h, sin_h = RL.host_h(slack)
    kw = dict(M=M, T=Tn, d_x=p(tx), d_y=p(ty), d_heading=p(th), d_len_or_null=p(tl), hl=hl, hw=hw, wb=wb, win_ix0=win[0], win_iy0=win[1],
              win_nx=win[2], win_ny=win[3], K=Kn, C=Cn, d_key=(C.c_void_p * 3)(*ptrs["d_key"]), d_qmin=(C.c_void_p * 3)(*ptrs["d_qmin"]),
              r2_cap=(C.c_int32 * 3)(*pad([int(r) for r in r2_caps], 3, -5)), map_of=(C.c_int32 * 8)(*pad([int(k) for k in map_of], 8, 99)),
              d_v=p(tv), d_arc=p(ta), a_brake=float(a_brake), dt=float(dt), h_thr=thr.ctypes.data_as(C.POINTER(C.c_int32)), B=int(B),
              d_speed_of=p(tsp), d_harm_rows=p(trow), harm_limit=float(harm_limit), d_finite_or_null=p(tf), d_cost_or_null=p(tc),
              d_safe_or_null=p(ts), d_harm=p(out.harm), d_user=p(out.user), d_closing=p(out.closing), d_at=p(out.at), d_commit=p(out.commit),
              d_first=p(out.first), dir_mask=int(dir_mask), cos_h=cos_h, sin_h=sin_h, d_cosine=p(out.cosine))
    kw.update(over)
    for k in drop:
        kw[k] = None
    args = N.HiddenBrakeImpactLanes(**kw)
    rc = sm.ctx._lib.fo_scene_hidden_brake_impact_lanes(sm.ctx._h, C.byref(args), N.current_stream(0))
    torch.cuda.synchronize()
    msg = sm.ctx._lib.fo_last_error(sm.ctx._h).decode()
    res = SimpleNamespace(**{k: _np(getattr(out, k)) for k in OUTPUTS})
    res.cost, res.safe = (None if tc is None else _np(tc)), (None if ts is None else _np(ts))
    return rc, msg, res


def _untouched(out):
    return all((getattr(out, k).view(np.uint8) == PATTERN).all() for k in OUTPUTS)


def _assert_written(out, what):
    for k in INT_OUTPUTS:
        assert (getattr(out, k) != PAT_I32).all(), (what, k)
    for k in F64_OUTPUTS:
        assert (getattr(out, k) != PAT_F64).all(), (what, k)


def _moves(sm, moves):
    from frenetix_occlusion import _native as N
    assert FG._set_moves(sm, moves) == N.FO_OK


# ------------------------------------------------------------------------------------------------ 1. the tie
def _tie(torch, sm, sc, M, B, keys, qmins, thr, map_of, r2_caps, rows, speed_of, what, alias=(), last=False):
    """the three ways of knowing nothing -- no lane-bound class, a table of 0xFF alone, heading_slack = pi -- against the head-on entry
    on the same device inputs: the shared outputs bit for bit, closing == speed + speed_of bit for bit, cosine == 1.0"""
    cut = lambda a: None if a is None else (a[len(a) - M:] if last else a[:M])
    x, y, head, v, arc, lens = (cut(a) for a in (sc.x, sc.y, sc.head, sc.v, sc.arc, sc.lens))
    qm = [cut(q) for q in qmins]
    Cn = len(thr)
    every = (1 << Cn) - 1
    rc, msg, ref = IG._raw_impact(torch, sm, sc.win, r2_caps, keys, qm, x, y, head, v, arc, sc.a_brake, sc.dt, thr, map_of, B, rows, speed_of,
                                  lens=lens, alias=alias)
    assert rc == 0, (what, msg)
    want_closing = np.where(ref.at >= 0, ref.speed + np.asarray(speed_of, dtype=np.float64)[:, None], 0.0)
    for name, table, mask, slack in (("dir_mask = 0", "cross", 0, 0.0), ("a table of 0xFF", "any", every, 0.0), ("slack = pi", "cross", every, math.pi)):
        _moves(sm, LC.table(table))
        rc, msg, out = _raw_lanes(torch, sm, sc.win, r2_caps, keys, qm, x, y, head, v, arc, sc.a_brake, sc.dt, thr, map_of, B, rows, speed_of, mask,
                                  slack, lens=lens, alias=alias)
        assert rc == 0, (what, name, msg)
        _assert_written(out, (what, name))
        for k in SHARED:
            got, want = getattr(out, k), getattr(ref, k)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, name, k, np.argwhere(got != want)[:4].tolist())
        assert out.closing.tobytes() == want_closing.tobytes(), (what, name, "closing", np.argwhere(out.closing != want_closing)[:4].tolist())
        assert (out.cosine == 1.0).all(), (what, name)
    return ref


@pytest.mark.parametrize("T_", [1, 2, 31, 65])
def test_tie_to_the_head_on_entry_at_every_group_size(torch_cuda, T_):
    """T in {1, 2, 31, 65} x B in {1, 2, 5, T}, M at per_block - 1, per_block, per_block + 1 of every (T, B), on three maps, on the scene's
    first M trajectories (lengths 0, 1, 2 lead them) and on its last M (the seed's ragged lengths)"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc = VG._scene(VG.TIE_SCENES[T_], US.USERS)
    rows, speed_of = IC.rows_of(IC.KINDS5), [u[0] for u in US.USERS]
    hits = 0
    for B in sorted({b for b in (1, 2, 5, T_) if b <= T_}):
        per = VG._per_block(T_, 3, B)
        for M in sorted({m for m in (per - 1, per, per + 1) if m >= 1}):
            assert M + 3 <= sc.M
            for last in (False, True):
                ref = _tie(torch, sm, sc, M, B, sc.keys, sc.qmins, sc.thr, sc.map_of, sc.r2_caps, rows, speed_of, (T_, B, M, last), last=last)
                hits += int((ref.at >= 0).sum())
    assert hits > 0


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("C_", [1, 4, 5, 8])
def test_tie_over_class_and_map_counts(torch_cuda, C_, K):
    """C in {1, 4, 5, 8} x K in {1, 2, 3}: all six instantiations, class c on map (c + 1) % K -- and, with K >= 2, map 1 handed over as
    the very BUFFER of map 0"""
    torch = torch_cuda
    sm, _ = UG._parked()
    sc, keys, qmins, cap = UG._three_maps()
    map_of = [(c + 1) % K for c in range(C_)]
    rows, speed_of = IC.rows_of(IC.KINDS8[:C_]), UG.SPEEDS8[:C_]
    for B in (5, 31):
        _tie(torch, sm, sc, sc.M, B, keys[:K], qmins[:K], sc.thr[:C_], map_of, [cap] * K, rows, speed_of, (C_, K, B))
    if K >= 2:
        same = [keys[0]] + keys[:K - 1]
        same_q = [qmins[0]] + qmins[:K - 1]
        _tie(torch, sm, sc, sc.M, 5, same, same_q, sc.thr[:C_], map_of, [cap] * K, rows, speed_of, (C_, K, "alias"), alias=(1, 0))


# ------------------------------------------------------------------------------------------------ 2. the checker
def _assert_checker(torch, sm, what, win, r2_caps, keys, qmins, x, y, head, v, arc, a_brake, dt, thr, map_of, B, rows, speed_of, mask, slack,
                    moves, lens=None, finite=None, road=None, origin=SC.ORIGIN, cs=SC.CS):
    """the entry against tests/ref_hidden_impact_lanes.py run on the users entry's brake_first / stop / first of the same device inputs:
    closing and cosine bit for bit, at and user exactly, harm to 1e-9"""
    _moves(sm, moves)
    rc, msg, users = UG._raw_users(torch, sm, win, r2_caps, keys, qmins, x, y, head, v, arc, a_brake, dt, thr, map_of, lens)
    assert rc == 0, (what, msg)
    rc, msg, out = _raw_lanes(torch, sm, win, r2_caps, keys, qmins, x, y, head, v, arc, a_brake, dt, thr, map_of, B, rows, speed_of, mask, slack,
                              lens=lens, finite=finite)
    assert rc == 0, (what, msg)
    _assert_written(out, what)
    cos_h, sin_h = RL.host_h(slack)
    harm, user, clos, at, cosn, n_open, by_start = RL.impact_lanes(
        keys, win, SC.road_raster() if road is None else road, moves, origin, cs, x, y, head, arc, v, HL, HW, WB, a_brake, dt, thr, map_of, B, rows, speed_of,
        mask, cos_h, sin_h, users.brake_first, users.stop, users.first, lens, finite)
    assert n_open == 0 and RL.close_starts(by_start) == 0, what
    assert np.array_equal(out.first, users.first), what
    assert np.array_equal(out.at, at), (what, "at", np.argwhere(out.at != at)[:4].tolist())
    assert out.closing.tobytes() == clos.tobytes(), (what, "closing", np.argwhere(out.closing != clos)[:4].tolist(), out.closing[out.closing != clos][:4],
                                                     clos[out.closing != clos][:4])
    assert out.cosine.tobytes() == cosn.tobytes(), (what, "cosine", np.argwhere(out.cosine != cosn)[:4].tolist())
    worst = float(np.abs(out.harm - harm).max()) if harm.size else 0.0
    assert worst <= TOL, (what, "harm", worst)
    assert np.array_equal(out.user, user), (what, "user")
    return out


@pytest.mark.parametrize("case", range(len(LC.RAW_CASES)))
def test_raw_entry_scenes_with_hand_built_move_tables(torch_cuda, case):
    """tests/hidden_impact_lanes_cases.RAW_CASES: masks none, all and mixed -- a lane-bound class and a free class on the same map --, the
    lane table and the striped one, slacks 0, 0.2 and pi / 2, C x K over 4- and 8-wide kernels on one to three maps"""
    torch = torch_cuda
    sm, _ = UG._parked()
    name, C_, K, tab, mask, slack, B = LC.RAW_CASES[case]
    sc, keys, qmins, thr, map_of, r2_caps, rows, speed_of = LC.raw_scene(name, C_, K)
    out = _assert_checker(torch, sm, LC.RAW_CASES[case], sc.win, r2_caps, keys, qmins, sc.x, sc.y, sc.head, sc.v, sc.arc, sc.a_brake, sc.dt, thr,
                          map_of, B, rows, speed_of, mask, slack, LC.table(tab), lens=sc.lens)
    print(f"{LC.RAW_CASES[case]}: {int((out.at >= 0).sum())} pairs with a hit, {int((out.cosine < 1.0).sum())} below head-on, "
          f"cosines {sorted(set(np.round(out.cosine.ravel(), 3).tolist()))[:8]}")
    if mask == 0:
        assert (out.cosine == 1.0).all()


# ------------------------------------------------------------------------------------------------ 3. a hand case with known numbers
def _hand(torch, sm, h, B, mask=1, slack=0.0, rows=(LC.CAR_ROW,), speed_of=(LC.CAR_SPEED,), check=True):
    if check:
        return _assert_checker(torch, sm, "hand", h.win, [h.r2_cap], [h.key], [h.qmin], h.x, h.y, h.head, h.v, h.arc, h.a_brake, h.dt, h.thr, [0], B,
                               list(rows), list(speed_of), mask, slack, h.moves)
    _moves(sm, h.moves)
    rc, msg, out = _raw_lanes(torch, sm, h.win, [h.r2_cap], [h.key], [h.qmin], h.x, h.y, h.head, h.v, h.arc, h.a_brake, h.dt, h.thr, [0], B,
                              list(rows), list(speed_of), mask, slack)
    assert rc == 0, msg
    return out


def test_hand_case_with_known_numbers(torch_cuda):
    """the ego heads East at 8 m/s and brakes at 4 m/s^2 (dt 0.5: poses 0 4 7 9 10 m); its front reaches a wall of cells at 10 m at sample 2
    with u = 4 m/s left, where a car at 13.9 m/s may be: from a north-bound cross lane cosine = cos 67.5 deg = 0.38268343236508967...,
    closing = sqrt(16 + 193.21 + 2 * 4 * 13.9 * 0.38268...) = 15.86708...; from the oncoming lane cosine 1, closing 17.9; from the ego's own
    lane behind it cosine = -cos 22.5 deg = -0.92387953251128674, closing 10.31865...; from an off-lane cell 1 and 17.9"""
    torch = torch_cuda
    sm, road = UG._parked()
    assert abs(LC.COS_67_5 - math.cos(math.radians(67.5))) <= 1e-15 and abs(LC.COS_157_5 - math.cos(math.radians(157.5))) <= 1e-15
    assert abs(LC.HAND[0][3] - 15.867085) <= 1e-5 and abs(LC.HAND[2][3] - 10.318653) <= 1e-5 and LC.HAND[1][3] == 17.9
    for name, byte, cosine, closing in LC.HAND:
        h = LC.hand_case(8.0, 4.0, 10.0, byte)
        assert np.array_equal(road, h.road)
        out = _hand(torch, sm, h, 1)
        assert out.first.tolist() == [[2]] and out.at.tolist() == [[0]] and out.user.tolist() == [0], name
        assert abs(out.cosine[0, 0] - cosine) <= 1e-15 and abs(out.closing[0, 0] - closing) <= 1e-14, (name, out.cosine, out.closing)
        assert (out.cosine[0, 0] == 1.0) == (cosine == 1.0) and (cosine < 1.0 or out.closing[0, 0] == 17.9), name
        want = 1.0 / (1.0 + math.exp(LC.CAR_ROW[0] + LC.CAR_ROW[1] * closing))
        assert abs(out.harm[0, 0] - want) <= TOL, name
        free = _hand(torch, sm, h, 1, mask=0)                          # the same car, not lane-bound: head-on
        assert free.cosine.tolist() == [[1.0]] and free.closing.tolist() == [[17.9]] and free.harm[0, 0] >= out.harm[0, 0], name


# ------------------------------------------------------------------------------------------------ 4. the edges
NORTH, WEST, EAST = RF.sector(90), RF.sector(180), RF.sector(0)


def test_a_hit_cell_at_the_footprints_edge(torch_cuda):
    """the wall's first column is a north-bound lane, its second the oncoming one; braking from 8 m/s the poses are x0 + 0 4 7 9: the front
    edge first covers the wall at sample 3, and lies 1e-9 m beyond or short of the centres of the second column's cells -- inside, the
    oncoming byte counts (cosine 1); outside, the cross lane alone (cos 67.5 deg)"""
    torch = torch_cuda
    sm, _ = UG._parked()
    g0 = int(round((12.0 - SC.ORIGIN[0]) / SC.CS))
    for eps, cosine in ((1e-9, 1.0), (-1e-9, LC.COS_67_5)):
        x0 = LC.cell_centre_x(g0 + 1) + eps - (9.0 + LC.FRONT)
        h = LC.hand_case(8.0, 4.0, 12.0, (NORTH, WEST, WEST, WEST), x0=x0)
        assert h.wall_gx == g0 and 7.0 + x0 + LC.FRONT < LC.cell_centre_x(g0)
        out = _hand(torch, sm, h, 1)
        assert out.at.tolist() == [[0]] and abs(out.cosine[0, 0] - cosine) <= 1e-15, (eps, out.cosine)
        assert abs(out.closing[0, 0] - LC.closing_of(2.0, LC.CAR_SPEED, cosine)) <= 1e-14          # 8 - 4 * 1.5 = 2 m/s left


def test_a_key_at_the_threshold_counts_and_one_above_does_not(torch_cuda):
    """the wall's first column holds key 7 on a north-bound lane, the others key 8 on the oncoming one, all under the footprint at the
    hit: at thr = 7 the first column alone is a hit cell, at thr = 8 all are"""
    torch = torch_cuda
    sm, _ = UG._parked()
    for thr, cosine in ((7, LC.COS_67_5), (8, 1.0)):
        h = LC.hand_case(8.0, 4.0, 10.0, (NORTH, WEST, WEST, WEST), keys_at_wall=(7, 8, 8, 8), thr=thr, x0=0.25)
        out = _hand(torch, sm, h, 1)
        assert out.at.tolist() == [[0]] and abs(out.cosine[0, 0] - cosine) <= 1e-15, (thr, out.cosine)
    h = LC.hand_case(8.0, 4.0, 10.0, NORTH, keys_at_wall=(8, 8, 8, 8), thr=7)
    out = _hand(torch, sm, h, 1)
    assert out.at.tolist() == [[-1]] and out.closing.tolist() == [[0.0]] and out.cosine.tolist() == [[1.0]] and out.user.tolist() == [-1]


def test_hit_cells_outside_the_window_and_off_the_raster(torch_cuda):
    """outside the window a cell of raster road carries key 0 and its own byte of the table; a window cell off the raster carries its key
    and 0xFF"""
    torch = torch_cuda
    sm, _ = UG._parked()
    # a window over a part of the road (columns 30 .. 99): the road beyond its east end, a north-bound lane, is hit at key 0
    win = SC.WINDOWS[1]
    east_end = SC.ORIGIN[0] + (win[0] + win[2]) * SC.CS                 # 39 m
    h = LC.hand_case(8.0, 4.0, east_end, NORTH, keys_at_wall=(), beside=NORTH, win=win, x0=east_end - 10.0)
    assert (h.key == LC.NONE).all()
    out = _hand(torch, sm, h, 1)
    assert out.at.tolist() == [[0]] and abs(out.cosine[0, 0] - LC.COS_67_5) <= 1e-15, out.cosine
    # the rim of the whole-raster window beyond the raster's east end (columns 164 .. 167) holds key 0: off the raster, 0xFF whatever the
    # table says beside it; the same key on the raster's last columns reads the table
    end = SC.ORIGIN[0] + SC.RNX * SC.CS                                 # 71 m
    for wall_x, cosine in ((end, 1.0), (end - 2.0, LC.COS_67_5)):
        h = LC.hand_case(8.0, 4.0, wall_x, NORTH, beside=NORTH, x0=wall_x - 10.0)
        out = _hand(torch, sm, h, 1)
        assert out.at.tolist() == [[0]] and abs(out.cosine[0, 0] - cosine) <= 1e-15, (wall_x, out.cosine)


def test_the_met_case_against_a_manoeuvre_hit(torch_cuda):
    """the wall at 14 m: braking from b = 0 the ego comes to rest short of it; the candidate itself reaches it at sample 3 at 8 m/s, the
    starts 1 and 2 hit it on their manoeuvres at less: the met pose prices the class, at = 3, against a north-bound lane at cos 67.5 deg"""
    torch = torch_cuda
    sm, _ = UG._parked()
    h = LC.hand_case(8.0, 4.0, 14.0, NORTH)
    out = _hand(torch, sm, h, 6)
    assert out.first.tolist() == [[3]] and out.at.tolist() == [[3]] and abs(out.cosine[0, 0] - LC.COS_67_5) <= 1e-15
    assert abs(out.closing[0, 0] - LC.closing_of(8.0, LC.CAR_SPEED, LC.COS_67_5)) <= 1e-14
    out = _hand(torch, sm, h, 3)                                       # B = 3: the met start is not looked at, the manoeuvres from 1 and 2 are
    assert out.at[0, 0] in (1, 2) and out.closing[0, 0] < LC.closing_of(8.0, LC.CAR_SPEED, LC.COS_67_5)
    # a_brake = 0: the manoeuvre is the candidate; met at sample 3 from b = 3 on, hit on the manoeuvre at the same place before
    h = LC.hand_case(8.0, 0.0, 14.0, (NORTH, WEST, WEST, WEST))
    _hand(torch, sm, h, 6)


def test_two_classes_first_hit_at_one_pose_against_different_maps(torch_cuda):
    """class 0 on map 0, whose wall is the first column (a north-bound lane); class 1 on map 1, whose wall is the second column (the
    oncoming lane): both are first hit at the same pose, each by the cells of its own map"""
    torch = torch_cuda
    sm, _ = UG._parked()
    h = LC.hand_case(8.0, 4.0, 10.0, (NORTH, WEST, WEST, WEST), keys_at_wall=(0, LC.NONE, LC.NONE, LC.NONE), x0=0.25)
    h2 = LC.hand_case(8.0, 4.0, 10.0, (NORTH, WEST, WEST, WEST), keys_at_wall=(LC.NONE, 0, LC.NONE, LC.NONE), x0=0.25)
    thr = np.zeros((2, h.T), dtype=np.int32)
    rows, speed_of = [LC.CAR_ROW, LC.CAR_ROW], [LC.CAR_SPEED, 7.0]
    for map_of, keys, qmins in (([0, 1], [h.key, h2.key], [h.qmin, h2.qmin]), ([1, 0], [h2.key, h.key], [h2.qmin, h.qmin])):
        out = _assert_checker(torch, sm, ("two maps", map_of), h.win, [1, 1], keys, qmins, h.x, h.y, h.head, h.v, h.arc, h.a_brake, h.dt, thr, map_of,
                              1, rows, speed_of, 0b11, 0.0, h.moves)
        assert out.at.tolist() == [[0], [0]] and abs(out.cosine[0, 0] - LC.COS_67_5) <= 1e-15 and out.cosine[1, 0] == 1.0, out.cosine
        assert out.closing[1, 0] == 4.0 + 7.0 and abs(out.closing[0, 0] - LC.closing_of(4.0, LC.CAR_SPEED, LC.COS_67_5)) <= 1e-14


def test_a_hit_at_the_last_moving_sample_counts_and_one_at_the_stop_does_not(torch_cuda):
    """braking from 8 m/s at 4 m/s^2 the ego stands from sample 4 on (poses 0 4 7 9 10 10 ...): a wall first covered at sample 3 = st - 1 is
    hit with 2 m/s left; one first covered at sample 4 = st meets a standing ego and carries no harm"""
    torch = torch_cuda
    sm, _ = UG._parked()
    out = _hand(torch, sm, LC.hand_case(8.0, 4.0, 12.0, NORTH), 1)
    assert out.at.tolist() == [[0]] and out.commit.tolist() == [[0]] and abs(out.closing[0, 0] - LC.closing_of(2.0, LC.CAR_SPEED, LC.COS_67_5)) <= 1e-14
    out = _hand(torch, sm, LC.hand_case(8.0, 4.0, 13.0, NORTH), 1)
    assert out.at.tolist() == [[-1]] and out.commit.tolist() == [[-1]] and out.closing.tolist() == [[0.0]] and out.cosine.tolist() == [[1.0]]
    assert out.harm.tolist() == [[0.0, 0.0]] and out.user.tolist() == [-1]


# ------------------------------------------------------------------------------------------------ 5. a real scene
def test_never_above_head_on_on_scenario_1(torch_cuda, tmp_path):
    """scenario 1 with its own lane_move_raster and the three README users: for every candidate harm <= the head-on harm, per user
    closing <= speed + speed_of, commit and first are the head-on call's; the pedestrian (not lane-bound) is priced as before"""
    torch = torch_cuda
    import test_hidden_witness_gpu as WG
    from frenetix_occlusion import synthetic as SY
    sc = T._scenario("scenario1")
    fo = WG._interface(tmp_path, sc)
    ego, yaw = WG._drive(fo, sc, 3)
    traj = SY.make_trajectories(64, 31, WG.DT, seed=WG.SEED, ego_pos=ego, ego_yaw=yaw)
    users = ((2.0, "road", "any"), (7.0, "road", "lanes"), (13.9, "road", "lanes"))
    assert fo.sensor_model.lane_moves is not None
    head = fo.hidden_brake_impact(traj, users, starts=5)
    lanes = fo.hidden_brake_impact(traj, users, starts=5, approach="lanes")
    wide = fo.hidden_brake_impact(traj, users, starts=5, approach="lanes", heading_slack=math.pi)
    torch.cuda.synchronize()
    assert lanes.speed is None and lanes.approach == "lanes" and head.closing is None and head.approach == "head_on"
    w_head = _np(head.closing_speed(0)), _np(head.closing_speed(1)), _np(head.closing_speed(2))
    for c in range(3):
        assert (_np(lanes.closing)[c] <= w_head[c]).all(), c
    assert _np(lanes.closing)[0].tobytes() == w_head[0].tobytes() and (_np(lanes.cosine)[0] == 1.0).all()
    assert (_np(lanes.harm)[:, 0] <= _np(head.harm)[:, 0]).all()
    for name in ("commit", "first"):
        assert torch.equal(getattr(lanes, name), getattr(head, name)), name
    for name in SHARED:
        assert torch.equal(getattr(wide, name), getattr(head, name)), name
    assert torch.equal(wide.closing, torch.stack([head.closing_speed(c) for c in range(3)])) and (wide.cosine == 1.0).all()
    cosn = _np(lanes.cosine)
    print(f"scenario 1: obstacle harm head-on max {_np(head.harm)[:, 0].max():.4f}, by approach max {_np(lanes.harm)[:, 0].max():.4f}; "
          f"{int((cosn < 1.0).sum())} of {int((_np(lanes.at) >= 0).sum())} hits below head-on; users change for "
          f"{int((_np(lanes.user) != _np(head.user)).sum())} of {len(cosn[0])} candidates")
    with pytest.raises(ValueError, match="closing_speed"):
        lanes.impact_speed()
    picked = _np(lanes.closing_speed())
    user = _np(lanes.user)
    assert np.array_equal(picked, np.where(user >= 0, _np(lanes.closing)[np.clip(user, 0, None), np.arange(len(user))], 0.0))
    assert np.abs(np.stack([_np(lanes.harm_of(c))[:, 0] for c in range(3)]).max(axis=0) - _np(lanes.harm)[:, 0]).max() <= TOL


# ------------------------------------------------------------------------------------------------ 6. the fold, the step
def _iv(**over):
    kw = dict(vehicle=VG.VEH3, ego_mass=RC.VEH[3], users=LANE_USERS, kinds=STEP_KINDS, dt=0.1, a_brake=8.0, starts=5, harm_limit=0.1,
              approach="lanes", heading_slack=0.1)
    kw.update(over)
    return kw


def _step_then_stage(torch, k, tr=None, **over):
    from frenetix_occlusion.step import PlanningStep
    tr = k.tr if tr is None else tr
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced")
    out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    assert not hasattr(out, "hidden_impact_verdict")
    before = (out.cost.clone(), out.safe.clone())
    iv = k.sm.hidden_brake_impact(*tr[:4], cost=out.cost, safe=out.safe, **_iv(**over))
    torch.cuda.synchronize()
    return (_np(before[0]), _np(before[1])), (_np(out.cost), _np(out.safe)), iv


def test_fold_on_the_rows_of_a_real_step(torch_cuda):
    """clean rows: the fold is the checker's on what the stage wrote; the stage itself is the checker on the device data it walked on;
    never above the head-on stage"""
    torch = torch_cuda
    k = VG._stack(torch)
    assert k.sm.lane_moves is not None
    before, after, iv = _step_then_stage(torch, k)
    IG._assert_fold(before, after, iv, 0.1)
    x, y, v = (_np(t) for t in (k.tr[0], k.tr[1], k.tr[3]))
    w = k.sm.window
    out = _assert_checker(torch, k.sm, "stage", (w.ix0, w.iy0, w.nx, w.ny), [c.r2_cap for c in iv.clearances], [_np(c.key) for c in iv.clearances],
                    [_np(c.qmin) for c in iv.clearances], x, y, _np(iv.poses.heading), v, _np(iv.poses.arc), 8.0, 0.1, iv.thr, iv.map_of, 5,
                          iv.rows, iv.speed_of, 0b110, 0.1, k.sm.lane_moves, finite=_np(iv.poses.finite), road=k.sm.road_raster(),
                          origin=tuple(k.sm.raster_origin), cs=k.sm.cell_size)
    for name in OUTPUTS:                                               # (the checker's call set the very table the model holds)
        assert getattr(out, name).tobytes() == _np(getattr(iv, name)).tobytes(), name
    rc_out = _np(iv.closing)
    _, _, head = _step_then_stage(torch, k, approach="head_on", heading_slack=0.0)
    assert (rc_out <= _np(torch.stack([head.closing_speed(c) for c in range(3)]))).all() and (_np(iv.harm)[:, 0] <= _np(head.harm)[:, 0]).all()
    assert iv.approach == "lanes" and iv.heading_slack == 0.1 and iv.speed is None
    before, after, iv_inf = _step_then_stage(torch, k, harm_limit=math.inf)
    IG._assert_fold(before, after, iv_inf, math.inf)
    assert np.array_equal(after[1], before[1])


def test_a_refused_step_and_a_non_finite_candidate(torch_cuda):
    """a refused step stays unsafe and gets the two columns; a NaN, an inf and a -inf pose fail closed even at harm_limit = inf"""
    torch = torch_cuda
    import test_rule_refusal_gpu as RG
    k = VG._stack(torch, RG.REFUSING_CELL)
    before, after, iv = _step_then_stage(torch, k)
    RG.assert_refused(SimpleNamespace(cost=torch.as_tensor(before[0]), safe=torch.as_tensor(before[1])))
    IG._assert_fold(before, after, iv, 0.1)
    assert not after[1].any() and after[0][:, RI.C_RES0].tobytes() == _np(iv.harm)[:, 0].tobytes()
    k = VG._stack(torch)
    tr = [t.clone() for t in k.tr]
    tr[0][3, 7], tr[2][11, 0], tr[3][40, 15] = float("nan"), float("inf"), float("-inf")
    before, after, iv = _step_then_stage(torch, k, tr=tr, harm_limit=math.inf)
    IG._assert_fold(before, after, iv, math.inf)
    harm, user = _np(iv.harm), _np(iv.user)
    for m in (3, 11, 40):
        assert (harm[m].tolist(), user[m], after[1][m], after[0][m, RI.C_SAFE], after[0][m, RI.C_RES0], after[0][m, RI.C_RES1]) == ([1.0, 1.0], -2, 0, 0.0, 1.0, -2.0), m
    rest = [m for m in range(RC.M) if m not in (3, 11, 40)]
    assert (user[rest] >= -1).all() and np.array_equal(after[1][rest], before[1][rest])


def test_step_with_the_approach_is_the_call_and_a_step_without_the_stage_is_unchanged(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion.step import PlanningStep
    k = VG._stack(torch)
    plain, staged, iv = _step_then_stage(torch, k)
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_impact_verdict=_iv())
    for _ in range(2):
        out = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
        torch.cuda.synchronize()
        assert _np(out.cost).tobytes() == staged[0].tobytes() and np.array_equal(_np(out.safe), staged[1])
        for name in OUTPUTS:
            assert torch.equal(getattr(out.hidden_impact_verdict, name), getattr(iv, name)), name
        assert out.hidden_impact_verdict.speed is None
    out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced").run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert not hasattr(out, "hidden_impact_verdict") and _np(out.cost).tobytes() == plain[0].tobytes() and np.array_equal(_np(out.safe), plain[1])
    # the default approach is the head-on stage as it was: the keyword spelled out changes nothing
    _, staged_head, head = _step_then_stage(torch, k, approach="head_on", heading_slack=0.0)
    kw = {key: val for key, val in _iv().items() if key not in ("approach", "heading_slack")}
    out = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", hidden_impact_verdict=kw).run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert _np(out.cost).tobytes() == staged_head[0].tobytes() and torch.equal(out.hidden_impact_verdict.speed, head.speed)
    assert out.hidden_impact_verdict.closing is None


# ------------------------------------------------------------------------------------------------ 7. every byte is written
def test_every_byte_of_every_output_is_written(torch_cuda):
    torch = torch_cuda
    sm, _ = UG._parked()
    _moves(sm, LC.table("cross"))
    sc = VG._scene(VG.TIE_SCENES[31], US.USERS)
    rows, speed_of = IC.rows_of(IC.KINDS5), [u[0] for u in US.USERS]
    per = VG._per_block(31, 3, 5)
    for M in (1, per - 1, per, per + 1, sc.M):
        for lens, finite in ((None, None), (sc.lens[:M], np.arange(M, dtype=np.uint8) % 2)):
            rc, msg, out = _raw_lanes(torch, sm, sc.win, sc.r2_caps, sc.keys, [q[:M] for q in sc.qmins], sc.x[:M], sc.y[:M], sc.head[:M], sc.v[:M],
                                      sc.arc[:M], sc.a_brake, sc.dt, sc.thr, sc.map_of, 5, rows, speed_of, 0b11111, lens=lens, finite=finite)
            assert rc == 0, msg
            _assert_written(out, (M, lens is None))
            if finite is not None:
                assert (out.user[finite == 0] == -2).all() and (out.harm[finite == 0] == 1.0).all() and (out.user[finite == 1] >= -1).all()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_of_the_c_entry(torch_cuda):
    torch = torch_cuda
    from frenetix_occlusion import _native as N
    sm, _ = UG._parked()
    h = LC.hand_case(8.0, 4.0, 10.0, NORTH)
    _moves(sm, h.moves)
    cost0, safe0 = np.full((1, 16), 0.5), np.ones(1, dtype=np.uint8)
    base = dict(lens=None, finite=np.ones(1, dtype=np.uint8), cost=cost0, safe=safe0, harm_limit=0.1)

    def call(B=1, thr=h.thr, keys=None, r2=None, map_of=(0,), dir_mask=1, slack=0.0, **kw):
        args = dict(base)
        args.update(kw)
        a_brake, dt = args.pop("a_brake", h.a_brake), args.pop("dt", h.dt)
        return _raw_lanes(torch, sm, h.win, [h.r2_cap] if r2 is None else r2, [h.key] if keys is None else keys,
                          [h.qmin] * (1 if keys is None else len(keys)), h.x, h.y, h.head, h.v, h.arc, a_brake, dt, thr, map_of, B, [LC.CAR_ROW],
                          [LC.CAR_SPEED], dir_mask, slack, **args)

    def refused(what, code=N.FO_E_ARG, **kw):
        rc, msg, out = call(**kw)
        assert rc == code and msg.startswith("fo_scene_hidden_brake_impact_lanes:") and what in msg, (what, rc, msg)
        assert _untouched(out), what
        assert (out.cost is None or (out.cost == 0.5).all()) and (out.safe is None or (out.safe == 1).all()), what

    rc, msg, out = call()
    assert rc == N.FO_OK and abs(out.cosine[0, 0] - LC.COS_67_5) <= 1e-15 and out.cost[0, RI.C_RES0] == out.harm[0, 0], msg
    # the new refusals
    refused("dir_mask", dir_mask=0b10)
    refused("dir_mask", dir_mask=0x80000000)
    for bad in (float("nan"), float("inf"), 1.5, -1.0000001):
        refused("cos_h", cos_h=bad)
        refused("cos_h", sin_h=bad)
    for name in ("d_harm", "d_user", "d_closing", "d_cosine", "d_at", "d_commit", "d_first"):
        refused("d_closing", drop=(name,))
    assert FG._set_moves(sm, None) == N.FO_OK                                            # no move table
    refused("move table", code=N.FO_E_STATE)
    rc, msg, out = call(dir_mask=0)                                                     # ... which nobody reads without a lane-bound class
    assert rc == N.FO_OK and out.cosine.tolist() == [[1.0]] and out.closing.tolist() == [[17.9]], msg
    _moves(sm, h.moves)
    # those of the head-on entry, through the one set of checks
    refused("harm_limit", harm_limit=-0.5)
    refused("harm_limit", harm_limit=float("nan"))
    refused("d_speed_of", drop=("d_speed_of",))
    refused("d_speed_of", drop=("d_harm_rows",))
    refused("B = 0", B=0)
    refused("B = 17", B=h.T + 1)
    refused("go together", cost=None)
    refused("go together", safe=None)
    refused("K = 0", K=0)
    refused("K = 4", K=4)
    refused("C = 0", C=0, dir_mask=0)
    refused("C = 9", C=9)
    refused("h_thr", h_thr=None)
    refused("window", win_nx=0)
    refused("r2_cap[0]", r2=[-1])
    refused("map_of[0] = 1", map_of=(1,))
    refused("M = -1", M=-1)
    refused("a_brake", a_brake=float("nan"))
    refused("dt", dt=0.0)
    refused("T = 255", T=255)
    refused("decreases", thr=np.array([[5, 4] + [9] * (h.T - 2)]))
    refused("lies beyond", thr=h.thr + 169 * (h.r2_cap + 1))
    for name in ("d_x", "d_y", "d_heading"):
        refused("d_x", drop=(name,))
    refused("d_key[0]", drop_map=(("d_key", 0),))
    refused("d_v", drop=("d_arc",))
    refused("half extents", hl=-0.1)
    rc, msg, out = call(M=0)
    assert rc == N.FO_OK and _untouched(out)
    ctx = N.Context(0)                                                                  # a context without a map
    assert ctx._lib.fo_scene_hidden_brake_impact_lanes(ctx._h, C.byref(N.HiddenBrakeImpactLanes()), None) == N.FO_E_STATE


def test_refusals_of_the_python_layer(torch_cuda):
    torch = torch_cuda
    k = VG._stack(torch)
    k.sm.launch(k.sc.ego, k.sc.yaw)
    call = lambda **over: k.sm.hidden_brake_impact(*k.tr[:4], **_iv(**over))
    for bad in (dict(approach="sideways"), dict(approach=None), dict(heading_slack=-0.1), dict(heading_slack=float("nan")),
                dict(heading_slack=float("inf")), dict(heading_slack="wide"), dict(approach="head_on", heading_slack=-1.0)):
        with pytest.raises(ValueError, match="hidden_brake_impact"):
            call(**bad)
    moves, k.sm.lane_moves = k.sm.lane_moves, None
    try:
        with pytest.raises(ValueError, match="lane_moves"):
            call()
        call(users=tuple((s, m, "any") for s, m, _ in LANE_USERS))     # nobody is lane-bound: served without a table
    finally:
        k.sm.lane_moves = moves
    torch.cuda.synchronize()
    iv = call(heading_slack=4.0)                                       # h >= pi: head-on for everybody
    torch.cuda.synchronize()
    assert (iv.cosine == 1.0).all()
