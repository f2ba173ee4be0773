"""Scenes for the tests of the brake ladder by road users (DESIGN.md §5.10 "Brake ladder by road users"), shared by
tests/test_hidden_brake_ladder_users_cpu.py -- which holds the checker alone to conditions on them, so that a degenerate scene cannot
hide a failure -- and tests/test_hidden_brake_ladder_users_gpu.py, which runs the same scenes on the device.  The scenes are
tests/hidden_brake_users_scenes.user_scene's (the fans and class bytes of tests/hidden_brake_scenes.py, every forecast's key map and
clearance by the checkers) with the ladders of tests/hidden_brake_ladder_scenes.levels_of and a number of brake starts."""
import functools

import numpy as np

import hidden_brake_ladder_scenes as LS
import hidden_brake_scenes as SC
import hidden_brake_users_scenes as US
import ref_hidden_brake_ladder_users as LU
import ref_hidden_clearance as HC

# eight speeds (scaled by the horizon as in hidden_brake_classes_scenes.speeds_for): unsorted, one repeated, a motionless class
SPEEDS8 = (8.0, 1.5, 0.0, 4.0, 4.0, 6.5, 0.25, 2.0)
FORECASTS = (("road", "lanes"), ("euclid", "any"), ("road", "any"))
# how the classes name their maps: K, map_of[c], and the forecast behind each map handed over.  "same": two maps that are the same
# buffer; "gap": three maps of which no class names the middle one
LAYOUTS = {
    "1": (1, lambda c: 0, (0,)),
    "2": (2, lambda c: c % 2, (0, 1)),
    "3": (3, lambda c: (c + 1) % 3, (0, 1, 2)),
    "same": (2, lambda c: c % 2, (2, 2)),
    "gap": (3, lambda c: 2 * (c % 2), (0, 1, 2)),
}

# (seed, M, T, ragged, C, layout, L, B): the smallest shapes at which the launch plan (csrc/fo_scene_plan.hpp brake_ladder_users_*)
# changes form.  Lp = the power of two >= L lanes per (m, b); G = the power of two >= min(B Lp, 256) lanes per trajectory, doubled while
# the 256 / G trajectories of a workgroup need more than 32 KB of rows (T (48 + 4 K) bytes each); per = 256 / G.
SCENES = [
    (124, 3, 31, False, 5, "3", 23, 31),    # the interface's default ladder from every start: Lp = 32, G = 256, per = 1, 4 rounds
    (35, 70, 31, True, 4, "2", 2, 1),       # B = 1, L = 2: the rows decide, G = 16, per = 16 -- five workgroups, the last one part full
    (32, 3, 31, True, 8, "gap", 33, 1),     # Lp = 64 with 31 padded lanes, G = 64, per = 4: a workgroup with one subgroup idle
    (33, 1, 31, False, 1, "1", 64, 31),     # every lane a level, G = 256, 8 rounds; one class (width 4, three absent)
    (21, 70, 2, True, 5, "same", 1, 2),     # T = 2 = B, L = 1: G = 2, per = 128; the commit shuffle over two lanes
    (22, 3, 2, False, 8, "3", 64, 1),       # T = 2, B = 1: no pose but the first
    (51, 3, 33, True, 4, "3", 2, 33),       # B Lp = 66: G = 128, per = 2 -- a trajectory over two waves, commit through LDS
    (52, 1, 33, False, 5, "2", 23, 1),      # G = 32, per = 8 with one trajectory
    (81, 2, 254, False, 3, "3", 2, 1),      # T = 254: two trajectories' rows are 30 KB, G = 128 by the rows alone; C T = 762
    (53, 3, 33, False, 4, "1", 5, 33),      # Lp = 8, G = 256: 32 brake starts a round, two rounds, the second with one start
    (91, 1, 100, False, 8, "3", 48, 1),     # 4 * 8 * 100 + 8 * 48 = 3 584 bytes: the kernel argument filled to its last byte
]


def expected_plan(T, K, C, L, B):
    """(Lp, G, per_block, lds_bytes): the Python restatement of csrc/fo_scene_plan.hpp's brake_ladder_users_* functions"""
    Lp = 1
    while Lp < L:
        Lp *= 2
    G = Lp
    while G < 256 and G < B * Lp:
        G *= 2
    while G < 256 and (256 // G) * T * (48 + 4 * K) > 32768:
        G *= 2
    per = 256 // G
    return Lp, G, per, per * T * (48 + 4 * K) + 4 * C * T + 4 * C * 256


def arrival_of(key, thr_row):
    """the arrival map of one class behind its key map, by the tie ``A <= j iff key <= thr[j]`` (uint8, 255 = never)"""
    key, thr_row = np.asarray(key, dtype=np.int64), np.asarray(thr_row, dtype=np.int64)
    A = np.searchsorted(thr_row, key.ravel(), side="left").reshape(key.shape)      # the first j with thr[j] >= key (thr does not decrease)
    return np.where(A < len(thr_row), A, 255).astype(np.uint8)


def scene(seed, M, T, ragged, C, layout, L, B):
    """the scene of a spec: ``keys``, ``qmins`` [K] by the checkers (every forecast at the cap of the fastest class, so that any class
    may be held against any map), ``thr [C, T]``, ``map_of``, ``r2_caps``, ``levels``, ``starts``"""
    sc = US.user_scene((seed, M, T, 0, ragged), tuple((s, "road", "any") for s in SPEEDS8[:C]), maps=False)
    K, of, behind = LAYOUTS[layout]
    cap = sc.r2_caps[0]
    made = {f: US.forecast_maps(sc, FORECASTS[f], cap) for f in sorted(set(behind))}
    sc.keys, sc.qmins = [made[f][0] for f in behind], [made[f][1] for f in behind]      # ("same": the very same arrays twice)
    sc.map_of, sc.r2_caps = [of(c) for c in range(C)], [cap] * K
    sc.levels, sc.starts = LS.levels_of(L), B
    return sc


def hand_scene():
    """the hand case of tests/test_hidden_brake_ladder_users_cpu.py on the road of tests/hidden_brake_scenes.py, for the device: three
    candidates drive east along y = 0 at 8 m/s (0.8 m a sample, T = 31) from x = 0, 0.3 and -2; the ladder is 0, 3, 8 m/s^2.  As in the
    hand case a cell's key is the SAMPLE at which hidden traffic reaches it and thr[c][j] = j.  Map 0: the band 12 <= x < 13 is
    reached at sample 20 and nothing else ever.  Map 1: the road from x = 22 on is hidden from the start.  The vehicle reaches from
    0.83 m behind its reference point to 3.68 m in front of it.  Candidate 0 from b = 0: without braking its rear is at 15.17 at sample
    20, past the band, and its front meets x = 22 at sample 23, moving; at 3 m/s^2 it lies over 9.47 .. 13.98 at sample 20, in the
    band and moving until sample 27, and never gets beyond 14.8; at 8 m/s^2 its front stays short of 8.1.  User 0 (map 0): unclear =
    no, YES, no; user 1 (map 1): YES, no, no; required_all = 2, above both users' own 0 and 1"""
    from types import SimpleNamespace
    M, T = 3, 31
    win = SC.WINDOWS[0]
    x = np.array([0.0, 0.3, -2.0])[:, None] + 0.8 * np.arange(T)[None]
    y = np.zeros((M, T))
    head = np.zeros((M, T, 2))
    head[..., 0] = 1.0
    col = lambda wx: int((wx - SC.ORIGIN[0]) / SC.CS) - win[0]
    keys = [np.full((win[3], win[2]), HC.NONE, dtype=np.int64) for _ in range(2)]
    keys[0][:, col(12.0):col(13.0)] = 20
    keys[1][:, col(22.0):] = 0
    road = SC.road_raster()
    qmins = [np.asarray(HC.clearance(k, win, road, SC.ORIGIN, SC.CS, x, y, head, SC.HL, SC.HW, SC.WB)) for k in keys]
    return SimpleNamespace(M=M, T=T, win=win, road=road, x=x, y=y, head=head, v=np.full((M, T), 8.0), arc=SC.travelled_arc(x, y), lens=None,
                           dt=SC.DT, keys=keys, qmins=qmins, thr=np.tile(np.arange(T, dtype=np.int64), (2, 1)), map_of=[0, 1], r2_caps=[1, 1],
                           levels=np.array([0.0, 3.0, 8.0]), starts=T)


def check(sc, keys=None, qmins=None, v=None, arc=None):
    """the checker on a scene, or on edited data of it"""
    pick = lambda given, own: getattr(sc, own) if given is None else given
    return LU.ladder_users(pick(keys, "keys"), sc.win, sc.road, pick(qmins, "qmins"), SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, pick(arc, "arc"),
                           pick(v, "v"), SC.HL, SC.HW, SC.WB, sc.levels, sc.starts, sc.dt, sc.thr, sc.map_of, sc.lens)


@functools.lru_cache(maxsize=None)
def checked(spec):
    """(scene, the checker's LadderUsers): computed once per process, shared by the tests, never changed"""
    sc = hand_scene() if spec == "hand" else scene(*spec)
    return sc, check(sc)
