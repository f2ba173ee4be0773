"""Scenes for the brake ladder's tests (DESIGN.md §5.10 "Brake ladder"), shared by tests/test_hidden_brake_ladder_cpu.py -- which
holds the checker alone to conditions on them, so that a degenerate scene cannot hide a failure -- and
tests/test_hidden_brake_ladder_gpu.py, which runs the same scenes on the device.  The scenes themselves are
tests/hidden_brake_scenes.scene's; a ladder scene adds the levels and the number of brake starts."""
import functools

import numpy as np

import hidden_brake_scenes as SC
import ref_hidden_brake_ladder as L

FULL_LADDER = np.linspace(0.5, 11.5, 23)       # 0.5, 1.0, ..., 11.5 m/s^2: the interface's default at a_max = 11.5


def levels_of(K):
    """the ladder of K levels: ``np.linspace(0.5, 11.5, K)``, ``[8.0]`` for K = 1"""
    return np.array([8.0]) if K == 1 else np.linspace(0.5, 11.5, K)


# the six scenes the conditions are stated for, (seed, M, T, entry, ragged) of tests/hidden_brake_scenes.RANDOM_SCENES, on the full
# ladder from every brake start
CONDITION_SCENES = [(31, 7, 31, 2, False), (32, 8, 31, 0, True), (33, 9, 31, 1, False), (35, 70, 31, 1, True), (51, 3, 33, 1, False),
                    (62, 4, 64, 0, False)]

# (seed, M, T, entry, ragged, K, B): the switch points of the launch plan (csrc/fo_scene_plan.hpp brake_ladder_*).  Kp = the power
# of two >= K lanes per (m, b); G = the power of two >= min(B Kp, 256) lanes per trajectory, doubled while the 256 / G trajectories
# of a workgroup need more than 32 KB of rows (48 T bytes each); per = 256 / G.  M takes the three values around `per`.
#   K over {1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64}, B over {1, a middle value, T}, T over {1, 2, 31, 33, 64, 65, 254}
SHAPE_SCENES = [
    # T = 1: one brake start, no pose at all.  K = 1: G = 1, per = 256
    (11, 255, 1, 0, False, 1, 1), (12, 256, 1, 1, True, 1, 1), (13, 257, 1, 2, False, 1, 1),
    # T = 2, K = 2, B = 2: G = 4, per = 64
    (21, 63, 2, 1, False, 2, 2), (22, 64, 2, 2, True, 2, 2), (23, 65, 2, 0, False, 2, 2),
    # T = 2, K = 1, B = 2: G = 2, per = 128 (the commit shuffle over two lanes); K = 5 (Kp = 8), B = 1: G = 8, per = 32
    (24, 127, 2, 0, False, 1, 2), (25, 128, 2, 1, True, 1, 2), (26, 129, 2, 2, False, 1, 2),
    (27, 31, 2, 2, False, 5, 1), (28, 32, 2, 0, True, 5, 1), (29, 33, 2, 1, False, 5, 1),
    # T = 31, K = 4, B = 1: the lanes ask for G = 4 (per = 64), the rows allow per = 16 (G = 16): the LDS cap decides
    (31, 15, 31, 2, False, 4, 1), (32, 16, 31, 0, True, 4, 1), (33, 17, 31, 1, False, 4, 1),
    # T = 33, K = 5 (Kp = 8), B = 4: G = 32, per = 8; K = 3 (Kp = 4), B = 16: G = 64, per = 4
    (51, 7, 33, 1, False, 5, 4), (52, 8, 33, 2, False, 5, 4), (53, 9, 33, 0, True, 5, 4),
    (54, 3, 33, 0, True, 3, 16), (55, 4, 33, 1, False, 3, 16), (56, 5, 33, 2, False, 3, 16), (57, 2, 33, 1, False, 2, 33),
    # a trajectory over two waves (G = 128, per = 2): K = 64, B = 2; K = 9 (Kp = 16), B = 8; K = 17 (Kp = 32), B = 3 (a padded round)
    (34, 1, 31, 0, False, 64, 2), (35, 2, 31, 1, True, 64, 2), (36, 3, 31, 2, False, 64, 2),
    (37, 3, 31, 1, True, 9, 8), (38, 3, 31, 0, False, 17, 3),
    # ... and over four (G = 256, per = 1): K = 63, 33 and 32 lanes of 64, 64 and 32; B = T with rounds of 8, 16 and 32 brake starts
    (41, 2, 31, 0, True, 63, 4), (42, 1, 31, 1, False, 33, 5), (43, 2, 31, 2, False, 32, 31), (44, 3, 31, 0, True, 16, 31),
    (45, 2, 31, 1, False, 8, 31), (46, 1, 31, 0, False, 8, 31),
    # T = 64 and 65 (at Kp = 4 a round holds 64 brake starts: one round, and two), B in the middle and at T
    (62, 2, 64, 0, False, 4, 64), (63, 2, 64, 1, True, 2, 33), (71, 2, 65, 0, False, 3, 65), (72, 3, 65, 1, True, 1, 32),
    # T = 254: two trajectories' rows are 24 KB; K = 1, B = 1 leaves one lane of 128 with work; B = T walks 254 brake starts
    (81, 1, 254, 1, False, 1, 1), (82, 2, 254, 0, False, 1, 1), (83, 3, 254, 2, True, 1, 1), (84, 1, 254, 1, False, 2, 254),
    (85, 2, 254, 0, True, 5, 100),
]


def expected_plan(T, K, B):
    """(Kp, G, per_block, lds_bytes): the Python restatement of csrc/fo_scene_plan.hpp's brake_ladder_* functions"""
    Kp = 1
    while Kp < K:
        Kp *= 2
    G = Kp
    while G < 256 and G < B * Kp:
        G *= 2
    while G < 256 and (256 // G) * 48 * T > 32768:
        G *= 2
    per = 256 // G
    return Kp, G, per, per * 48 * T + 1024


def scene(seed, M, T, entry, ragged, K=23, B=None):
    sc = SC.scene(seed, M, T, entry, ragged)
    sc.levels = FULL_LADDER if K == 23 else levels_of(K)
    sc.starts = T if B is None else B
    return sc


@functools.lru_cache(maxsize=None)
def checked(spec):
    """(scene, A, first, the checker's five outputs) of a scene on the CPU forecast's own map: computed once per process"""
    sc = scene(*spec)
    A, _, first = SC.arrival_and_first(sc)
    ref = L.ladder(A, sc.win, sc.road, first, SC.ORIGIN, SC.CS, sc.x, sc.y, sc.head, sc.arc, sc.v, SC.HL, SC.HW, SC.WB, sc.levels,
                   sc.starts, sc.dt, sc.lens)
    return sc, A, first, ref
