"""The scenes of tests/test_scene_forms_gpu.py on the CPU oracle alone: each sits on the switch point it is meant for (piece
count, obstacle count, window size -- tests/scene_forms.py::expected_form) and is not trivial there: something is occluded,
cells are settled by the exact rule (the settle kernel's work), a hole ring is skipped where SKIP is meant, obstacles are
seen by a ray and by a probe only where obstacles are meant.  Prints the facts per scene (pytest -s)."""
import math
import os
import time

import numpy as np
import pytest

import scene_forms as F
from frenetix_occlusion import scenario as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _report(name, s, forced=False, dt=None):
    form = F.expected_form(s["E"], s["O"], s["skipped"] > 0, s["n"] * s["n"], forced)
    print(f"{name}: E={s['E']} chunks={s['chunks']} O={s['O']} n={s['n']} nb={s['nb']} form(NW, SKIP, two_launch)={form} "
          f"n_occ={s['n_occ']} n_exact={s['n_exact']} skipped={s['skipped']}" + ("" if dt is None else f" oracle {dt:.2f} s"))
    return form


def test_expected_form_restates_the_host_rules():
    cells = 301 * 301
    assert F.expected_form(4096, 0, False, cells, False) == (1, False, False)
    assert F.expected_form(4097, 0, False, cells, False) == (5, False, False)
    assert F.expected_form(76, 16, True, cells, False) == (1, True, False)
    assert F.expected_form(76, 17, True, cells, False) == (5, True, False)
    assert F.expected_form(76, 0, False, cells, True) == (5, False, False)
    assert F.expected_form(76, 0, False, 724 * 724, False) == (1, False, False)
    assert F.expected_form(76, 0, True, 725 * 725, True) == (5, True, True)
    # the window edges of SensorModel._window_for: 724 cells is the last one-launch window
    assert {r: (F.window_edge(r), F.n_blocks(F.window_edge(r) ** 2)) for r in F.LARGE_WINDOWS} == F.LARGE_WINDOWS
    assert F.n_blocks(724 * 724) == 2048 and F.n_blocks(725 * 725) == 2054


@pytest.mark.parametrize("name", list(F.L_ROADS))
def test_l_roads_land_on_their_piece_counts_and_reach_the_last_chunk(oracle, name):
    n_main, E, chunks, ego = F.L_ROADS[name]
    geo = F.l_road(n_main)
    assert len(geo.edges) == E and F.n_chunks(E) == chunks
    t = time.perf_counter()
    s = F.oracle_step(oracle, geo, [], ego)
    form = _report(name, s, dt=time.perf_counter() - t)
    assert form == (1 if chunks <= 64 else 5, False, False)
    assert s["n_occ"] > 0 and s["n_exact"] > 0 and s["vis_cells"] > 100      # the arm hides behind the corner (10, -3)
    assert s["hid"].max() // 64 == chunks - 1                                 # a ray ends on a piece of the last chunk
    if chunks > 320:   # every wave of five has hits among the chunks of its second trip
        assert F.second_trip_waves(s["hid"], E) == set(range(5))


@pytest.mark.parametrize("O", [16, 17])
@pytest.mark.parametrize("radius", list(F.FRAME_RADII))
def test_frame_scene_has_every_kind_of_obstacle(oracle, O, radius):
    geo = F.frame_map()
    assert len(geo.edges) == 76 and list(geo.ring_is_hole).count(True) == 1
    seen = {}
    for L in (100.0, math.inf):
        s = F.oracle_step(oracle, geo, F.frame_obstacles(O), F.FRAME_EGO, n_rays=F.FRAME_RAYS, radius=radius, shadow_length=L)
        form = _report(f"frame O={O} r={radius} L={L}", s)
        assert form == (1 if O <= 16 else 5, F.FRAME_RADII[radius], False)
        assert (s["skipped"] > 0) == F.FRAME_RADII[radius]
        assert s["n_occ"] > 0 and s["n_exact"] > 0
        E, vis, flags = s["E"], s["vis"], s["flags"]
        by_ray = set((s["hid"][s["hid"] >= E] - E).tolist())
        assert by_ray and any(vis[o] and o not in by_ray for o in range(O)) and not vis.all()
        assert flags[3] == 0 and flags[2] == 1 and (flags[[0, 1]] == 3).all()   # one absent, one bicycle
        # cell centres in the 5 mm skins of two obstacles at once, outside both rectangles: not visible
        x0, y0, ix0, iy0 = s["frame"]
        px, py = np.meshgrid(x0 + (ix0 + np.arange(s["n"]) + 0.5) * 0.5, y0 + (iy0 + np.arange(s["n"]) + 0.5) * 0.5)
        both = F.in_skin(s["corn"][0], px, py) & F.in_skin(s["corn"][1], px, py)
        both &= ~F.in_skin(s["corn"][0], px, py, 0.0) & ~F.in_skin(s["corn"][1], px, py, 0.0)
        assert both.sum() >= 2 and ((s["cls"][both] & 3) == 1).all()
        seen[L] = s["vis_cells"]
    assert seen[100.0] > seen[math.inf] + 100          # the shadow length decides cells


@pytest.mark.parametrize("O", [16, 17])
def test_frame_in_the_first_two_launch_window_skips_the_block(oracle, O):
    """SKIP and the two-launch compaction in one call: the frame's block is enclosed by a footprint of 120.6 m, the window has
    725 cells per side, and the obstacles' shadows put occluded cells on both sides of the scan kernel's first round"""
    geo = F.frame_map()
    t = time.perf_counter()
    s = F.oracle_step(oracle, geo, F.frame_obstacles(O), F.FRAME_EGO, n_rays=F.FRAME_RAYS, radius=F.FRAME_LARGE_RADIUS)
    form = _report(f"frame O={O} r={F.FRAME_LARGE_RADIUS}", s, dt=time.perf_counter() - t)
    assert (s["n"], s["nb"]) == (725, 2054) and form == (1 if O <= 16 else 5, True, True)
    assert s["skipped"] > 0 and s["n_exact"] > 0
    assert F.scan_rounds(s["occ"]) == {0, 1}
    assert np.array_equal(s["occ"], np.flatnonzero(s["cls"].reshape(-1) & 4))


@pytest.mark.parametrize("radius", list(F.LARGE_WINDOWS))
def test_large_windows_put_occluded_cells_on_both_sides_of_a_scan_round(oracle, radius):
    sc = F.large_window_scene(radius)
    geo = S.MapGeometry.from_lanelets(sc.lanelets)
    t = time.perf_counter()
    s = F.oracle_step(oracle, geo, sc.obstacles, sc.ego_initial, radius=radius)
    form = _report(f"large window r={radius}", s, dt=time.perf_counter() - t)
    n, nb = F.LARGE_WINDOWS[radius]
    assert (s["n"], s["nb"]) == (n, nb) and form == (1, False, nb > 2048)
    assert s["n_occ"] > 0 and s["n_exact"] > 0 and s["O"] > 0
    assert len(F.scan_rounds(s["occ"])) >= 2              # the carry from one 1024-entry round into the next matters
    assert np.array_equal(s["occ"], np.flatnonzero(s["cls"].reshape(-1) & 4))


def test_trusted_scenes_are_not_trivial(oracle):
    """scenario 1 at steps 0 / 25 and scenario 3, which the form tests run in both wave shapes"""
    sc = S.load_geometry_npz(os.path.join(GOLDEN, "scenario1_geometry.npz"))
    geo = S.MapGeometry.from_lanelets(sc.lanelets)
    for step in (0, 25):
        ego = sc.ego_initial.copy()
        ego[:2] += 0.7 * step * np.array([math.cos(ego[2]), math.sin(ego[2])])
        s = F.oracle_step(oracle, geo, sc.obstacles, ego, timestep=step)
        form = _report(f"scenario 1 step {step}", s)
        assert form == (1, step == 0, False) and s["n_occ"] > 0 and s["n_exact"] > 20
        if step == 0:
            assert s["skipped"] == 7
    sc = S.load_geometry_npz(os.path.join(GOLDEN, "scenario3_geometry.npz"))
    s = F.oracle_step(oracle, S.MapGeometry.from_lanelets(sc.lanelets), sc.obstacles, sc.ego_initial)
    assert _report("scenario 3", s)[0] == 1 and s["vis_cells"] > 100
