"""Occlusion memory without a GPU: the NumPy model of the definition on hand-built windows, the host's
reset rules against it, the configuration block and the ctypes mirror of fo_occlusion_memory_t."""
import math
import os

import numpy as np
import pytest

import ref_occlusion_memory as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROAD, VIS, OCC = 1, 2, 4


def _strip(n=12):
    """a road strip on raster rows 0..2, columns 0..n-1; nothing else is road"""
    road = np.zeros((6, n), dtype=np.uint8)
    road[0:3, :] = 1
    return road


def test_seen_cell_stays_cleared_until_the_reach_arrives_from_unobserved_road():
    road = _strip(12)
    win = (0, 0, 12, 6)
    cls = np.where(road[:, :] != 0, ROAD, 0).astype(np.uint8)
    # step 0: columns 0..5 of the strip visible, 6..11 road outside range (a source)
    c0 = cls.copy()
    c0[0:3, 0:6] |= VIS
    H0, out0 = R.step(c0, win, road, 0)
    assert np.array_equal(out0, c0)
    assert H0[0:3, 0:6].sum() == 0 and H0[0:3, 6:].all()
    # step 1: columns 0..4 hidden behind a parked car (occluded), 5 still visible; reach of 2 cells
    c1 = cls.copy()
    c1[0:3, 0:5] |= OCC
    c1[0:3, 5] |= VIS
    H1, out1 = R.step(c1, win, road, 4, H0, win)
    # nothing unobserved within two cells of columns 0..4 (column 6 is three cells from column 3 ... 4 is two from 6)
    assert (out1[0:3, 0:4] & OCC).sum() == 0
    assert (out1[0:3, 4] & OCC).all()          # (6 - 4)^2 = 4 <= R2: a road user from column 6 can be there
    assert np.array_equal(H1[0:3, 4], [1, 1, 1]) and H1[0:3, 0:4].sum() == 0
    # step 2: the same classes; the hidden set grows by the reach per step
    H2, out2 = R.step(c1, win, road, 4, H1, win)
    assert (out2[0:3, 2:5] & OCC).all() and (out2[0:3, 0:2] & OCC).sum() == 0
    H3, out3 = R.step(c1, win, road, 4, H2, win)
    assert (out3[0:3, 0:5] & OCC).all()


def test_cells_that_leave_the_window_count_as_road_sources():
    road = _strip(20)

    def seen(win):
        ix0, iy0, nx, ny = win
        c = np.where(road[iy0:iy0 + ny, ix0:ix0 + nx] != 0, ROAD, 0).astype(np.uint8)
        c[(c & ROAD) != 0] |= VIS
        return c
    w0, w1 = (0, 0, 8, 6), (4, 0, 8, 6)
    H0, _ = R.step(seen(w0), w0, road, 0)
    assert H0.sum() == 0
    # the window moves right by four cells: raster columns 0..3 leave it; everything in it is seen
    H1, _ = R.step(seen(w1), w1, road, 1, H0, w0)
    assert H1.sum() == 0
    # back to the first window with raster column 4 occluded: column 3 left the previous window, so it is unobserved road
    # and a source one cell away; column 5 was seen (H1 = 0)
    c2 = seen(w0)
    c2[0:3, 4] = ROAD | OCC
    c2[0:3, 5] = ROAD | OCC
    H2, out2 = R.step(c2, w0, road, 1, H1, w1)
    assert (out2[0:3, 4] & OCC).all() and H2[0:3, 4].all()
    assert (out2[0:3, 5] & OCC).sum() == 0 and H2[0:3, 5].sum() == 0
    # without the move (previous window = this one, everything seen) neither stays occluded
    H2b, out2b = R.step(c2, w0, road, 1, np.zeros((6, 8), dtype=np.uint8), w0)
    assert (out2b & OCC).sum() == 0


def test_outside_previous_window_is_a_source():
    road = _strip(20)
    w1 = (6, 0, 8, 6)
    c1 = np.where(road[0:6, 6:14] != 0, ROAD, 0).astype(np.uint8)
    c1[0:3, 0] |= OCC
    c1[0:3, 1:] |= VIS
    # the previous window covered raster columns 6..13 only, all seen: column 5 was never observed
    H0 = np.zeros((6, 8), dtype=np.uint8)
    H1, out1 = R.step(c1, w1, road, 1, H0, (6, 0, 8, 6))
    assert (out1[0:3, 0] & OCC).all() and H1[0:3, 0].all()
    # the same with the previous window shifted left over column 5 (seen there): cleared
    H0s = np.zeros((6, 8), dtype=np.uint8)
    H1s, out1s = R.step(c1, w1, road, 1, H0s, (2, 0, 8, 6))
    assert (out1s[0:3, 0] & OCC).sum() == 0 and H1s[0:3, 0].sum() == 0


def test_non_road_cells_are_never_sources():
    road = np.zeros((7, 7), dtype=np.uint8)
    road[3, 3] = 1                                 # one road cell surrounded by off-road
    win = (0, 0, 7, 7)
    c = np.zeros((7, 7), dtype=np.uint8)
    c[3, 3] = ROAD | OCC
    prev = np.zeros((7, 7), dtype=np.uint8)        # previous step: the road cell seen
    H, out = R.step(c, win, road, 8, prev, win)
    assert out[3, 3] == ROAD and H.sum() == 0
    # off-road cells outside the previous window and outside the raster are no sources either
    H2, out2 = R.step(c, win, road, 8, np.zeros((1, 1), dtype=np.uint8), (3, 3, 1, 1))
    assert out2[3, 3] == ROAD


def test_r2_boundary_is_inclusive_and_integer():
    road = np.ones((1, 12), dtype=np.uint8)
    win = (0, 0, 12, 1)
    prev = np.zeros((1, 12), dtype=np.uint8)
    prev[0, 0] = 1                                 # the only source: raster column 0
    c = np.full((1, 12), ROAD, dtype=np.uint8)
    c[0, 5] |= OCC
    for r2, kept in ((24, False), (25, True)):     # dx^2 = 25 exactly
        H, out = R.step(c, win, road, r2, prev, win)
        assert bool(out[0, 5] & OCC) == kept, r2
    assert (3, 4) in R.offsets(25) and (0, 5) in R.offsets(25) and (1, 5) not in R.offsets(25)
    # R2 = floor(rho^2 / cs^2) in float64: a reach of exactly 2.5 m at 0.5 m cells is 25
    assert R.reach_r2(2.0, 1.0, 0.5, 0.5) == 25
    from frenetix_occlusion.sensor_model import occlusion_memory_r2
    for v, dt, m, cs in ((13.9, 0.1, math.sqrt(2) * 0.5, 0.5), (2.0, 1.0, 0.5, 0.5), (13.9, 0.3, 0.0, 0.25), (0.0, 0.1, 0.0, 0.5)):
        assert occlusion_memory_r2(v, dt, m, cs) == R.reach_r2(v, dt, m, cs)


def test_reset_is_the_memoryless_classes():
    rng = np.random.default_rng(5)
    road = (rng.random((30, 30)) < 0.7).astype(np.uint8)
    win = (3, 4, 20, 20)
    c = np.where(road[4:24, 3:23] != 0, ROAD, 0).astype(np.uint8)
    c[(c & ROAD) != 0] |= rng.choice(np.array([0, VIS, OCC], dtype=np.uint8), size=int((c & ROAD).sum()))
    H, out = R.step(c, win, road, 0)
    assert np.array_equal(out, c)
    assert np.array_equal(H, np.where((c & VIS) != 0, 0, c & ROAD))


@pytest.mark.parametrize("impl", ["model", "host"])
def test_every_reset_rule(impl):
    from frenetix_occlusion.sensor_model import OcclusionMemoryPlan
    if impl == "model":
        m = R.Memory(13.9, 0.1, 0.5)
        plan = m.plan

        def commit(t):
            m.prev, m.explicit = (None, None), False
            if t is not None:
                m.t = t
        reset = m.reset
    else:
        p = OcclusionMemoryPlan(13.9, None, 0.5, 0.1)
        plan, commit, reset = p.next_step, p.commit, p.reset
    assert plan(0) == (0, "first")
    commit(0)
    r2 = R.reach_r2(13.9, 0.1, math.sqrt(2) * 0.5, 0.5)
    assert plan(1) == (r2, None) and r2 == 17
    commit(1)
    assert plan(1)[1] == "time" and plan(0)[1] == "time" and plan(None)[1] == "time"
    commit(None)                                   # a step without a timestep: Δt counts from timestep 1
    assert plan(3) == (R.reach_r2(13.9, 0.2, math.sqrt(2) * 0.5, 0.5), None)
    reset()
    assert plan(3) == (0, "explicit")
    commit(3)
    assert plan(4) == (r2, None)
    # reach: sqrt(R2) beyond 32 cells = 16 m at 0.5 m cells; from timestep 3, 11 steps give 13.9 * 1.1 + 0.71 = 15.998 m
    # (R2 = 1023), 12 steps 17.39 m (R2 = 1209)
    assert plan(15)[1] == "reach" and plan(14) == (1023, None)
    assert R.reach_r2(13.9, 1.2, math.sqrt(2) * 0.5, 0.5) > 32 * 32 >= R.reach_r2(13.9, 1.1, math.sqrt(2) * 0.5, 0.5)


def test_config_block_and_defaults(tmp_path):
    import yaml
    from frenetix_occlusion import interface
    with open(os.path.join(ROOT, "frenetix-occlusion_amd", "frenetix_occlusion", "config", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["accelerator"]["occlusion_memory"] == {"enabled": False, "v_max": 13.9, "margin": None}
    assert interface.occlusion_memory_config(cfg["accelerator"]) == {"enabled": False, "v_max": 13.9, "margin": None}
    assert interface.occlusion_memory_config({}) == {"enabled": False, "v_max": 13.9, "margin": None}
    assert interface.occlusion_memory_config(None)["enabled"] is False
    assert interface.occlusion_memory_config({"occlusion_memory": {"enabled": True, "v_max": 5, "margin": 1}}) == \
        {"enabled": True, "v_max": 5.0, "margin": 1.0}
    with pytest.raises(ValueError):
        interface.occlusion_memory_config({"occlusion_memory": {"v_max": -1.0}})
    assert hasattr(interface.FOInterface, "reset_occlusion_memory")
    import inspect
    from frenetix_occlusion.step import PlanningStep
    assert inspect.signature(PlanningStep.run).parameters["timestep"].default is None


def test_ctypes_mirror_has_the_layout_of_the_header(tmp_path):
    import ctypes as C
    import subprocess
    from frenetix_occlusion import _native as N
    fields = [n for n, *_ in N.OcclusionMemory._fields_]
    src = tmp_path / "om_layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fo_hip.h"', 'int main(void) {',
             'printf("%d %zu\\n", FO_OCCLUSION_MEMORY_MAX_HALO, sizeof(fo_occlusion_memory_t));']
    lines += ['printf("%%zu\\n", offsetof(fo_occlusion_memory_t, %s));' % f for f in fields]
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "om_layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == N.OCCLUSION_MEMORY_MAX_HALO == R.MAX_HALO
    assert out[1] == C.sizeof(N.OcclusionMemory)
    assert out[2:] == [getattr(N.OcclusionMemory, f).offset for f in fields]
    assert "fo_scene_set_occlusion_memory" in N.EXPORTS
