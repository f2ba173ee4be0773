"""CPU side of the extended future-visibility sweep (fo_scene_future_visibility_ex): the NumPy checker of
tests/ref_future_visibility.py against the C oracle, FOObstacles.rows_at against update, the packing of a predictions dict
into occluder slices, and the ctypes mirror of fo_future_visibility_t against the header."""
import math
import os

import numpy as np
import pytest

import ref_future_visibility as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load(name):
    from frenetix_occlusion import scenario as S
    if name == "city":
        return S.synthetic_urban_grid()
    return S.load_geometry_npz(os.path.join(GOLDEN, f"{name}_geometry.npz"))


@pytest.mark.parametrize("name", ["scenario1", "scenario3", "city"])
def test_checker_equals_the_c_oracle_on_one_slice(oracle, name):
    """full circle, world-aligned, one slice: counts bit-for-bit and areas to 1e-12 against fo_oracle_future_visibility"""
    from frenetix_occlusion import scenario as S, synthetic as SY
    from frenetix_occlusion.sensor_model import ray_dirs
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    sc = _load(name)
    ego = sc.ego_initial
    edges = S.MapGeometry.from_lanelets(sc.lanelets).edges
    ob = FOObstacles(sc.obstacles)
    ob.update(0)
    corn, _, flags = ob.arrays()
    # an occluded list of the shape the visibility stage leaves: ascending indices of a window about the ego
    cs, nx, ny = 0.5, 241, 241
    rx0, ry0 = float(np.floor(ego[0])) - 60.0, float(np.floor(ego[1])) - 60.0
    rng = np.random.default_rng(5)
    occ = np.sort(rng.choice(nx * ny, 4000, replace=False)).astype(np.int32)
    traj = SY.make_trajectories(5, seed=3, ego_pos=ego[:2], ego_yaw=float(ego[2]))
    dirs = ray_dirs(192)
    ref_rev, ref_area = oracle.future_visibility(traj["x"], traj["y"], 5, dirs, 50.0, edges, corn, flags, occ, rx0, ry0, cs,
                                                 0, 0, nx)
    rev, area, new, any_ = RF.future_visibility(traj["x"], traj["y"], 5, dirs, 50.0, edges, corn[None], flags[None], occ,
                                                rx0, ry0, cs, 0, 0, nx)
    assert ref_rev.max() > 0
    assert np.array_equal(rev, ref_rev)
    np.testing.assert_allclose(area, ref_area, rtol=1e-12, atol=1e-9)
    assert np.array_equal(new.sum(axis=1), any_) and (any_ >= rev.max(axis=1)).all() and (any_ <= len(occ)).all()


def test_checker_sector_is_inside_the_full_circle():
    """an open fan counts a subset of what the full circle about the same pose counts, and nothing behind the pose"""
    from frenetix_occlusion import scenario as S
    from frenetix_occlusion.sensor_model import ray_dirs
    sc = _load("scenario1")
    ego = sc.ego_initial
    edges = S.MapGeometry.from_lanelets(sc.lanelets).edges
    cs, nx = 0.5, 201
    rx0, ry0 = float(ego[0]) - 50.25, float(ego[1]) - 50.25
    occ = np.arange(nx * nx, dtype=np.int32)[::7]
    x, y = np.full((1, 1), ego[0]), np.full((1, 1), ego[1])
    head = np.array([[[math.cos(ego[2]), math.sin(ego[2])]]])
    empty_c, empty_f = np.zeros((1, 0, 4, 2)), np.zeros((1, 0), np.uint8)
    full, _, _, _ = RF.future_visibility(x, y, 1, ray_dirs(720), 50.0, edges, empty_c, empty_f, occ, rx0, ry0, cs, 0, 0, nx)
    sec, a_sec, _, _ = RF.future_visibility(x, y, 1, ray_dirs(257, 0.0, 120.0), 50.0, edges, empty_c, empty_f, occ, rx0, ry0,
                                            cs, 0, 0, nx, full=False, heading=head)
    assert 0 < sec[0, 0] < full[0, 0] and a_sec[0, 0] > 0
    d = RF.pose_fan(ray_dirs(257, 0.0, 120.0), head[0, 0])
    assert (d @ head[0, 0] > 0.4999).all()     # every ray within 60 deg of the heading


def _rows_of_update(obstacles, t):
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    ob = FOObstacles(obstacles)
    ob.update(t)
    corn, _, flags, _, _ = ob.arrays_full()
    return np.array(corn, dtype=np.float64).reshape(len(ob), 4, 2), np.array(flags, dtype=np.uint8)


@pytest.mark.parametrize("helper", [True, False])
def test_rows_at_is_what_update_writes(monkeypatch, helper):
    from frenetix_occlusion.utils import fo_obstacle
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    if not helper:
        monkeypatch.setattr(fo_obstacle, "_pyhost", lambda: None)
    elif fo_obstacle._pyhost() is None:
        pytest.fail("the C helper was not built")
    sc = _load("scenario1")
    last = max(o.initial_time_step + len(o.states) for o in sc.obstacles if o.role != "static")
    ts = [0, last // 2, last + 7]
    ob = FOObstacles(sc.obstacles)
    ob.update(0)
    before = [a.copy() for a in ob.arrays_full()]
    corn, flags = ob.rows_at(ts)
    for a, b in zip(before, ob.arrays_full()):         # nothing moved
        assert np.array_equal(a, b)
    assert corn.shape == (3, len(ob), 4, 2) and flags.shape == (3, len(ob))
    for i, t in enumerate(ts):
        c, f = _rows_of_update(sc.obstacles, t)
        assert corn[i].tobytes() == c.tobytes() and np.array_equal(flags[i], f), t
    assert not np.array_equal(corn[0], corn[1])         # the cars drive
    assert (flags[2] & 1).sum() < (flags[0] & 1).sum()  # and leave


def test_predictions_dict_packs_into_slices():
    from frenetix_occlusion.utils.fo_obstacle import FOObstacles
    sc = _load("scenario1")
    ob = FOObstacles(sc.obstacles)
    ob.update(0)
    corn0, _, flags0, _, _ = ob.arrays_full()
    o = ob.fo_obstacles[0]
    pos = np.array([[10.0, 20.0], [11.0, 20.5], [12.5, 21.0]])
    ori = np.array([0.1, 0.2, 0.3])
    preds = {o.obstacle_id: {"pos_list": pos, "orientation_list": ori}, 10 ** 9: {"pos_list": pos, "orientation_list": ori}}
    samples = [0, 1, 2, 5]
    corn, flags = ob.predicted_rows(preds, samples)
    assert corn.shape == (4, len(ob), 4, 2) and flags.shape == (4, len(ob))
    for s, j in enumerate(samples):
        jj = min(j, 2)
        want = o._o.corners((pos[jj, 0], pos[jj, 1], ori[jj]))
        assert corn[s, 0].tobytes() == want.tobytes()
        assert flags[s, 0] & 3 == 3
        # obstacles without a prediction stay where they are
        assert corn[s, 1:].tobytes() == np.asarray(corn0)[1:].tobytes() and np.array_equal(flags[s, 1:], flags0[1:])
    # the corner formula with the obstacle's own dimensions: side lengths are its length and width
    c = corn[0, 0]
    assert math.isclose(np.hypot(*(c[2] - c[1])), o.length, rel_tol=1e-12)
    assert math.isclose(np.hypot(*(c[1] - c[0])), o.width, rel_tol=1e-12)
    none_c, none_f = ob.predicted_rows(None, [0, 5])
    assert np.array_equal(none_c[1], corn0) and np.array_equal(none_f[1], flags0)


def test_ctypes_struct_has_the_layout_of_the_header(tmp_path):
    """the ctypes mirror of fo_future_visibility_t against what a C compiler makes of include/fo_hip.h"""
    import ctypes as C
    import subprocess
    from frenetix_occlusion import _native as native
    fields = [n for n, *_ in native.FutureVisibility._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fo_hip.h"', 'int main(void) {',
             'printf("%zu %d\\n", sizeof(fo_future_visibility_t), FO_FUTURE_VISIBILITY_MAX_CELLS);']
    lines += ['printf("%%zu\\n", offsetof(fo_future_visibility_t, %s));' % f for f in fields]
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out[:2]] == [C.sizeof(native.FutureVisibility), native.FUTURE_VISIBILITY_MAX_CELLS]
    assert [int(v) for v in out[2:]] == [getattr(native.FutureVisibility, f).offset for f in fields]
    assert "fo_scene_future_visibility_ex" in native.EXPORTS
