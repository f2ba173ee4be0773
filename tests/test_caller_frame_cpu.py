"""The caller's curvilinear frame of the spawn rule families (``accelerator.spawn.frame: caller``), host side: the NumPy
frame of the frame model ("The caller's frame"), the table the locator builds from a frame object
(``spawn_locator.caller_frame_table``) and its refusals, ``frame_fit_m``, and the rule checker
(oracle/fo_spawn_rules_ref.py) run through two frames on one curved scene.

``InterpolatedNormalFrame`` transcribes the model operation for operation as csrc/fo_spawn_rules.hpp computes it
(``rl_cf_segment``, ``rl_cf_sd``, ``rl_cf_to_cart``): base points and normals interpolated linearly in s between the
vertices, the CommonRoad style.  tests/test_caller_frame_gpu.py hands it to the device and to the checker."""
import math
import warnings
from types import SimpleNamespace

import numpy as np
import pytest


def _pathlength(p):
    from frenetix_occlusion.utils.curvilinear import pathlength
    return pathlength(p)


class InterpolatedNormalFrame:
    """(s, d) <-> (x, y) about a polyline with a normal per vertex: s_i = the polyline's arc length, b(s) and n(s) linear
    between the vertices, (x, y) = b(s) + d n(s); a point with no root of cross(q - b, n) = 0 on any segment (before the
    first or after the last normal) raises ValueError, like pycrccosy.  ``normals`` default: the normalised average of the
    adjacent segment normals (CommonRoad's choice; the end vertices take their segment's)."""

    def __init__(self, path, normals=None):
        self.path = np.asarray(path, dtype=np.float64)
        self.s = _pathlength(self.path)
        if normals is None:
            seg = np.diff(self.path, axis=0)
            t = seg / np.hypot(seg[:, 0], seg[:, 1])[:, None]
            sn = np.stack((-t[:, 1], t[:, 0]), -1)
            normals = np.concatenate((sn[:1], sn[:-1] + sn[1:], sn[-1:]))
            normals = normals / np.hypot(normals[:, 0], normals[:, 1])[:, None]
        self.normals = np.asarray(normals, dtype=np.float64)
        self.h = np.diff(self.s)

    def _segment(self, i, x, y, best):
        """(squared distance, lambda) of the nearer root of segment i in [0, 1] if nearer than best[0] (the smaller root first)"""
        p, n, p1, n1 = self.path[i], self.normals[i], self.path[i + 1], self.normals[i + 1]
        r0, r1, r4, r5 = float(p[0]), float(p[1]), float(n[0]), float(n[1])
        wx, wy = x - r0, y - r1
        ex, ey, fx, fy = float(p1[0]) - r0, float(p1[1]) - r1, float(n1[0]) - r4, float(n1[1]) - r5
        a = fx * ey - fy * ex
        b = (wx * fy - wy * fx) - (ex * r5 - ey * r4)
        c = wx * r5 - wy * r4
        l1 = math.nan
        if abs(a) <= 1e-12 * abs(b):
            if b == 0.0:
                return None
            l0 = -c / b
        else:
            disc = b * b - 4.0 * a * c
            if not disc >= 0.0:
                return None
            sq = math.sqrt(disc)
            t = -0.5 * (b + (sq if b >= 0.0 else -sq))
            l0 = t / a
            l1 = c / t if t != 0.0 else math.nan
            if l1 < l0:
                l0, l1 = l1, l0
        out = None
        for lam in (l0, l1):
            if lam >= -1e-12 and lam <= 1.0 + 1e-12:
                lam = min(max(lam, 0.0), 1.0)
                px, py = x - (r0 + lam * ex), y - (r1 + lam * ey)
                d2 = px * px + py * py
                if d2 < best:
                    best, out = d2, (d2, lam)
        return out

    def convert_to_curvilinear_coords(self, x, y):
        x, y = float(x), float(y)
        best, k, lam = math.inf, -1, 0.0
        for i in range(len(self.path) - 1):
            r = self._segment(i, x, y, best)
            if r is not None:
                best, lam, k = r[0], r[1], i
        if k < 0:
            raise ValueError("point outside the projection domain")
        p, n, p1, n1 = self.path[k], self.normals[k], self.path[k + 1], self.normals[k + 1]
        bx, by = p[0] + lam * (p1[0] - p[0]), p[1] + lam * (p1[1] - p[1])
        nx, ny = n[0] + lam * (n1[0] - n[0]), n[1] + lam * (n1[1] - n[1])
        px, py = x - bx, y - by
        return np.array([self.s[k] + lam * self.h[k], (px * nx + py * ny) / (nx * nx + ny * ny)])

    def convert_to_cartesian_coords(self, s, d):
        s, d = float(s), float(d)
        if s < self.s[0] or s > self.s[-1]:
            raise ValueError("s outside the reference path")
        k = int(min(np.searchsorted(self.s, s, side="right") - 1, len(self.path) - 2))
        p, n, p1, n1 = self.path[k], self.normals[k], self.path[k + 1], self.normals[k + 1]
        lam = (s - self.s[k]) / self.h[k]
        bx, by = p[0] + lam * (p1[0] - p[0]), p[1] + lam * (p1[1] - p[1])
        nx, ny = n[0] + lam * (n1[0] - n[0]), n[1] + lam * (n1[1] - n[1])
        return np.array([bx + d * nx, by + d * ny])

    def convert_list_of_points_to_curvilinear_coords(self, points, num_threads=1):
        out = []
        for q in points:
            q = np.asarray(q, dtype=np.float64).reshape(-1)
            out.append(self.convert_to_curvilinear_coords(q[0], q[1]))
        return out


def bend_path(radius=8.0, step_deg=30.0, lead=30.0, tail=30.0, left=True):
    """a straight lead-in along +x ending at the origin, a circular bend of 90 deg with a vertex every step_deg, a straight
    tail: the coarse vertices make the polyline frame and the interpolated-normal frame disagree between them"""
    lead_x = np.linspace(-lead, 0.0, int(lead) + 1)
    ang = np.radians(np.arange(step_deg, 90.0 + 1e-9, step_deg))
    sg = 1.0 if left else -1.0
    arc = np.stack((radius * np.sin(ang), sg * radius * (1.0 - np.cos(ang))), -1)
    tail_y = sg * (radius + np.linspace(1.0, tail, int(tail)))
    return np.concatenate((np.stack((lead_x, np.zeros_like(lead_x)), -1), arc,
                           np.stack((np.full_like(tail_y, radius), tail_y), -1)))


def test_round_trip_within_20_m_of_a_curved_path():
    """to_cart(to_curv(q)) = q to 1e-9 m for seeded points within 20 m of a tight bend -- on its inside farther out than the
    radius, several segments have roots (and one segment both of its roots)"""
    path = bend_path(radius=6.0, step_deg=15.0)
    f = InterpolatedNormalFrame(path)
    rng = np.random.default_rng(11)
    done, multi = 0, 0
    centre = np.array([0.0, 6.0])
    for _ in range(600):
        i = int(rng.integers(len(path) - 1))
        base = path[i] + rng.random() * (path[i + 1] - path[i])
        q = base + rng.uniform(-20.0, 20.0, 2)
        if rng.random() < 0.3:        # the inside of the bend, past the centre of curvature
            q = centre + rng.uniform(-3.0, 3.0, 2)
        try:
            s, d = f.convert_to_curvilinear_coords(q[0], q[1])
        except ValueError:
            continue
        np.testing.assert_allclose(f.convert_to_cartesian_coords(s, d), q, rtol=0, atol=1e-9)
        roots = sum(f._segment(k, float(q[0]), float(q[1]), math.inf) is not None for k in range(len(path) - 1))
        multi += roots > 1
        done += 1
    assert done > 400 and multi > 50


def test_the_vertices_project_onto_themselves():
    """every vertex of a path projects in the path's own frame, the last one too (its root is 1 + a rounding error)"""
    from test_spawn_rules_gpu import _random_case
    from frenetix_occlusion import scenario as S
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    scs = [S.load_geometry_npz(os.path.join(g, f"scenario{i}_geometry.npz")) for i in (1, 2, 3)]
    rng = np.random.default_rng(7)
    for _ in range(30):
        path = _random_case(rng, scs)[2]
        if len(path) < 4:
            continue
        f = InterpolatedNormalFrame(path)
        for i, p in enumerate(path):
            s, d = f.convert_to_curvilinear_coords(p[0], p[1])
            assert abs(s - f.s[i]) <= 1e-9 and abs(d) <= 1e-9


def test_points_beyond_the_end_normals_are_refused():
    f = InterpolatedNormalFrame(bend_path())
    for q in ((-31.0, 0.5), (-35.0, -4.0), (8.5, 39.5), (5.0, 45.0)):
        with pytest.raises(ValueError):
            f.convert_to_curvilinear_coords(*q)
    for s in (-0.1, f.s[-1] + 0.1):
        with pytest.raises(ValueError):
            f.convert_to_cartesian_coords(s, 0.0)


def test_the_host_table_reproduces_the_frame_and_measures_its_fit():
    from frenetix_occlusion.spawn_locator import caller_frame_table, frame_table_to_cart
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    path = bend_path()
    f = InterpolatedNormalFrame(path)
    tab, fit = caller_frame_table(f, path)
    assert tab.shape == (len(path), 6)
    np.testing.assert_array_equal(tab[:, :2], path)
    np.testing.assert_allclose(tab[:, 2], f.s, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(tab[:, 3], _pathlength(path))          # the polyline arc lengths the turn rule reads
    np.testing.assert_allclose(tab[:, 4:6], f.normals, rtol=0, atol=1e-12)
    assert fit < 1e-12
    for s in np.linspace(0.0, f.s[-1], 57):
        for d in (-4.0, 0.0, 2.5):
            np.testing.assert_allclose(frame_table_to_cart(tab, s, d), f.convert_to_cartesian_coords(s, d), rtol=0, atol=1e-12)
    # the polyline frame of a bent path is NOT of this model between its vertices: measured, and said once
    tab_p, fit_p = caller_frame_table(PolylineCS(path), path)
    assert fit_p > 1e-3
    sl = _locator(path, "caller", PolylineCS(path))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        sl._frame_setup()
        sl._frame_setup()
    assert sl.frame_fit_m == pytest.approx(fit_p) and sum("caller's frame" in str(w.message) for w in rec) == 1


class _Counting:
    def __init__(self, f):
        self.f, self.calls = f, 0

    def __getattr__(self, name):
        m = getattr(self.f, name)

        def call(*a, **k):
            self.calls += 1
            return m(*a, **k)
        return call


def _locator(path, frame, cosy):
    """a SpawnLocator without a GPU: only the host parts of the frame set-up run (no device table is uploaded)"""
    from frenetix_occlusion.spawn_locator import SpawnLocator
    sl = SpawnLocator.__new__(SpawnLocator)
    sl.ref_path, sl.cosy_cl, sl.frame, sl.frame_fit_m = np.asarray(path, float), cosy, frame, None
    sl._frame_src, sl._d_frame6, sl._d_path6 = None, None, "polyline table"
    sl.device = "cpu"
    return sl


def test_the_table_is_built_once_per_object():
    path = bend_path()
    c = _Counting(InterpolatedNormalFrame(path))
    sl = _locator(path, "caller", c)
    t1, fr = sl._frame_setup()
    assert fr == 1 and c.calls > 0
    n = c.calls
    assert sl._frame_setup()[0] is t1 and c.calls == n          # the same object: no call on it, no new table
    sl.cosy_cl = _Counting(InterpolatedNormalFrame(path))
    assert sl._frame_setup()[0] is not t1 and sl.cosy_cl.calls > 0
    sl.cosy_cl = None                                             # no object: the polyline table
    assert sl._frame_setup() == ("polyline table", 0)
    assert _locator(path, "polyline", c)._frame_setup() == ("polyline table", 0)


def test_set_up_refuses_frames_the_device_cannot_follow():
    from frenetix_occlusion.spawn_locator import caller_frame_table
    path = bend_path()
    f = InterpolatedNormalFrame(path)

    class NonMonotone(InterpolatedNormalFrame):
        def convert_to_curvilinear_coords(self, x, y):
            s, d = super().convert_to_curvilinear_coords(x, y)
            return np.array([s if s < 20.0 else 40.0 - s, d])
    with pytest.raises(ValueError, match="strictly increasing at reference path vertex"):
        caller_frame_table(NonMonotone(path), path)
    # the frame of a shorter path: the last vertices do not project
    with pytest.raises(ValueError, match=r"vertex \d+ .*does not project"):
        caller_frame_table(InterpolatedNormalFrame(path[:-5]), path)
    # a frame based on another line (1 m to the side): the base points are not the path's vertices
    with pytest.raises(ValueError, match="vertex 0 is"):
        caller_frame_table(InterpolatedNormalFrame(path + f.normals), path)
    nz = f.normals.copy()
    nz[3] = 0.0
    with pytest.raises(ValueError, match="normal at reference path vertex 3 is zero"):
        caller_frame_table(InterpolatedNormalFrame(path, nz), path)


def test_unknown_frame_value_is_refused():
    from frenetix_occlusion.spawn_locator import SpawnLocator
    sm = SimpleNamespace(ctx=None, device=SimpleNamespace(index=0), route_table=None)
    cfg = {"accelerator": {"spawn": {"frame": "frenet"}}}
    with pytest.raises(ValueError, match="polyline' or 'caller"):
        SpawnLocator(None, bend_path(), cfg, sm)


def test_the_checker_spawns_elsewhere_in_the_two_frames():
    """the rule checker with InterpolatedNormalFrame and with PolylineCS on one curved scene (every cell road and occluded
    but a visible disc around the ego; a lanelet heading that turns): the turn rule's pedestrian lands in other cells"""
    from frenetix_occlusion.utils.curvilinear import PolylineCS
    from oracle.fo_spawn_rules_ref import CellView, SpawnRules
    cfg = {"spawn_locator": {"spawn_points_behind_turn": True, "spawn_point_behind_static_obstacle": True,
                             "spawn_point_behind_dynamic_obstacle": False, "max_static_spawn_points": 1,
                             "max_dynamic_spawn_points": 1},
           "agent_manager": {"pedestrian": {"width": 0.5, "length": 0.3}}}
    path = bend_path(radius=9.0, step_deg=45.0)
    ego = np.array([-12.0, 0.0])
    w = SimpleNamespace(x0=-60.0, y0=-60.0, cs=0.5, ix0=0, iy0=0, nx=240, ny=240)
    xs = w.x0 + (np.arange(w.nx) + 0.5) * w.cs
    gx, gy = np.meshgrid(xs, xs)
    cls = np.full((w.ny, w.nx), 1 | 4, dtype=np.uint8)
    cls[np.hypot(gx - ego[0], gy - ego[1]) < 14.0] = 1 | 2
    view = CellView(cls, w)
    lane_yaw_at = lambda xy: 0.0 if xy[0] < -1.0 else math.pi / 2.0
    got = {}
    for name, f in (("caller", InterpolatedNormalFrame(path)), ("polyline", PolylineCS(path))):
        rules = SpawnRules(cfg, path, f, lane_yaw_at, lambda xy: None, [])
        ego_cl = f.convert_to_curvilinear_coords(ego[0], ego[1])
        pts = rules.find(view, ego, ego_cl, 6.0, 0.0)
        assert rules.last_intention == "left turn" and [p.source for p in pts] == ["left turn"]
        got[name] = pts[0]
    a, b = got["caller"].position, got["polyline"].position
    assert view._cell(a) != view._cell(b) and np.hypot(*(a - b)) > 0.1
