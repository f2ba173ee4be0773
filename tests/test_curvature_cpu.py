"""``frenetix_occlusion.utils.curvilinear.curvature`` against analytic curves.  The function decides on the host which spawn
rule families run at all (the ego's intention, thresholds +-0.10 1/m), for the device and for its checker alike, so no
device-against-checker comparison can see a defect in it.

Allowed error, derived from the vertex spacing and the curve, never from the function's output.  The function differentiates
x(s), y(s) twice w.r.t. the polyline's arc length with the three-point formula for uneven spacing inside (error of one
application <= h_max^2 / 6 * max|f'''|) and two-point differences at both ends.  For a curve of curvature |k| <= K and
|dk/ds| <= A (unit speed: |f'''| <= M3 = K^2 + A, |f''''| <= M4 = K^3 + 3 K A; the chords shorten the parameter by a factor
1 - (h K)^2 / 24 at most):
    first derivatives   d1 = h_max^2 / 6 * M3 + h_max^2 K^2 / 24
    second derivatives  d2 = 2 d1 / h_min + h_max^2 / 6 * M4        (the formula's weights sum to <= 2 / h_min in magnitude: an
                                                                     irregular error of the inputs is amplified by that)
    curvature           2 d2 + 5 d1 K                                (numerator terms x'y'', x''y' with |x'|, |y'| <= 1,
                                                                     |x''|, |y''| <= K; the denominator within 1 +- 3 d1)
This holds from the third vertex to the third from last; the two vertices at either end see a one-sided first derivative
(the chord's direction: the tangent half a step further on), which only lowers the magnitude there."""
import math

import numpy as np
import pytest

from frenetix_occlusion.spawn_locator import intention_from_curvature
from frenetix_occlusion.utils.curvilinear import curvature


def allowed_error(h_min, h_max, K, A=0.0):
    M3, M4 = K * K + A, K ** 3 + 3.0 * K * A
    d1 = h_max ** 2 / 6.0 * M3 + h_max ** 2 * K * K / 24.0
    d2 = 2.0 * d1 / h_min + h_max ** 2 / 6.0 * M4
    return 2.0 * d2 + 5.0 * d1 * K


def _uneven(rng, total, h_min, h_max):
    """arc lengths 0 ... >= total with steps drawn from [h_min, h_max]"""
    s = [0.0]
    while s[-1] < total:
        s.append(s[-1] + float(rng.uniform(h_min, h_max)))
    return np.array(s)


@pytest.mark.parametrize("radius", [9.5, 10.0, 10.5])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_circles_on_both_sides_of_the_intention_threshold(radius, sign):
    """arcs of 9.5 / 10 / 10.5 m radius (curvature 0.1053 / 0.1 / 0.0952: either side of the 0.10 threshold and on it),
    left and right, vertices every 0.1 ... 0.2 m of arc at seeded uneven steps: allowed error 3.4e-3 < the 4.8e-3 to the
    threshold, so the side of the threshold follows from the bound"""
    rng = np.random.default_rng(int(radius * 10))
    h_lo, h_hi = 0.1, 0.2
    arc = _uneven(rng, 25.0, h_lo, h_hi)
    ang = arc / radius
    p = np.stack((radius * np.sin(ang), sign * radius * (1.0 - np.cos(ang))), -1)
    h = np.hypot(*np.diff(p, axis=0).T)                         # the chords: what the function sees as spacing
    assert h.min() >= h_lo * (1.0 - (h_hi / radius) ** 2 / 24.0) - 1e-12 and h.max() <= h_hi
    tol = allowed_error(h.min(), h.max(), 1.0 / radius)
    assert tol < 0.0048
    k = curvature(p)
    assert k.shape == (len(p),)
    assert np.abs(k[2:-2] - sign / radius).max() <= tol
    assert (sign * k[[0, 1, -2, -1]] <= 1.0 / radius + tol).all() and (sign * k[[0, 1, -2, -1]] >= 0.0).all()
    if radius != 10.0:
        want = 0 if radius > 10.0 else (1 if sign > 0 else 2)
        assert intention_from_curvature(k) == want


def test_straight_line_with_repeated_vertices():
    """a straight line at an oblique heading, uneven steps, every fifth vertex stored twice (and one three times), no jitter:
    repeated vertices are dropped (one value per distinct vertex), no division by zero, and the curvature is rounding only --
    coordinates up to L = 60 m carry eps L each, two differences divide by h_min twice: 64 eps L / h_min^2"""
    rng = np.random.default_rng(5)
    s = _uneven(rng, 60.0, 0.2, 1.5)
    d = np.array([math.cos(0.7), math.sin(0.7)])
    base = np.array([12.0, -7.0])[None] + s[:, None] * d[None]
    rep = np.repeat(base, np.where(np.arange(len(base)) % 5 == 0, 2, 1), axis=0)
    rep = np.insert(rep, 3, rep[3], axis=0)
    assert len(rep) > len(base) + 5
    with np.errstate(all="raise"):
        k = curvature(rep)
    assert k.shape == (len(base),) and np.isfinite(k).all()
    assert np.abs(k).max() <= 64.0 * np.finfo(float).eps * 60.0 / 0.2 ** 2
    np.testing.assert_array_equal(k, curvature(base))
    assert intention_from_curvature(k) == 0


def test_clothoid_entry_against_mpmath():
    """the entry of a bend: curvature a s with a = 0.01 1/m^2 over 12 m (0 -> 0.12 1/m), the vertices from mpmath's Fresnel
    integrals at 30 digits, uneven steps of 0.1 ... 0.2 m: K = 0.12, A = 0.01"""
    import mpmath as mp
    mp.mp.dps = 30
    a = 0.01
    rng = np.random.default_rng(9)
    s = _uneven(rng, 12.0, 0.1, 0.2)
    s = s[s <= 12.0]
    scale = mp.sqrt(mp.pi / a)
    p = np.array([[float(scale * mp.fresnelc(si / scale)), float(scale * mp.fresnels(si / scale))] for si in s])
    h = np.hypot(*np.diff(p, axis=0).T)
    tol = allowed_error(h.min(), h.max(), a * 12.0, a)
    assert tol < 0.01
    k = curvature(p)
    assert np.abs(k[2:-2] - a * s[2:-2]).max() <= tol
    assert intention_from_curvature(k) == 1 and intention_from_curvature(curvature(p * np.array([1.0, -1.0]))) == 2


def test_windows_of_two_and_three_vertices():
    """two vertices have no curvature (zeros); three vertices at equal chords h on a circle of radius R, turning by phi from
    chord to chord (h = 2 R sin(phi / 2)), give closed forms of the difference scheme itself: the end values see
    (chord 2 - chord 1) / (2 h) against one chord, cos(phi / 2) / (2 R); the middle value sees it against the mean chord,
    1 / (2 R cos^2(phi / 2)) -- a three-vertex window shows HALF the curve's curvature (rounding: 1e-12 relative)"""
    assert curvature(np.array([[0.0, 0.0], [3.0, 4.0]])).tolist() == [0.0, 0.0]
    for R, phi, sign in ((8.0, 0.2, 1.0), (10.0, 0.05, -1.0), (4.0, 0.5, 1.0)):
        ang = np.array([0.0, phi, 2.0 * phi])
        p = np.stack((R * np.sin(ang), sign * R * (1.0 - np.cos(ang))), -1)
        k = curvature(p)
        end, mid = math.cos(phi / 2.0) / (2.0 * R), 1.0 / (2.0 * R * math.cos(phi / 2.0) ** 2)
        np.testing.assert_allclose(k, sign * np.array([end, mid, end]), rtol=1e-12, atol=0)
