"""The collision-probability gate (collision_probability.py:49-67,75: a CP is computed only where the nearest of the three
means mean + j dev, j = 0, +1, -1, is not more than 5 m from the ego sample) replayed operation for operation on the samples
of tests/golden/cp_gate_boundary.npz -- ego samples within three ulps of the 5 m circle around one of the means, produced by
the reference's own code (gen_golden.py gate).  The sweep kernels evaluate the gate in fo_gate_d2 (csrc/fo_sweep_common.hpp): the
mean displaced first, then the ego subtracted, each square rounded, the sum, no contraction.  NumPy float64 does exactly
that; a fused multiply-add is emulated exactly with fractions.Fraction.  CPU only."""
import glob
import os
import re
from fractions import Fraction

import numpy as np

from golden_util import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-occlusion_amd", "csrc")
SWEEP = [os.path.join(CSRC, "fo_sweep.hip")] + sorted(glob.glob(os.path.join(CSRC, "fo_sweep_*.hpp")))   # the translation unit
M2_IN = 25.000000000000004      # the queue kernel's square-root-free form of !(sqrt(m2) > 5.0)


def _fma(a, b, c):
    """a * b + c rounded once (v_fma_f64 / v_fmac_f64)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _samples():
    """(ego x, ego y, mean x, mean y, dev x, dev y, reference decision) of every (trajectory, agent, sample) with a mean:
    ego sample i, agent mean i-1, heading i (Q1), dev = cos / sin of the heading times half the prediction's length"""
    g, traj, agents, _, _ = load_case("cp_gate_boundary")
    T = traj["x"].shape[1]
    ex, ey = traj["x"][:, None, 1:], traj["y"][:, None, 1:]
    mx, my = agents["pos"][None, :, :T - 1, 0], agents["pos"][None, :, :T - 1, 1]
    hdev = agents["shape"][:, 0] / 2.0
    devx = (np.cos(agents["yaw"][:, 1:T]) * hdev[:, None])[None]
    devy = (np.sin(agents["yaw"][:, 1:T]) * hdev[:, None])[None]
    shp = np.broadcast_shapes(ex.shape, mx.shape)
    return tuple(np.broadcast_to(v, shp) for v in (ex, ey, mx, my, devx, devy)) + (g["ref_in_gate"],)


def _fixed_d2(ex, ey, mx, my, devx, devy):
    """fo_gate_d2, operation for operation (NumPy does not contract)"""
    cx, cy = mx - ex, my - ey
    fx, fy = (mx + devx) - ex, (my + devy) - ey
    bx, by = (mx - devx) - ex, (my - devy) - ey
    return np.fmin(cx * cx + cy * cy, np.fmin(fx * fx + fy * fy, bx * bx + by * by))


def _old_d2(ex, ey, mx, my, devx, devy, fused=True, displace_difference=True):
    """the gate the kernels had before fo_gate_d2: r = ego - mean, then (r -+ dev)^2 summed, which the compiler contracted to
    one multiply and one fused multiply-add; the two flags take one of the two departures from the reference at a time"""
    out = np.empty(ex.shape)
    for n, (a, b, c, d, e, f) in enumerate(zip(ex, ey, mx, my, devx, devy)):
        if displace_difference:
            rx, ry = a - c, b - d
            terms = ((rx, ry), (rx - e, ry - f), (rx + e, ry + f))
        else:
            terms = ((c - a, d - b), ((c + e) - a, (d + f) - b), ((c - e) - a, (d - f) - b))
        out[n] = min((_fma(qx, qx, qy * qy) if fused else qx * qx + qy * qy) for qx, qy in terms)
    return out


def test_fixture_sits_on_the_gate_boundary():
    """the fixture really probes the boundary: samples on both sides of it around all three means, at every map offset"""
    g, _, _, _, _ = load_case("cp_gate_boundary")
    ing, tgt, mean, ulps = g["ref_in_gate"], g["sample_target"], g["sample_mean"], g["sample_ulps"]
    M, A, _ = ing.shape
    on = ing[np.arange(M)[:, None], tgt[:, 1:], np.arange(1, tgt.shape[1])[None, :] - 1]      # the targeted pair's decision
    for j in range(3):
        sel = (mean[:, 1:] == j) & (np.abs(ulps[:, 1:]) <= 3)
        assert on[sel].any() and (~on[sel]).any(), j
    assert on[ulps[:, 1:] == 90].all() and on[ulps[:, 1:] == 91].all() and not on[ulps[:, 1:] == 92].any()
    offs = np.floor(np.log10(np.abs(g["agent_pos"][:, 0, 0]))).astype(int)
    assert set(offs.tolist()) == {1, 2, 3}          # 20 m, 1e2 m + 20, 1e3 m + 20, 5e3 m + 20
    assert (g["ref_cp"][ing] >= 1e-3).all() and (g["ref_cp"][~ing] == 0.0).all()
    assert 0.02 < ing.mean() < 0.2 and (g["agent_cov"][:, :, 0, 1] != 0).any(axis=1).sum() >= 4


def test_kernel_gate_expression_decides_every_fixture_sample_like_the_reference():
    ex, ey, mx, my, devx, devy, ing = _samples()
    m2 = _fixed_d2(ex, ey, mx, my, devx, devy)
    assert np.array_equal(m2 <= M2_IN, ing)                      # the queue kernel's test
    assert np.array_equal(~(np.sqrt(m2) > 5.0), ing)             # the generic kernel's test
    # the square-root-free threshold is the last double whose correctly rounded root is 5.0
    assert np.sqrt(M2_IN) == 5.0 and np.sqrt(np.nextafter(M2_IN, np.inf)) > 5.0 and M2_IN == np.nextafter(25.0, np.inf)


def test_the_old_gate_expression_misdecides_fixture_samples():
    """test-the-test: the fixture tells the old arithmetic apart -- fused squares, the displacement added to the
    difference ego - mean, and each of the two on its own -- so the GPU tests on it fail for a kernel that goes back to it"""
    ex, ey, mx, my, devx, devy, ing = _samples()
    m2 = _fixed_d2(ex, ey, mx, my, devx, devy)
    near = np.abs(m2 - 25.0) < 1e-9 * 25.0           # everything else is decided the same way by any of the forms
    assert near.sum() > 1000
    args = [v[near] for v in (ex, ey, mx, my, devx, devy)]
    wrong = {}
    for fused, disp in ((True, True), (False, True), (True, False)):
        wrong[(fused, disp)] = int(((_old_d2(*args, fused=fused, displace_difference=disp) <= M2_IN) != ing[near]).sum())
    assert all(n > 0 for n in wrong.values()), wrong
    assert wrong[(True, True)] >= 10, wrong


def test_both_sweep_kernels_evaluate_the_gate_through_the_replayed_function():
    """the replay above is fo_gate_d2's text: pin that text, its contraction pragma, and that both kernels call it"""
    src = "\n".join(open(f).read() for f in SWEEP)
    m = re.search(r"__device__ __forceinline__ double fo_gate_d2\(double mx, double my, double devx, double devy, double ex, "
                  r"double ey\) \{(.*?)\n\}", src, re.S)
    assert m, "fo_gate_d2 not found"
    body = " ".join(m.group(1).split())
    assert body == ("#pragma clang fp contract(off) const double cx = mx - ex, cy = my - ey; "
                    "const double fx = (mx + devx) - ex, fy = (my + devy) - ey; "
                    "const double bx = (mx - devx) - ex, by = (my - devy) - ey; "
                    "return fmin(cx * cx + cy * cy, fmin(fx * fx + fy * fy, bx * bx + by * by));"), body
    assert len(re.findall(r"fo_gate_d2\(", src)) == 3         # the definition, the generic kernel, the queue kernel
    assert "m2 <= 25.000000000000004" in src and "!(sqrt(fo_gate_d2(" in src
