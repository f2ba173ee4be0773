"""The exact-reference fixtures of the sweep's DCE rounding and CP box sums (tests/golden/dce_rounding.npz, cp_exact.npz):
they regenerate bit for bit from tests/ref_sweep_exact.py, they probe what they claim to, and the oracle -- the checker of
the rest of the suite -- reproduces them: DCE exactly, diagonal CP within 1e-13, correlated CP within 1e-12."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_sweep_exact as G  # noqa: E402
import ref_sweep_exact as R  # noqa: E402
from golden_util import GOLDEN, load_case  # noqa: E402

pytest.importorskip("mpmath")


def _stored(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def dce_new():
    return G.dce_contents()


ERF_ARGS = []


@pytest.fixture(scope="module")
def cp_new():
    return G.cp_contents(ERF_ARGS)


@pytest.mark.parametrize("name", ["dce_rounding", "cp_exact"])
def test_fixtures_regenerate_bit_for_bit(name, dce_new, cp_new):
    new = dce_new if name == "dce_rounding" else cp_new
    old = _stored(name)
    assert sorted(old) == sorted(new)
    for k in old:
        a, b = np.asarray(old[k]), np.asarray(new[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 300 * 1024


def test_dce_fixture_covers_ties_both_roundings_and_the_half_millimetre():
    g = _stored("dce_rounding")
    tie, mm, gap = g["rec_tie"], g["rec_mm"], g["rec_gap_mm"]
    assert tie.sum() >= 100                               # exact half-millimetre ties, rounded half to even ...
    assert (mm[tie] % 2 == 0).all() and len(np.unique(mm[tie])) >= 12
    # ... and samples within a few 1e-13 mm of a tie on both sides (a few steps of 2^-51 m)
    assert (gap[~tie] < 1e-12).sum() >= 100
    # agent 3: walks with several samples of one pair at the pair's rounded minimum
    walk = g["rec_a"] == 3
    dce = g["ref_dce"]
    n_at_min = [np.sum((g["rec_m"] == m) & walk & (mm == dce[m, 3] * 1000)) for m in np.nonzero(g["pair_agent"] == 3)[0]]
    assert sum(n > 1 for n in n_at_min) >= 30
    # the 0.5 mm boundary: both roundings occur, and `safe` differs between them
    half = np.array([str(s).startswith("half-mm") for s in g["label"]])
    assert set(dce[half, 4] * 1000) == {0.0, 1.0}
    assert not g["ref_safe"][half & (dce[:, 4] == 0)].any() and g["ref_safe"][half & (dce[:, 4] > 0)].all()
    # rotated near-ties: every sample evaluated exactly is farther than the stated margin from a half millimetre
    rot = g["rec_a"] == 5
    assert rot.sum() >= 40 and (gap[rot] > R.ROT_MARGIN * 1e3).all()


def test_dce_oracle_matches_the_exact_reference(oracle):
    g, traj, agents, veh, dt = load_case("dce_rounding")
    ref = oracle.sweep(traj, agents, veh, dt, thr={"ttc": float(g["ttc_thr"])})
    PF, PI = oracle.PF, oracle.PI
    for name, key in (("dce", "ref_dce"), ("ttc", "ref_ttc"), ("ttce", "ref_ttce")):
        bad = np.argwhere(ref["pair_f"][..., PF[name]] != g[key])
        assert len(bad) == 0, f"{name}: {len(bad)} pairs differ, (m, a) e.g. {bad[:10].tolist()}"
    assert np.array_equal(ref["pair_i"][..., PI["time_dce"]], g["ref_time_dce"])
    assert np.array_equal(ref["safe"].astype(bool), g["ref_safe"])


def test_cp_fixture_covers_every_table_node_phase_and_rule_switch(cp_new):
    g = _stored("cp_exact")
    # every node 0..768 of the erf table at seven phases in [-1/2, 1/2] (node 0 has only the non-negative ones)
    u = np.abs(ERF_ARGS[0]) * 128
    node = np.rint(u)
    keep = node <= 768
    bins = np.clip(np.floor((u - node + 0.5) * 7), 0, 6).astype(int)
    hit = set(zip(node[keep].astype(int), bins[keep]))
    assert len(hit) == 769 * 7 - 3
    assert (u >= 6 * 128).sum() > 1000
    # sigma^2 from 1e-6 to 1e4 and the zero matrix; rho on both sides of every rule switch
    cov = g["agent_cov"][:, 0]
    sxx = cov[:, 0, 0]
    assert sxx[sxx > 0].min() <= 1e-6 and sxx.max() >= 1e4 and ((cov == 0).all(axis=(1, 2))).any()
    rho = cov[:, 0, 1] / np.sqrt(cov[:, 0, 0] * cov[:, 1, 1])
    for v in R.RHO_SWITCH:
        assert (rho == math.nextafter(v, 0.0)).any() and (rho == math.nextafter(v, 1.0)).any(), v
    assert (np.abs(rho) == 0.99).sum() >= 2
    cp = g["ref_cp"]
    n = int(g["n_diag"])
    assert (cp[:, :n] > 0).sum() > 8000 and (cp[:, n:] > 0).sum() > 100


def test_cp_oracle_matches_the_exact_reference(oracle):
    g, traj, agents, veh, dt = load_case("cp_exact")
    ref = oracle.sweep(traj, agents, veh, dt)
    cp = ref["lists"][:, :, oracle.LST["cp"], :]
    n = int(g["n_diag"])
    for sl, tol, what in ((slice(0, n), 1e-13, "diagonal"), (slice(n, None), 1e-12, "correlated")):
        err = np.abs(cp[:, sl] - g["ref_cp"][:, sl])
        bad = np.argwhere(err > tol)
        assert len(bad) == 0, f"{what}: {len(bad)} samples off by up to {err.max():.3g}, (m, a, t-1) e.g. {bad[:10].tolist()}"
