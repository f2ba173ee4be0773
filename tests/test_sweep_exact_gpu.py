"""The sweep kernels against the exact references of tests/golden/dce_rounding.npz and cp_exact.npz (written by
tests/golden/gen_sweep_exact.py; this module reads only those files and NumPy):

* DCE's millimetre rounding at exact half-millimetre ties, a few 2^-51 m around them, at the 0.5 mm boundary (where TTC
  and `safe` straddle) and in walks with tied samples next to the queue kernels' (nmm + 0.51) mm pruning bound:
  dce, time_dce, ttc, ttce and safe exactly;
* the diagonal CP within the bound fo_sweep_common.hpp states for its erf table (2.6e-10), over every table node and phase,
  sigma^2 from 1e-6 to 1e4; the correlated CP within 1e-9, rho on both sides of every rule switch.

For every kernel form, both list formats and the reduced mode.  Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

from golden_util import load_case
from test_sweep_gate_gpu import KERNEL_FORMS, _set_env
from test_sweep_gpu import ATOL, _hip_sweep

pytestmark = pytest.mark.gpu

CP_ERF_BOUND = 2.6e-10      # fo_sweep_common.hpp, fo_erf_fast128: what the dropped Taylor terms may cost a collision probability


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU test selected but no GPU visible"
    return torch


def _first(bad):
    return bad[:10].tolist()


@pytest.mark.parametrize("form,env", KERNEL_FORMS, ids=[f[0] for f in KERNEL_FORMS])
def test_dce_rounding_matches_the_exact_reference(torch_cuda, monkeypatch, form, env):
    from frenetix_occlusion import _native as N
    g, traj, agents, veh, dt = load_case("dce_rounding")
    thr = {"ttc": float(g["ttc_thr"])}
    assert 0 < g["ref_safe"].sum() < len(g["ref_safe"])
    _set_env(monkeypatch, env)
    for lists in ("f64", "f32x"):
        out = _hip_sweep(torch_cuda, traj, agents, veh, dt, thr=thr, lists=lists)
        pf, pi = out["pair_f"], out["pair_i"]
        for name, key in (("dce", "ref_dce"), ("ttc", "ref_ttc"), ("ttce", "ref_ttce")):
            bad = np.argwhere(pf[..., N.PF[name]] != g[key])
            assert len(bad) == 0, f"{form}/{lists}: {name} differs on {len(bad)} pairs, (m, a) e.g. {_first(bad)}, " \
                                  f"got {pf[..., N.PF[name]][tuple(bad[0])]!r}, want {g[key][tuple(bad[0])]!r}"
        bad = np.argwhere(pi[..., N.PI["time_dce"]] != g["ref_time_dce"])
        assert len(bad) == 0, f"{form}/{lists}: time_dce differs on {len(bad)} pairs, (m, a) e.g. {_first(bad)}"
        bad = np.nonzero(out["safe"].astype(bool) != g["ref_safe"])[0]
        assert len(bad) == 0, f"{form}/{lists}: safe differs on trajectories {bad[:10].tolist()}"
        np.testing.assert_array_equal(out["cost"][:, N.COST["min_dce"]], g["ref_dce"].min(axis=1))
    red = _hip_sweep(torch_cuda, traj, agents, veh, dt, thr=thr, mode="reduced")
    assert np.array_equal(red["safe"].astype(bool), g["ref_safe"]), form
    np.testing.assert_array_equal(red["cost"][:, N.COST["min_dce"]], g["ref_dce"].min(axis=1))
    np.testing.assert_array_equal(red["cost"][:, N.COST["min_ttce"]], g["ref_ttce"].min(axis=1))
    np.testing.assert_array_equal(red["cost"][:, N.COST["wttc"]], g["ref_ttc"].min(axis=1))


@pytest.mark.parametrize("form,env", KERNEL_FORMS, ids=[f[0] for f in KERNEL_FORMS])
def test_cp_matches_the_exact_reference(torch_cuda, monkeypatch, form, env):
    from frenetix_occlusion import _native as N
    g, traj, agents, veh, dt = load_case("cp_exact")
    want = g["ref_cp"]
    n = int(g["n_diag"])
    _set_env(monkeypatch, env)
    got = _hip_sweep(torch_cuda, traj, agents, veh, dt)
    cp = got["lists"][:, :, N.LST["cp"], :]
    for sl, tol, what in ((slice(0, n), CP_ERF_BOUND, "diagonal"), (slice(n, None), ATOL, "correlated")):
        err = np.abs(cp[:, sl] - want[:, sl])
        bad = np.argwhere(err > tol)
        if len(bad):
            bad[:, 1] += sl.start
        assert len(bad) == 0, f"{form}: {what} CP off by up to {err.max():.3g} on {len(bad)} samples, (m, a, t-1) e.g. {_first(bad)}"
    mx = want.max(axis=-1)
    tol = np.where(np.arange(want.shape[1]) < n, CP_ERF_BOUND, ATOL)
    gx = _hip_sweep(torch_cuda, traj, agents, veh, dt, lists="f32x")
    assert np.array_equal(gx["lists"][:, :, N.LST["cp"], :], cp.astype(np.float32)), form
    for out in (got, gx):
        err = np.abs(out["pair_f"][..., N.PF["max_collision_probability"]] - mx)
        assert (err <= tol).all(), f"{form}: max_collision_probability, (m, a) e.g. {_first(np.argwhere(err > tol))}"
    red = _hip_sweep(torch_cuda, traj, agents, veh, dt, mode="reduced")
    err = np.abs(red["cost"][:, N.COST["max_collision_probability_all"]] - mx.max(axis=1))
    assert (err <= ATOL).all(), f"{form}: max_collision_probability_all, m e.g. {np.nonzero(err > ATOL)[0][:10].tolist()}"
