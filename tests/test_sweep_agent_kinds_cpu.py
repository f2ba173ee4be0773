"""The reference side of tests/test_sweep_agent_kinds_gpu.py, without a GPU: the agent set of tests/sweep_agent_kind_cases.py is
what its header says, and the oracle finds an in-gate pair and a pair with DCE = 0 in every per-agent body of the queue kernel,
at both horizons and under both coefficient sets -- so a green GPU run cannot come from an empty case."""
import pytest

import sweep_agent_kind_cases as K


@pytest.mark.parametrize("T", K.HORIZONS)
def test_every_body_of_the_agent_set_is_exercised(oracle, T):
    usual, flipped = (name for name, _ in K.harm_coeffs(oracle))
    b0 = K.assert_every_body_is_exercised(oracle, T, usual)
    b1 = K.assert_every_body_is_exercised(oracle, T, flipped)
    # the second coefficient set moves the two-coefficient agents, and only them, to the generic body
    assert [(a, b) for a, b in zip(b0, b1) if a != b] == [(K.HM_DVMAX, K.HM_GENERIC)] * b0.count(K.HM_DVMAX)
    assert b0.count(K.HM_DVMAX) >= 4 and b0.count(K.HM_LR4S) >= 3 and b0.count(K.HM_GENERIC) == 1


def test_the_coefficient_sets_differ_where_they_should(oracle):
    """the obstacle-side harm of the two-coefficient agents moves with `ped_speed`; the LR4S agents and every geometric output
    do not"""
    import numpy as np
    O = oracle
    a, b = (K.oracle_run(O, 31, name) for name, _ in K.harm_coeffs(O))
    oh = O.LST["obst_harm"]
    lr4s = [k for k, ag in enumerate(K.AGENTS) if ag[1] in K.PROT1]
    two = [k for k, ag in enumerate(K.AGENTS) if ag[1] in K.PROT0 and ag[2] > 1]
    assert np.array_equal(a["lists"][:, lr4s], b["lists"][:, lr4s], equal_nan=True)
    for k in two:
        assert not np.array_equal(a["lists"][:, k, oh], b["lists"][:, k, oh], equal_nan=True), k
    for name in ("dce", "ttc", "ttce", "max_collision_probability"):
        assert np.array_equal(a["pair_f"][..., O.PF[name]], b["pair_f"][..., O.PF[name]], equal_nan=True), name
