"""The two-rank shard of a planning step with the harm ladder by approach angle (PlanningStep(shard=,
hidden_harm_ladder_lanes_verdict=); DESIGN.md §5.10 "Harm ladder by approach angle"): two processes on one GPU
(tests/hidden_harm_ladder_lanes_dist_worker.py), the collective over gloo -- rows [lo, hi) of every rank are the unsharded step + stage,
bit for bit."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_hidden_brake_harm_ladder as RH
import rule_refusal_cases as RC
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RANKS_LIMIT = 200         # seconds the worker processes may take


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(RANKS_LIMIT + 60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _run_ranks(tmp_path, world, backend):
    """tests/hidden_harm_ladder_lanes_dist_worker.py as ``world`` processes, started as tests/test_distributed_gpu._run_ranks starts its worker"""
    import test_distributed_gpu as DG
    port = DG._free_port()
    out = str(tmp_path / f"harm_ladder_lanes_{backend}_{world}.npz")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(T.ROOT, "tests", "hidden_harm_ladder_lanes_dist_worker.py"), "--backend", backend,
                                       "--out", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=RANKS_LIMIT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    return np.load(out)


def test_two_ranks_shard_the_step_with_the_stage(torch_cuda, tmp_path):
    """rank 1 holds rows 65 .. 129, its stage runs on those rows and on its cut of the ragged lengths and is queued BEFORE the
    all-gather: the gathered cost matrix, every rank's own rows and all nine outputs of the stage are the unsharded step + stage"""
    z = _run_ranks(tmp_path, 2, "gloo")
    M = RC.M
    assert int(z["world"]) == 2 and [tuple(r) for r in z["rows"]] == [(0, 65), (65, 130)]
    assert z["cost_all"].shape == (M, 16) and z["cost_all"].tobytes() == z["ref_cost"].tobytes()
    assert z["local_cost"].tobytes() == z["ref_cost"].tobytes() and np.array_equal(z["local_safe"], z["ref_safe"])
    for name in RH.OUTPUTS:
        assert z["local_" + name].shape == z["ref_" + name].shape and z["local_" + name].tobytes() == z["ref_" + name].tobytes(), name
    want_cost, want_safe = RH.fold(z["plain_cost"], (z["plain_cost"][:, RH.C_SAFE] > 0.5).astype(np.uint8), z["ref_need"], z["ref_user"],
                                   z["ref_decel"], z["ref_harm_at"].shape[1], 4.0)
    assert want_cost.tobytes() == z["ref_cost"].tobytes() and np.array_equal(want_safe, z["ref_safe"])
    assert (z["plain_cost"][:, 14:16] == 0.0).all()
    for lo, hi in z["rows"]:                                        # the stage did something on either side of the boundary
        assert (z["ref_harm_at"][lo:hi] > 0.0).any()
        assert z["cost_all"][lo:hi, RH.C_RES0].tobytes() == z["ref_decel"][lo:hi].tobytes()
    ends = np.clip(z["lengths"], 0, RC.T)
    assert (ends == 0).any() and (z["ref_need"][ends == 0] == -1).all() and (z["ref_harm_at"][ends == 0] == 0.0).all() and ((ends > 0) & (ends < 5)).any()
