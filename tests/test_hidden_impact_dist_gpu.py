"""The two-rank shard of the impact verdict stage (PlanningStep(shard=, hidden_impact_verdict=); DESIGN.md §5.10 "Impact verdict" and
"Impact verdict by approach angle"), for both approaches: two processes on one GPU, the collective over gloo, in the style of
tests/test_hidden_brake_verdict_gpu.py's shard test and its worker.  The test is about those processes: it starts
tests/hidden_impact_dist_worker.py twice per approach and reads what rank 0 wrote."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_hidden_impact as RI
import rule_refusal_cases as RC
import test_hidden_reach_gpu as T
from test_hidden_reach_gpu import torch_cuda  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RANK_LIMIT = 200          # seconds the ranks of one run may take
HARM_LIMIT = 0.1          # of tests/test_hidden_impact_lanes_gpu._iv


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(RANK_LIMIT + 60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _run_ranks(tmp_path, world, approach):
    import test_distributed_gpu as DG
    port = DG._free_port()
    out = str(tmp_path / f"impact_{approach}_{world}.npz")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(T.ROOT, "tests", "hidden_impact_dist_worker.py"), "--approach", approach,
                                       "--out", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=RANK_LIMIT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    return np.load(out)


@pytest.mark.parametrize("approach", ["head_on", "lanes"])
def test_two_ranks_shard_the_step_with_the_impact_stage(torch_cuda, tmp_path, approach):
    """rank 1 holds rows 65 .. 129: its stage runs on those rows and on its cut of the ragged lengths and is queued BEFORE the all-gather.
    Rows [lo, hi) of every rank in cost_all are the unsharded step + stage bit for bit -- the two columns, the lowered flag and every
    column the stage does not own -- and what each rank holds of its own rows, put end to end, is the unsharded answer too"""
    world = 2
    z = _run_ranks(tmp_path, world, approach)
    M = RC.M
    per = -(-M // world)
    assert int(z["world"]) == world and [tuple(r) for r in z["rows"]] == [(min(r * per, M), min(r * per + per, M)) for r in range(world)]
    assert z["cost_all"].shape == (M, 16) and z["cost_all"].tobytes() == z["ref_cost"].tobytes()
    for lo, hi in z["rows"]:
        assert hi > lo
        assert z["cost_all"][lo:hi, RI.C_RES0].tobytes() == z["ref_harm"][lo:hi, 0].tobytes()
        assert np.array_equal(z["cost_all"][lo:hi, RI.C_RES1], z["ref_user"][lo:hi].astype(np.float64))
        assert np.array_equal(z["cost_all"][lo:hi, RI.C_SAFE], z["ref_safe"][lo:hi].astype(np.float64))
    assert z["local_cost"].tobytes() == z["ref_cost"].tobytes() and np.array_equal(z["local_safe"], z["ref_safe"])
    assert z["local_harm"].tobytes() == z["ref_harm"].tobytes() and np.array_equal(z["local_user"], z["ref_user"])
    assert np.array_equal(z["local_at"], z["ref_at"]) and z["local_per_user"].tobytes() == z["ref_per_user"].tobytes()
    # the stage did something on either side of the boundary, and the case is not degenerate
    want_cost, want_safe = RI.fold(z["plain_cost"], (z["plain_cost"][:, RI.C_SAFE] > 0.5).astype(np.uint8), z["ref_harm"], z["ref_user"], HARM_LIMIT)
    assert want_cost.tobytes() == z["ref_cost"].tobytes() and np.array_equal(want_safe, z["ref_safe"])
    assert (z["plain_cost"][:, 14:16] == 0.0).all()
    for lo, hi in z["rows"]:                                        # (a row without a hit gets user -1: the stage shows in every row)
        assert (z["ref_cost"][lo:hi, RI.C_RES1] != z["plain_cost"][lo:hi, RI.C_RES1]).any()
    assert (z["ref_user"] >= 0).any() and (z["ref_harm"][:, 0] > 0.0).any()
    assert (z["plain_cost"][:, RI.C_SAFE] > z["ref_cost"][:, RI.C_SAFE]).any()                    # a flag was lowered
    none = np.clip(z["lengths"], 0, RC.T) == 0
    assert none.any() and (z["ref_user"][none] == -1).all() and (z["ref_harm"][none] == 0.0).all()
    if approach == "lanes":
        assert (z["ref_cosine"] < 1.0).any() and (z["ref_cosine"][0] == 1.0).all()                # lane-bound users bite, the pedestrian is free
