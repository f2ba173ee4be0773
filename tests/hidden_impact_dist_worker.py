"""One rank of a sharded planning step WITH the impact verdict stage (started by tests/test_hidden_impact_dist_gpu.py in the way
tests/test_hidden_brake_verdict_gpu.py starts tests/hidden_verdict_dist_worker.py: one process per rank, RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT from the environment, before the child has touched a GPU).  Every rank builds the stack of tests/rule_refusal_cases.py on the
right-turn scene and the same 130 candidates with ragged lengths, and runs ``PlanningStep(shard=CostGather, hidden_impact_verdict=...)``
with the ``--approach`` asked for: the stage folds into this rank's rows and the one all-gather follows it.  Rank 0 writes what it
gathered, what every rank holds of its own rows, and the unsharded step + stage it computes itself, into an .npz.  Every rank is on GPU 0,
the collective goes over the CPU (gloo)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "frenetix-occlusion_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--approach", required=True, choices=["head_on", "lanes"])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

    import numpy as np
    import torch
    import torch.distributed as dist
    import hidden_verdict_dist_worker as HW
    import rule_refusal_cases as RC
    import test_hidden_impact_lanes_gpu as LG
    from frenetix_occlusion import distributed as D
    from frenetix_occlusion.step import PlanningStep

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    k = RC.stack(torch, RC.turn_scene(0.5))
    M, T = RC.M, RC.T
    iv = LG._iv(lengths=HW.lengths(M, T), approach=args.approach, heading_slack=0.1 if args.approach == "lanes" else 0.0)
    per_user = "closing" if args.approach == "lanes" else "speed"
    cg = D.CostGather(M, device=torch.device("cpu"))
    assert (cg.world, cg.rank) == (world, rank) and cg.collective
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", shard=cg, hidden_impact_verdict=iv)
    for _ in range(2):
        o = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert o.rows == D.shard_bounds(M, world, rank) == (cg.lo, cg.hi) and cg.calls == 2
    n = o.rows[1] - o.rows[0]
    stage = o.hidden_impact_verdict
    assert tuple(o.cost.shape) == (n, 16) and tuple(stage.harm.shape) == (n, 2) and tuple(o.cost_all.shape) == (M, 16)
    cpu = lambda t: t.cpu().numpy().copy()
    mine = dict(rows=o.rows, cost=cpu(o.cost), safe=cpu(o.safe), harm=cpu(stage.harm), user=cpu(stage.user), at=cpu(stage.at),
                per_user=cpu(getattr(stage, per_user)), total=float(np.nansum(o.cost_all.cpu().numpy())))
    got = [None] * world
    dist.all_gather_object(got, mine)
    assert len({g["total"] for g in got}) == 1                                # every rank holds the same gathered matrix
    if rank == 0:
        # the unsharded answer: the plain step, then the stage by its own call on all M candidates
        o1 = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced").run(k.sc.ego, k.sc.yaw, k.sc.v)
        plain = o1.cost.clone()
        ref = k.sm.hidden_brake_impact(*k.tr[:4], cost=o1.cost, safe=o1.safe, **iv)
        torch.cuda.synchronize()
        np.savez(args.out, world=world, cost_all=cpu(o.cost_all), rows=np.array([g["rows"] for g in got]),
                 local_cost=np.concatenate([g["cost"] for g in got]), local_safe=np.concatenate([g["safe"] for g in got]),
                 local_harm=np.concatenate([g["harm"] for g in got]), local_user=np.concatenate([g["user"] for g in got]),
                 local_at=np.concatenate([g["at"] for g in got], axis=1), local_per_user=np.concatenate([g["per_user"] for g in got], axis=1),
                 plain_cost=cpu(plain), ref_cost=cpu(o1.cost), ref_safe=cpu(o1.safe), ref_harm=cpu(ref.harm), ref_user=cpu(ref.user),
                 ref_at=cpu(ref.at), ref_per_user=cpu(getattr(ref, per_user)), lengths=iv["lengths"],
                 ref_cosine=cpu(ref.cosine) if args.approach == "lanes" else np.ones((3, M)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
