"""One rank of a sharded planning step WITH the harm ladder by approach angle (started by tests/test_hidden_harm_ladder_lanes_dist_gpu.py in the way
tests/test_distributed_gpu.py starts tests/dist_worker.py: one process per rank, RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the
environment, before the child has touched a GPU).  Every rank builds the stack of tests/rule_refusal_cases.py on the right-turn scene
and the same 130 candidates with ragged lengths, and runs ``PlanningStep(shard=CostGather, hidden_harm_ladder_lanes_verdict=...)``: the stage
folds into this rank's rows and the one all-gather follows it.  Rank 0 writes what it gathered, what every rank holds of its own rows,
and the unsharded step + stage it computes itself, into an .npz.

    --backend gloo: every rank on GPU 0, the collective over the CPU;  --backend nccl: one GPU per rank
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "frenetix-occlusion_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="gloo", choices=["nccl", "gloo"])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", "0")) if args.backend == "nccl" else 0

    import numpy as np
    import torch
    import torch.distributed as dist
    import rule_refusal_cases as RC
    import ref_hidden_brake_harm_ladder as RH
    import test_hidden_harm_ladder_lanes_gpu as LG
    from hidden_verdict_dist_worker import lengths
    from frenetix_occlusion import distributed as D
    from frenetix_occlusion.step import PlanningStep

    torch.cuda.set_device(local)
    if args.backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    k = RC.stack(torch, RC.turn_scene(0.5))
    M, T = RC.M, RC.T
    hl = LG._hl(lengths=lengths(M, T), starts=T)         # (every brake start: with the ragged lengths both ranks' rows then hold hits)
    cg = D.CostGather(M, device=torch.device("cuda", local) if args.backend == "nccl" else torch.device("cpu"), force=args.backend == "nccl")
    assert (cg.world, cg.rank) == (world, rank) and cg.collective and cg.gathered.data_ptr() != cg.mine.data_ptr()
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", shard=cg, hidden_harm_ladder_lanes_verdict=hl)
    for _ in range(2):
        o = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert o.rows == D.shard_bounds(M, world, rank) == (cg.lo, cg.hi) and cg.calls == 2
    n = o.rows[1] - o.rows[0]
    got_hl = o.hidden_harm_ladder_lanes_verdict
    assert tuple(o.cost.shape) == (n, 16) and tuple(got_hl.need.shape) == (n,) and tuple(got_hl.harm_at.shape) == (n, len(hl["levels"]))
    assert tuple(o.cost_all.shape) == (M, 16)
    host = lambda t: t.cpu().numpy().copy()
    mine = dict(rows=o.rows, cost=host(o.cost), safe=host(o.safe), total=float(np.nansum(np.where(np.isinf(host(o.cost_all)), 1.0, host(o.cost_all)))),
                **{name: host(getattr(got_hl, name)) for name in RH.OUTPUTS})
    got = [None] * world
    dist.all_gather_object(got, mine)
    assert len({g["total"] for g in got}) == 1                                # every rank holds the same gathered matrix
    if rank == 0:
        # the unsharded answer: the plain step, then the stage by its own call on all M candidates
        ps1 = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced")
        o1 = ps1.run(k.sc.ego, k.sc.yaw, k.sc.v)
        plain = o1.cost.clone()
        ref = k.sm.hidden_brake_harm_ladder_lanes(*k.tr[:4], cost=o1.cost, safe=o1.safe, **hl)
        torch.cuda.synchronize()
        per_class = ("need_of", "first")                                      # [C, M]: the candidates are the last axis
        cat = lambda name: np.concatenate([g[name] for g in got], axis=-1 if name in per_class else 0)
        np.savez(args.out, world=world, cost_all=host(o.cost_all), rows=np.array([g["rows"] for g in got]), local_cost=cat("cost"),
                 local_safe=cat("safe"), plain_cost=host(plain), ref_cost=host(o1.cost), ref_safe=host(o1.safe), lengths=hl["lengths"],
                 **{"local_" + name: cat(name) for name in RH.OUTPUTS}, **{"ref_" + name: host(getattr(ref, name)) for name in RH.OUTPUTS})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
