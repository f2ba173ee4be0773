"""One rank of a sharded planning step WITH the fail-safe verdict stage (started by tests/test_hidden_brake_verdict_gpu.py in the way
tests/test_distributed_gpu.py starts tests/dist_worker.py: one process per rank, RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from
the environment, before the child has touched a GPU).  Every rank builds the stack of tests/rule_refusal_cases.py on the right-turn
scene and the same 130 candidates with ragged lengths, and runs ``PlanningStep(shard=CostGather, hidden_verdict=...)``: the stage
folds into this rank's rows and the one all-gather follows it.  Rank 0 writes what it gathered, what every rank holds of its own rows,
and the unsharded step + stage it computes itself, into an .npz.

    --backend gloo: every rank on GPU 0, the collective over the CPU;  --backend nccl: one GPU per rank (a single rank where the
    machine has one GPU: the collective is forced, so the rows still go through all_gather_into_tensor on the GPU)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "frenetix-occlusion_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def lengths(M, T):
    """ragged lengths that differ on either side of every rank boundary: 0, 1, 2, .. T, beyond T, negative, and again"""
    import numpy as np
    return ((np.arange(M) * 5) % (T + 3) - 1).astype(np.int32)


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
    import test_hidden_brake_verdict_gpu as VG
    from frenetix_occlusion import distributed as D
    from frenetix_occlusion.step import PlanningStep

    torch.cuda.set_device(local)
    if args.backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    k = RC.stack(torch, RC.turn_scene(0.5))
    M, T = RC.M, RC.T
    hv = VG._hv(lengths=lengths(M, T))
    cg = D.CostGather(M, device=torch.device("cuda", local) if args.backend == "nccl" else torch.device("cpu"), force=args.backend == "nccl")
    assert (cg.world, cg.rank) == (world, rank) and cg.collective and cg.gathered.data_ptr() != cg.mine.data_ptr()
    ps = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced", shard=cg, hidden_verdict=hv)
    for _ in range(2):
        o = ps.run(k.sc.ego, k.sc.yaw, k.sc.v)
    torch.cuda.synchronize()
    assert o.rows == D.shard_bounds(M, world, rank) == (cg.lo, cg.hi) and cg.calls == 2
    n = o.rows[1] - o.rows[0]
    assert tuple(o.cost.shape) == (n, 16) and tuple(o.hidden_verdict.fail_safe.shape) == (n,) and tuple(o.cost_all.shape) == (M, 16)
    mine = dict(rows=o.rows, cost=o.cost.cpu().numpy().copy(), safe=o.safe.cpu().numpy().copy(),
                fail_safe=o.hidden_verdict.fail_safe.cpu().numpy().copy(), user=o.hidden_verdict.user.cpu().numpy().copy(),
                finite=o.hidden_verdict.poses.finite.cpu().numpy().copy(), total=float(np.nansum(o.cost_all.cpu().numpy())))
    got = [None] * world
    dist.all_gather_object(got, mine)
    assert len({g["total"] for g in got}) == 1                                # every rank holds the same gathered matrix
    if rank == 0:
        # the unsharded answer: the plain step, then the stage by its own call on all M candidates
        ps1 = PlanningStep(k.sm, k.sl, k.sw, *k.tr, mode="reduced")
        o1 = ps1.run(k.sc.ego, k.sc.yaw, k.sc.v)
        plain = o1.cost.clone()
        ref = k.sm.hidden_brake_verdict(*k.tr[:4], cost=o1.cost, safe=o1.safe, **hv)
        torch.cuda.synchronize()
        np.savez(args.out, world=world, cost_all=o.cost_all.cpu().numpy(), rows=np.array([g["rows"] for g in got]),
                 local_cost=np.concatenate([g["cost"] for g in got]), local_safe=np.concatenate([g["safe"] for g in got]),
                 local_fail_safe=np.concatenate([g["fail_safe"] for g in got]), local_user=np.concatenate([g["user"] for g in got]),
                 plain_cost=plain.cpu().numpy(), ref_cost=o1.cost.cpu().numpy(), ref_safe=o1.safe.cpu().numpy(),
                 ref_fail_safe=ref.fail_safe.cpu().numpy(), ref_user=ref.user.cpu().numpy(), lengths=hv["lengths"])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
