"""Shared by test_sasrec_fulleval_device_hip.py: the child process of the data-parallel case.  The data and the model are those of
tests/sasrec_deveval_cases.py."""
import sasrec_deveval_cases as cases


def dp_main():
    """One rank of evaluate_full_device under a process group (gloo ranks sharing one GPU), or the single process: prints its metrics as JSON."""
    import json
    import sys
    from adt_amd.dp import init_from_env
    from adt_amd.sasrec import utils as U
    from adt_amd.sasrec.device_eval import DeviceEvalData
    pg, rank, world, local = init_from_env("gloo")
    dev = "cuda:%d" % local
    train, valid, test, usernum, itemnum = cases.make_data(60)
    sampler = U.PopularSampler(train, valid, test, usernum, itemnum, 5)
    ds = U.EvalDataset(train, valid, test, usernum, itemnum, 8, sampler, "test", -1, frozen=False)
    data = DeviceEvalData.from_dataset(ds, dev, upload=False)
    (ndcg, hr), auc = U.evaluate_full_device(cases.flagship(dev), data, (5, 10), 8, process_group=pg)
    line = json.dumps({"rank": rank, "world": world, "users": len(ds.users), "ndcg": [ndcg[5], ndcg[10]], "hr": [hr[5], hr[10]], "auc": auc}) + "\n"
    if pg is None:
        sys.stdout.write(line)
        return
    import torch.distributed as dist
    for r in range(world):      # one rank at a time: the ranks share a pipe
        if r == rank:
            sys.stdout.write(line)
            sys.stdout.flush()
        dist.barrier(group=pg)
    dist.destroy_process_group()


if __name__ == "__main__":
    dp_main()
