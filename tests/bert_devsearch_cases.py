"""Shared by test_bert_devsearch_cpu.py and test_bert_devsearch_hip.py: the small data set, the seeded models and the entry point of the
process-group test.

Data.  tests/sasrec_deveval_cases.py:make_data(60): itemnum 150, 40 users with histories of 1 .. 60 actions (users 1 and 2 have no
held-out item), one interior id that occurs nowhere, id 0 never, and id itemnum = 150 in histories -- for BERT4Rec-ADT a drawable id, since
its table runs over ids 0 .. itemnum.  L = 8, S = 16.
"""
import numpy as np

import sasrec_deveval_cases as sc

ITEMNUM, L, S = sc.ITEMNUM, 8, 16
REC_CHOICE, IND_CHOICE = [0, 0.001, 0.01], [0, 0.001, 0.002]      # a 3 x 3 grid: nine candidate layers per depth


class Args:
    pass


def make_data():
    return sc.make_data(60)


def model_args(dev, d, H, precision, maxlen=L, dropout=0.0, attention_dropout=0.0):
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = dev, maxlen, H, 2, d, 2 * d
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision, a.initializer_range = dropout, attention_dropout, 2, precision, 0.02
    return a


def bert_model(dev, d=64, H=2, precision="bf16", seed=11):
    """A seeded BertModel over the data set: d 64 / H 2 runs as it is, d 50 / H 1 on padded lanes (feature stride 64)."""
    import torch
    from adt_amd.bert4rec.model import BertModel
    torch.manual_seed(seed)
    return BertModel(1, ITEMNUM, model_args(dev, d, H, precision)).eval()


def super_model(dev, seed=13, dropout=0.0, attention_dropout=0.0):
    import torch
    from adt_amd.bert4rec.superbert import SuperBertModel
    torch.manual_seed(seed)
    return SuperBertModel(1, ITEMNUM, REC_CHOICE, IND_CHOICE, model_args(dev, 64, 2, "f32", dropout=dropout, attention_dropout=attention_dropout))


def eval_sets(mode, sample_size=S):
    """(train, valid, test, usernum, sampler, BertEvalDataset of `mode`)."""
    from adt_amd.bert4rec import datasets as D
    train, valid, test, usernum, itemnum = make_data()
    sampler = D.PopularSampler(train, valid, test, usernum, itemnum, sample_size)
    return train, valid, test, usernum, sampler, D.BertEvalDataset(train, valid, test, usernum, itemnum, L, sampler, mode)


def dp_main():
    """One rank of FusedBertTrainer.evaluate(device_scores=True) under a process group (gloo ranks sharing one GPU), or the single
    process: prints its metrics as JSON."""
    import json
    import sys
    from adt_amd.bert4rec import datasets as D
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    from adt_amd.dp import init_from_env
    pg, rank, world, local = init_from_env("gloo")
    dev = "cuda:%d" % local
    train, valid, test, usernum, sampler, ds = eval_sets("test")
    dd = D.DeviceBertData(train, usernum, ITEMNUM, L, 0.2, dev)
    dd.add_eval(ds)
    tr = FusedBertTrainer(bert_model(dev), [0.1, 0.1], [0.1, 0.1], process_group=pg)
    (ndcg, hr), auc = tr.evaluate(dd.eval_batches("test", 8), device_scores=True)      # 38 users: five batches, three for rank 0
    line = json.dumps({"rank": rank, "world": world, "ndcg": [ndcg[5], ndcg[10]], "hr": [hr[5], hr[10]], "auc": auc}) + "\n"
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
