#!/usr/bin/env python3
"""Entry point of BERT4Rec-ADT on the MI355X path -- the counterpart of the reference's bert4rec/main.py + options.py +
BertTrainer.train (trainer.py:88-160): template override, get_lambda, masked-sequence training set, fused device-side
training step, evaluation of NDCG/HR@{5,10} and AUC on popularity-sampled candidates, model selection by valid AUC.

    python -m adt_amd.bert4rec.main --dataset ml-1m --synthetic ml1m --num_epochs 2
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from . import datasets as D
from . import utils as U
from .model import BertModel
from .trainer import FusedBertTrainer


def parse_args(argv=None):
    p = argparse.ArgumentParser()       # bert4rec/options.py:7-64
    p.add_argument("--dataset", default="ml-1m")
    p.add_argument("--data_dir", default="data")
    p.add_argument("--synthetic", default=None)
    p.add_argument("--dataset_random_seed", type=int, default=23)
    p.add_argument("--eval_set_size", type=int, default=-1)
    p.add_argument("--topk", type=int, default=-1)
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--eval_batch_size", type=int, default=512)
    p.add_argument("--eval_negative_sample_size", type=int, default=100)
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--weight_decay", type=float, default=0.001)
    p.add_argument("--num_epochs", type=int, default=100)
    p.add_argument("--clip", type=int, default=5)
    p.add_argument("--eval_interval", type=int, default=1)
    p.add_argument("--dupe_factor", type=int, default=10)
    p.add_argument("--prop_sliding_window", type=float, default=0.1)
    p.add_argument("--type_vocab_size", type=int, default=2)
    p.add_argument("--initializer_range", type=float, default=0.02)
    p.add_argument("--maxlen", type=int, default=200)
    p.add_argument("--hidden_units", type=int, default=64)
    p.add_argument("--inner_units", type=int, default=128)
    p.add_argument("--num_layers", type=int, default=2)
    p.add_argument("--num_heads", type=int, default=2)
    p.add_argument("--dropout", type=float, default=0.2)
    p.add_argument("--attention_dropout", type=float, default=0.2)
    p.add_argument("--mask_prob", type=float, default=0.2)
    p.add_argument("--template", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True)
    p.add_argument("--override", default=None, help="JSON applied after the template")
    p.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    p.add_argument("--use_graph", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True)
    p.add_argument("--eval_full", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=False,
                   help="also rank the held-out item against the whole catalogue at every evaluation")
    p.add_argument("--device_batches", action="store_true",
                   help="mask and build the training batches, and build the evaluation rows, on the GPU from resident sequences "
                        "(adt_bertbatch_build) instead of on the host; the masks come from a different random stream, so such a run is "
                        "not the host run's trajectory")
    p.add_argument("--remask_every_epoch", action="store_true",
                   help="with --device_batches: draw a fresh set of masks every epoch instead of one per example for the whole run")
    p.add_argument("--fused_head", action="store_true",
                   help="at --hidden_units 64: compute the all-item logits and the cross-entropy in the fused kernels (adt_lce_fwd_bwd), which keep "
                        "no (rows, items) logit matrix in memory, instead of the dense head; the probabilities enter the gradient products rounded "
                        "to bf16, so such a run is not the unfused run's trajectory.  Widths 128 / 256 use the fused head already; under "
                        "--precision f32 the flag has no effect")
    p.add_argument("--device_scores", action="store_true",
                   help="count the evaluation ranks on the GPU (adt_cand_rank_hist) and read one histogram per evaluation instead of the ranks of "
                        "every batch; the same candidates and the same ranks, with or without --device_batches")
    p.add_argument("--device_negatives", action="store_true",
                   help="with --device_batches: draw the evaluation candidates on the GPU (adt_evalcand_draw), once per run, instead of with the "
                        "host sampler.  Same distribution as the numpy sampler's candidates, but a hash stream of its own: different "
                        "candidates and therefore different metrics")
    args = p.parse_args(argv)
    if args.remask_every_epoch and not args.device_batches:
        p.error("--remask_every_epoch needs --device_batches")
    if args.device_negatives and not args.device_batches:
        p.error("--device_negatives needs --device_batches")
    return args


def _device_epoch(trainer, data, args, rng, salt, rank=0, world=1):
    """One epoch of --device_batches: the same rng.permutation(len(data)) call as BertTrainDataset.epoch_batches, uploaded once; full
    batches only; every rank builds its rows lo:hi of the global batch.  Returns the number of steps."""
    from ..dp import shard_bounds, skip_batch
    B = args.batch_size
    data.set_order(rng.permutation(len(data)))
    if skip_batch(B, world):
        return 0
    lo, hi = shard_bounds(B, rank, world)
    steps = len(data) // B
    for i in range(steps):
        trainer.step_device(data.train_stage(i * B, B, args.dataset_random_seed, salt, rows=(lo, hi) if world > 1 else None), b_offset=lo)
    return steps


def main(argv=None):
    args = parse_args(argv)
    from ..dp import init_from_env, shard_bounds, skip_batch
    pg, rank, world, local = init_from_env("nccl")     # torch.distributed.run sets RANK / LOCAL_RANK / WORLD_SIZE
    if pg is not None:
        args.device = "cuda:%d" % local
    if args.template:
        args = U.set_template(args)
    if args.override:
        for k, v in json.loads(args.override).items():
            setattr(args, k, v)
    lam = U.get_lambda(args.dataset, args.topk)
    if lam is None:
        raise SystemExit("no lambdas for dataset %r" % args.dataset)
    lambda1, lambda2 = lam
    path = os.path.join(args.data_dir, "%s.txt" % args.dataset)
    if not os.path.exists(path) and args.synthetic:
        from ..sasrec import synth
        if rank == 0:
            os.makedirs(args.data_dir, exist_ok=True)
            h, _, _ = synth.generate(args.synthetic, 23)
            synth.write(path, h)
        if world > 1:
            torch.distributed.barrier()
    user_train, user_valid, user_test, usernum, itemnum = D.data_partition(args.dataset, args.data_dir)
    for u in user_train:          # the training sequences include the validation item (bert4rec/trainer.py:165-167)
        user_train[u] = list(user_train[u]) + list(user_valid.get(u, []))
    if args.device_batches:
        train_ds = D.DeviceBertData(user_train, usernum, itemnum, args.maxlen, args.mask_prob, args.device, args.dupe_factor,
                                    args.prop_sliding_window)
    else:
        train_ds = D.BertTrainDataset(user_train, usernum, itemnum, args.maxlen, args.mask_prob, args.dataset_random_seed, args.dupe_factor,
                                      args.prop_sliding_window)
    sampler = D.PopularSampler(user_train, user_valid, user_test, usernum, itemnum, args.eval_negative_sample_size)
    val_ds = D.BertEvalDataset(user_train, user_valid, user_test, usernum, itemnum, args.maxlen, sampler, "val", args.eval_set_size)
    test_ds = D.BertEvalDataset(user_train, user_valid, user_test, usernum, itemnum, args.maxlen, sampler, "test", args.eval_set_size)
    if args.device_negatives:       # the host sampler is never called; one draw for the whole run, seeds 23 / 24 keep the two sets apart
        train_ds.add_eval(val_ds, candidates="device"), train_ds.add_eval(test_ds, candidates="device")
        train_ds.draw_eval("val", 23), train_ds.draw_eval("test", 24)
    elif args.device_batches:
        train_ds.add_eval(val_ds), train_ds.add_eval(test_ds)
    torch.manual_seed(23)
    model = BertModel(usernum, itemnum, args)
    if world > 1:
        torch.distributed.broadcast(model.master, 0)      # padded widths: the reference-shaped buffer travels, then push()
        model.push()
    trainer = FusedBertTrainer(model, lambda1, lambda2, lr=args.lr, betas=(0.9, 0.999), weight_decay=args.weight_decay, clip=args.clip,
                               process_group=pg, use_graph=args.use_graph, seed=23)
    rng = np.random.RandomState(23)

    def eval_batches(ds):
        return train_ds.eval_batches(ds.mode, args.eval_batch_size) if args.device_batches else ds.batches(args.eval_batch_size)
    best = dict(score=0.0, epoch=0, valid=None, test=None, auc_valid=0.0, auc_test=0.0)
    T, nseq = 0.0, 0
    for epoch in range(args.num_epochs):
        t0 = time.time()
        if args.device_batches:
            nseq += args.batch_size * _device_epoch(trainer, train_ds, args, rng, epoch if args.remask_every_epoch else 0, rank, world)
        else:
            for src, dec, lab in train_ds.epoch_batches(args.batch_size, rng):
                if len(src) != args.batch_size or skip_batch(len(src), world):
                    continue      # keep one captured graph shape (the reference's last partial batch is < 0.5 % of an epoch)
                if pg is None:
                    trainer.step(src, dec, lab)
                else:             # every rank draws the same global batch (same seed) and trains on its contiguous rows, with the
                    lo, hi = shard_bounds(len(src), rank, world)     # GLOBAL normalisers: label count, B*L*d, B*L*H of the whole batch
                    trainer.step(src[lo:hi], dec[lo:hi], lab[lo:hi], n_valid_global=int(np.count_nonzero(lab)), b_offset=lo,
                                 norms_scale=len(src) / float(hi - lo))
                nseq += len(src)
        torch.cuda.synchronize()
        T += time.time() - t0
        if (epoch + 1) % args.eval_interval == 0 or epoch + 1 == args.num_epochs:
            t_test, auc_test = trainer.evaluate(eval_batches(test_ds), device_scores=args.device_scores)
            t_valid, auc_valid = trainer.evaluate(eval_batches(val_ds), device_scores=args.device_scores)
            for k in (5, 10) if rank == 0 else ():
                print("epoch: %d, time: %f, valid (NDCG@%d: %.4f, HR@%d: %.4f, AUC: %s), test (NDCG@%d: %.4f, HR@%d: %.4f, AUC: %s)"
                      % (epoch + 1, T, k, t_valid[0][k], k, t_valid[1][k], auc_valid, k, t_test[0][k], k, t_test[1][k], auc_test))
            if args.eval_full:     # the held-out item against ALL unseen items (adt_full_rank), beside the sampled-negative metrics
                from ..sasrec.utils import evaluate_full
                f_test, _ = evaluate_full(model, test_ds, "test", (5, 10), args.eval_batch_size, process_group=pg)
                f_valid, _ = evaluate_full(model, val_ds, "val", (5, 10), args.eval_batch_size, process_group=pg)
                for k in (5, 10) if rank == 0 else ():
                    print("epoch: %d, full catalogue: valid (NDCG@%d: %.4f, HR@%d: %.4f), test (NDCG@%d: %.4f, HR@%d: %.4f)"
                          % (epoch + 1, k, f_valid[0][k], k, f_valid[1][k], k, f_test[0][k], k, f_test[1][k]))
            loss = float(trainer.loss())      # a collective under data parallelism: every rank calls it
            if rank == 0:
                print(json.dumps({"epoch": epoch + 1, "train_seconds": T, "sequences_per_sec": nseq / max(T, 1e-9), "loss": loss,
                                  "n_gpus": world, "valid": {"ndcg10": t_valid[0][10], "hr10": t_valid[1][10], "auc": auc_valid},
                                  "test": {"ndcg10": t_test[0][10], "hr10": t_test[1][10], "auc": auc_test}}), flush=True)
            if auc_valid >= best["score"]:
                best.update(score=auc_valid, epoch=epoch, valid=t_valid, test=t_test, auc_valid=auc_valid, auc_test=auc_test)
    if pg is not None:
        torch.distributed.destroy_process_group()
    return best


if __name__ == "__main__":
    main()
