"""STOSA-ADT: the host batch pipeline (DisenDataset.batch, matrix[users], the copies in model.stage) against batches built on the GPU
(--device_batches: DeviceDisenData / adt_seqbatch_build), at the Beauty template shape: B 256, eval batch 512, L 100, d 64, H 4, one
layer, dropout 0.3, bf16, captured step.  Reads only the seeded Beauty-shaped file it writes itself (stosa/main.py:_write_synthetic:
22,363 users, 12,101 items).

  python tools/bench_stosa_epoch.py [--out profiles/r13_stosa_device_batches.jsonl] [--reps 3]

One JSON line per measurement, each with median, min and max:
  (a) host_train_build / host_valid_build: the host build alone, ms per batch (40 training batches; 20 validation batches with
      matrix[users]), host clock;
  (b) device_train_stage / device_eval_batch: train_stage / eval_batch alone, ms per batch, HIP events;
  (c) train_epoch: one training epoch end to end (host clock around the loop of stosa/main.py, ending in a synchronise), sequences/s,
      host batches against device batches, alternating, `reps` epochs each after one warm-up epoch each;
  (d) valid_pass: one full-sort pass over all users (batches -> (N, 40) id lists; the metric scoring in Python that follows is the
      same for both and is timed once, as score_seconds), seconds, host against device batches, two-pass and --fused_eval;
  (e) scored_valid_pass: host clock from the first batch to the 13 scores in hand, ending in a synchronise, device batches: today's
      route (full_sort + get_full_sort_score) against --device_scores (full_sort_scores: adt_hit_hist, one 41-entry copy), two-pass and
      fused, alternating in one run;
  (f) search_eval: one SearcherEvolution.evaluate_candidates call over eight candidates on the full validation set, fused: all flags off
      against --device_batches --device_scores, alternating.
--parts picks the measurements (default abcdef); (e) and (f) are written to profiles/r14_stosa_device_scores.jsonl with --parts ef."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adt_amd.stosa import utils as U  # noqa: E402
from adt_amd.stosa.datasets import DeviceDisenData, DisenDataset, get_user_seqs  # noqa: E402
from adt_amd.stosa.main import _device_epoch, _write_synthetic, parse_args  # noqa: E402
from adt_amd.stosa.models import DisenDistSAModel  # noqa: E402
from adt_amd.stosa.trainer import FusedStosaTrainer, get_full_sort_score  # noqa: E402


def stats(xs, unit):
    return {"median_" + unit: float(np.median(xs)), "min_" + unit: float(min(xs)), "max_" + unit: float(max(xs)), "n": len(xs)}


def host_ms(fn, n):
    out = []
    for i in range(n):
        t0 = time.perf_counter()
        fn(i)
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def event_ms(fn, n, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for i in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--users", type=int, default=22363, help="users of the synthetic file (smaller: a rehearsal)")
    ap.add_argument("--parts", default="abcdef", help="which measurements to take, by letter")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stosa_epoch: no GPU (nothing here is measured on the CPU)")
    lines = []

    def emit(what, **kw):
        lines.append(dict({"what": what}, **kw))
        print(json.dumps(lines[-1]), flush=True)

    tmp = tempfile.mkdtemp()
    try:
        path = os.path.join(tmp, "Beauty.txt")
        _write_synthetic(path, users=cli.users)
        measure(cli, tmp, path, emit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def measure(cli, tmp, path, emit):
    user_seq, max_item, valid_matrix, test_matrix, num_users = get_user_seqs(path)
    args = U.set_template(parse_args(["--dataset", "Beauty"]))
    args.item_size, args.num_users, args.mask_id = max_item + 2, num_users, max_item + 1
    B, EB, L = args.batch_size, args.eval_batch_size, args.maxlen
    shape = {"users": num_users, "item_size": args.item_size, "B": B, "eval_B": EB, "L": L}
    lambda1, lambda2 = (x[:args.num_layers] for x in U.get_lambdas(args.dataset, args.topk))
    train_ds = DisenDataset(args, user_seq, "train", seed=args.seed)
    valid_ds = DisenDataset(args, user_seq, "valid", seed=args.seed + 1)
    model = DisenDistSAModel(args)
    trainer = FusedStosaTrainer(model, lambda1, lambda2, lr=args.lr, use_graph=True, seed=args.seed)
    dd = DeviceDisenData(user_seq, args.item_size, L, model.dev, valid_matrix, test_matrix)
    order = np.random.RandomState(1).permutation(num_users)
    dd.set_order(order)

    if "a" in cli.parts or "b" in cli.parts:
        # (a) the host build alone
        emit("host_train_build", **shape, **stats(host_ms(lambda i: train_ds.batch(order[i * B:(i + 1) * B]), 40), "ms"))

        def valid_build(i):
            users = np.arange(i * EB, (i + 1) * EB)
            valid_ds.batch(users)
            valid_matrix[users]
        emit("host_valid_build", **shape, **stats(host_ms(valid_build, 20), "ms"))
        # (b) the device build alone
        emit("device_train_stage", **shape, **stats(event_ms(lambda i: dd.train_stage(i * B, B, args.seed, i), 40), "ms"))
        emit("device_eval_batch", **shape, **stats(event_ms(lambda i: dd.eval_batch("valid", i * EB, EB), 20), "ms"))

    if "c" in cli.parts:
        # (c) one training epoch end to end
        def epoch(device):
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            if device:
                n = B * _device_epoch(trainer, dd, train_ds, args, trainer.nstep)
            else:
                for users, inp, dec, pos, neg, _ in train_ds.epoch_batches(B):
                    if len(users) == B:
                        trainer.step(inp, dec, pos, neg)
                        n += B
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)
        rates = {False: [], True: []}
        for rep in range(cli.reps + 1):
            for device in (False, True):
                r = epoch(device)
                if rep:                      # rep 0 warms both up (graph capture, first launches)
                    rates[device].append(r)
        for device in (False, True):
            emit("train_epoch", device_batches=device, **shape, **stats(rates[device], "sequences_per_sec"))
        emit("train_epoch_ratio", device_over_host=float(np.median(rates[True]) / np.median(rates[False])))

    # (d) one validation pass
    def batches(device):
        if device:
            return (dd.eval_batch("valid", s, min(EB, num_users - s)) for s in range(0, num_users, EB))
        return ((inp, valid_matrix[users], ans) for users, inp, _, _, _, ans in valid_ds.epoch_batches(EB, shuffle=False))
    if "d" in cli.parts:
        secs, preds = {}, {}
        for rep in range(cli.reps + 1):
            for fused in (False, True):
                for device in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pred, answers = trainer.full_sort(batches(device), fused=fused)
                    dt = time.perf_counter() - t0
                    preds[(fused, device)] = pred
                    if rep:
                        secs.setdefault((fused, device), []).append(dt)
        for fused in (False, True):
            for device in (False, True):
                emit("valid_pass", fused_eval=fused, device_batches=device, **shape, **stats(secs[(fused, device)], "seconds"))
            emit("valid_pass_ratio", fused_eval=fused, host_over_device_seconds=float(np.median(secs[(fused, False)]) / np.median(secs[(fused, True)])),
                 same_id_lists=bool(np.array_equal(preds[(fused, False)], preds[(fused, True)])))
        t0 = time.perf_counter()
        get_full_sort_score(answers, pred)
        emit("score_seconds", seconds=time.perf_counter() - t0)
    # (e) one validation pass to the 13 scores in hand
    def stages():
        return (dd.eval_stage("valid", s, min(EB, num_users - s)) for s in range(0, num_users, EB))
    if "e" in cli.parts:
        secs, scores = {}, {}
        for rep in range(cli.reps + 1):
            for fused in (False, True):
                for device_scores in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if device_scores:
                        sc = trainer.full_sort_scores(stages(), fused=fused)[0]
                    else:
                        pred, answers = trainer.full_sort(batches(True), fused=fused)
                        sc = get_full_sort_score(answers, pred)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    scores[(fused, device_scores)] = sc
                    if rep:
                        secs.setdefault((fused, device_scores), []).append(dt)
        for fused in (False, True):
            for device_scores in (False, True):
                emit("scored_valid_pass", fused_eval=fused, device_scores=device_scores, **shape, **stats(secs[(fused, device_scores)], "seconds"))
            emit("scored_valid_pass_ratio", fused_eval=fused,
                 today_over_device_scores_seconds=float(np.median(secs[(fused, False)]) / np.median(secs[(fused, True)])),
                 max_score_difference=float(np.abs(np.array(scores[(fused, False)]) - np.array(scores[(fused, True)])).max()),
                 fused_fallbacks=int(trainer.fused_fallbacks))

    # (f) the search: eight candidates over the full validation set
    if "f" in cli.parts:
        from adt_amd.stosa import evolution as ev
        sargs = ev.parse_args(["--dataset", "Beauty", "--data_dir", tmp + "/", "--device_batches"])
        sargs.data_file = path
        torch.manual_seed(sargs.seed)
        searcher = ev.SearcherEvolution(sargs)
        r = np.random.RandomState(2)
        cands = [[float(x) for x in r.rand(2 * sargs.num_layers)] for _ in range(8)]
        secs, outs = {False: [], True: []}, {}
        for rep in range(cli.reps + 1):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[on] = searcher.evaluate_candidates(cands, fused=True, device_batches=on, device_scores=on)
                torch.cuda.synchronize()
                if rep:
                    secs[on].append(time.perf_counter() - t0)
        sshape = dict(shape, L=sargs.maxlen, candidates=len(cands))
        for on in (False, True):
            emit("search_eval", fused_eval=True, device_batches=on, device_scores=on, **sshape, **stats(secs[on], "seconds"))
        emit("search_eval_ratio", off_over_on_seconds=float(np.median(secs[False]) / np.median(secs[True])),
             max_score_difference=float(max(abs(a[k] - b[k]) for a, b in zip(outs[False], outs[True]) for k in a)))


if __name__ == "__main__":
    main()
