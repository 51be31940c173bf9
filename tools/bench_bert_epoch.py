"""BERT4Rec-ADT: the host batch pipeline (BertTrainDataset, the fancy-indexed batch, BertModel.stage, BertEvalDataset.batches) against
batches masked and built on the GPU (--device_batches: DeviceBertData / adt_bertbatch_build), at the ml-1m template shape: B 256, L 200,
d 256, H 4, 2 + 2 layers, mask_prob 0.2, dupe_factor 10, prop_sliding_window 0.5, bf16, captured step.  Reads only the seeded synthetic
ml-1m file it writes itself (sasrec/synth.py: 6,040 users, 3,416 items).

  python tools/bench_bert_epoch.py [--out profiles/r15_bert_device_batches.jsonl] [--reps 3]

One JSON line per measurement, each with median, min and max; host and device paths alternate in one run:
  (a) startup: seconds from the parsed user_train to the first training batch staged on the device (host clock, ending in a
      synchronise), and the bytes of host arrays the path then holds;
  (b) host_train_build: fancy-indexing one 256-row batch and BertModel.stage's np.nonzero compaction, host clock, before any upload;
      host_train_stage: the same plus the uploads of BertModel.stage, ending in a synchronise; device_train_stage: train_stage alone,
      HIP events;
  (c) train_epoch: one training epoch end to end (host clock around the loop of bert4rec/main.py, ending in a synchronise), sequences/s,
      `reps` epochs each after one warm-up epoch each (--epoch_steps caps the steps of an epoch; default: the whole epoch);
  (d) valid_pass: one FusedBertTrainer.evaluate pass over the validation users, seconds.
--parts picks the measurements (default abcd); --preset picks the synthetic file (smaller: a rehearsal)."""
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
from adt_amd.bert4rec import datasets as D  # noqa: E402
from adt_amd.bert4rec import utils as U  # noqa: E402
from adt_amd.bert4rec.main import parse_args  # noqa: E402
from adt_amd.bert4rec.model import BertModel  # noqa: E402
from adt_amd.bert4rec.trainer import FusedBertTrainer  # noqa: E402
from adt_amd.sasrec import synth  # noqa: E402


def stats(xs, unit):
    return {"median_" + unit: float(np.median(xs)), "min_" + unit: float(min(xs)), "max_" + unit: float(max(xs)), "n": len(xs)}


def host_ms(fn, n, warmup=3):
    for i in range(warmup):
        fn(i)
    out = []
    for i in range(n):
        t0 = time.perf_counter()
        fn(warmup + i)
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
        fn(warmup + i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--preset", default="ml1m", help="synthetic preset of sasrec/synth.py (smaller: a rehearsal)")
    ap.add_argument("--epoch_steps", type=int, default=0, help="cap on the steps of a timed epoch (0: the whole epoch)")
    ap.add_argument("--parts", default="abcd", help="which measurements to take, by letter")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bert_epoch: no GPU (nothing here is measured on the CPU)")
    lines = []

    def emit(what, **kw):
        lines.append(dict({"what": what}, **kw))
        print(json.dumps(lines[-1]), flush=True)

    tmp = tempfile.mkdtemp()
    try:
        hist, _, _ = synth.generate(cli.preset, 23)
        synth.write(os.path.join(tmp, "ml-1m.txt"), hist)
        measure(cli, tmp, emit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def measure(cli, tmp, emit):
    args = U.set_template(parse_args(["--dataset", "ml-1m", "--data_dir", tmp]))
    user_train, user_valid, user_test, usernum, itemnum = D.data_partition(args.dataset, args.data_dir)
    for u in user_train:
        user_train[u] = list(user_train[u]) + list(user_valid.get(u, []))
    B, EB, L, seed = args.batch_size, args.eval_batch_size, args.maxlen, args.dataset_random_seed
    lambda1, lambda2 = U.get_lambda(args.dataset, args.topk)
    torch.manual_seed(23)
    model = BertModel(usernum, itemnum, args)
    trainer = FusedBertTrainer(model, lambda1, lambda2, lr=args.lr, weight_decay=args.weight_decay, clip=args.clip, use_graph=True, seed=23)
    shape = {"users": usernum, "items": itemnum, "B": B, "eval_B": EB, "L": L, "d": args.hidden_units, "dupe_factor": args.dupe_factor,
             "prop_sliding_window": args.prop_sliding_window, "mask_prob": args.mask_prob}

    def host_data():
        return D.BertTrainDataset(user_train, usernum, itemnum, L, args.mask_prob, seed, args.dupe_factor, args.prop_sliding_window)

    def device_data():
        return D.DeviceBertData(user_train, usernum, itemnum, L, args.mask_prob, model.dev, args.dupe_factor, args.prop_sliding_window)

    # (a) from the parsed sequences to the first batch staged on the device
    secs = {False: [], True: []}
    for rep in range(cli.reps if "a" in cli.parts else 1):
        for device in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if device:
                dd = device_data()
                dd.set_order(np.random.RandomState(23).permutation(len(dd)))
                dd.train_stage(0, B, seed, 0)
            else:
                train_ds = host_data()
                src, dec, lab = next(train_ds.epoch_batches(B, np.random.RandomState(23)))
                trainer.stage(src, dec, lab)
            torch.cuda.synchronize()
            secs[device].append(time.perf_counter() - t0)
    shape["examples"] = len(train_ds)
    assert len(dd) == len(train_ds), (len(dd), len(train_ds))
    if "a" in cli.parts:
        host_bytes = int(train_ds.src.nbytes + train_ds.dec.nbytes + train_ds.labels.nbytes)
        dev_bytes = int(sum(t.numel() * t.element_size() for t in (dd.seq_off, dd.seq_items, dd.win_start, dd.win_len, dd.order)))
        emit("startup", device_batches=False, host_array_bytes=host_bytes, **shape, **stats(secs[False], "seconds"))
        emit("startup", device_batches=True, host_array_bytes=0, device_resident_bytes=dev_bytes, **shape, **stats(secs[True], "seconds"))

    order = np.random.RandomState(1).permutation(len(dd))
    dd.set_order(order)
    if "b" in cli.parts:
        def gather_compact(i):
            idx = order[i * B:(i + 1) * B]
            src, dec, lab = train_ds.src[idx], train_ds.dec[idx], train_ds.labels[idx]
            flat = lab.reshape(-1)
            rows = np.nonzero(flat)[0].astype(np.int32)
            return src, dec, lab, rows, flat[rows]

        def host_stage(i):
            idx = order[i * B:(i + 1) * B]
            trainer.stage(train_ds.src[idx], train_ds.dec[idx], train_ds.labels[idx])
            torch.cuda.synchronize()
        emit("host_train_build", **shape, **stats(host_ms(gather_compact, 40), "ms"))
        emit("host_train_stage", **shape, **stats(host_ms(host_stage, 40), "ms"))
        emit("device_train_stage", **shape, **stats(event_ms(lambda i: dd.train_stage(i * B, B, seed, 0), 40), "ms"))

    if "c" in cli.parts:
        steps = len(dd) // B if cli.epoch_steps <= 0 else min(cli.epoch_steps, len(dd) // B)

        def epoch(device, rep):
            rng = np.random.RandomState(100 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if device:
                dd.set_order(rng.permutation(len(dd)))
                for i in range(steps):
                    trainer.step_device(dd.train_stage(i * B, B, seed, 0))
            else:
                for i, (src, dec, lab) in enumerate(train_ds.epoch_batches(B, rng)):
                    if i == steps:
                        break
                    trainer.step(src, dec, lab)
            torch.cuda.synchronize()
            return steps * B / (time.perf_counter() - t0)
        rates = {False: [], True: []}
        for rep in range(cli.reps + 1):
            for device in (False, True):
                r = epoch(device, rep)
                if rep:                      # rep 0 warms both up (graph capture, first launches)
                    rates[device].append(r)
        for device in (False, True):
            emit("train_epoch", device_batches=device, steps=steps, **shape, **stats(rates[device], "sequences_per_sec"))
        emit("train_epoch_ratio", device_over_host=float(np.median(rates[True]) / np.median(rates[False])))

    if "d" in cli.parts:
        sampler = D.PopularSampler(user_train, user_valid, user_test, usernum, itemnum, args.eval_negative_sample_size)
        val_ds = D.BertEvalDataset(user_train, user_valid, user_test, usernum, itemnum, L, sampler, "val", args.eval_set_size)
        t0 = time.perf_counter()
        dd.add_eval(val_ds)                  # also fills the sampler's cache, so that neither timed pass below samples
        emit("add_eval", seconds=time.perf_counter() - t0, users=len(val_ds))
        secs, metrics = {False: [], True: []}, {}
        for rep in range(cli.reps + 1):
            for device in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                metrics[device] = trainer.evaluate(dd.eval_batches("val", EB) if device else val_ds.batches(EB))
                torch.cuda.synchronize()
                if rep:
                    secs[device].append(time.perf_counter() - t0)
        for device in (False, True):
            emit("valid_pass", device_batches=device, **shape, **stats(secs[device], "seconds"))
        emit("valid_pass_ratio", host_over_device_seconds=float(np.median(secs[False]) / np.median(secs[True])),
             same_metrics=bool(metrics[False] == metrics[True]))


if __name__ == "__main__":
    main()
