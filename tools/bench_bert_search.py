"""BERT4Rec-ADT lambda search and evaluation: the host forms (BertTrainDataset, BertEvalDataset.batches, ranks read back per pass,
PopularSampler) against the device-resident ones (--device_batches / --device_scores / --device_negatives), at the
ml-1m template shape: B 256, eval batch 256, L 200, d 256, H 4, 2 + 2 layers, mask_prob 0.2, dupe_factor 10, prop_sliding_window 0.5,
100 sampled negatives, bf16.  Reads only the seeded synthetic ml-1m file it writes itself (sasrec/synth.py: 6,040 users, 3,416 items).

  python tools/bench_bert_search.py [--out profiles/r28_bert_device_search.jsonl] [--reps 3] [--epoch_steps 0]

One JSON line per measurement, each with median, min and max; host and device forms alternate inside every repetition, after one warm-up
of each:
  (a) search_startup: seconds from the parsed user_train to the first warm-up batch staged on the device (host clock, ending in a
      synchronise), and the bytes of host arrays the form then holds;
  (b) warmup_epoch: one warm-up epoch of the supernet (SuperBertTrainer.step on host batches / step_device on device batches), host
      clock ending in a synchronise, sequences/s (--epoch_steps caps the steps of an epoch; default: the whole epoch);
  (c) evaluate_candidates: one call for 16 and for 32 candidates over the validation users, seconds, in three forms: host batches +
      host scores, device batches + host scores, device batches + device scores (same candidates, so the records are compared);
      --group sets the candidates per pass (default: evaluate_candidates' own 16);
  (d) valid_pass: one scored validation pass of main.py's trainer (FusedBertTrainer.evaluate on device batches), with and without
      device_scores;
  (e) add_eval: DeviceBertData.add_eval with host candidates (a fresh PopularSampler each time: its cache is what is being timed) and
      with device candidates followed by draw_eval, ending in a synchronise.
--parts picks the measurements (default abcde); --preset picks the synthetic file (smaller: a rehearsal)."""
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
from adt_amd.bert4rec import evolution as ev  # noqa: E402
from adt_amd.bert4rec import utils as U  # noqa: E402
from adt_amd.bert4rec.main import parse_args as main_args  # noqa: E402
from adt_amd.bert4rec.model import BertModel  # noqa: E402
from adt_amd.bert4rec.trainer import FusedBertTrainer  # noqa: E402
from adt_amd.sasrec import synth  # noqa: E402


def stats(xs, unit):
    return {"median_" + unit: float(np.median(xs)), "min_" + unit: float(min(xs)), "max_" + unit: float(max(xs)), "n": len(xs)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--preset", default="ml1m", help="synthetic preset of sasrec/synth.py (smaller: a rehearsal)")
    ap.add_argument("--epoch_steps", type=int, default=0, help="cap on the steps of a timed warm-up epoch (0: the whole epoch)")
    ap.add_argument("--parts", default="abcde", help="which measurements to take, by letter")
    ap.add_argument("--group", type=int, default=16, help="candidates per pass of evaluate_candidates (its own default: 16)")
    ap.add_argument("--override", default=None, help="JSON applied after the template (a rehearsal at a small shape)")
    cli = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bert_search: no GPU (nothing here is measured on the CPU)")
    lines = []

    def emit(what, **kw):
        lines.append(dict({"what": what}, **kw))
        print(json.dumps(lines[-1]), flush=True)

    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    try:
        hist, _, _ = synth.generate(cli.preset, 23)
        synth.write(os.path.join(tmp, "ml-1m.txt"), hist)
        os.chdir(tmp)
        measure(cli, tmp, emit)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def templated(args, cli):
    args = U.set_template(args)
    for k, v in (json.loads(cli.override) if cli.override else {}).items():
        setattr(args, k, v)
    return args


def measure(cli, tmp, emit):
    args = templated(ev.parse_args(["--dataset", "ml-1m", "--data_dir", tmp, "--device_batches"]), cli)
    ev.set_rng_seed(args.seed)
    t, s = timed(lambda: ev.SearcherEvolution(args))      # the resident data and both host evaluation sets; no BertTrainDataset
    user_train, user_valid, user_test, usernum, itemnum = s.dataset
    B, EB, L, seed = args.batch_size, args.eval_batch_size, args.maxlen, args.dataset_random_seed
    shape = {"users": usernum, "items": itemnum, "B": B, "eval_B": EB, "L": L, "d": args.hidden_units, "H": args.num_heads,
             "dupe_factor": args.dupe_factor, "prop_sliding_window": args.prop_sliding_window, "mask_prob": args.mask_prob,
             "negatives": args.eval_negative_sample_size, "precision": args.precision, "examples": len(s.dev_data),
             "val_users": len(s.val_ds)}
    emit("searcher_construction", device_batches=True, seconds=t, supernet_parameters=int(s.model.flat.numel()), **shape)

    def host_data():
        return D.BertTrainDataset(user_train, usernum, itemnum, L, args.mask_prob, seed, args.dupe_factor, args.prop_sliding_window)

    def device_data():
        return D.DeviceBertData(user_train, usernum, itemnum, L, args.mask_prob, s.model.dev, args.dupe_factor, args.prop_sliding_window)

    # (a) from the parsed sequences to the first warm-up batch staged on the device
    train_ds = None
    secs = {False: [], True: []}
    for rep in range(cli.reps + 1 if "a" in cli.parts else 1):
        for device in (False, True):
            if device:
                def first():
                    dd = device_data()
                    dd.set_order(np.random.RandomState(23).permutation(len(dd)))
                    dd.train_stage(0, B, seed, 0)
                    return dd
            else:
                def first():
                    ds = host_data()
                    s.trainer._stage(*next(ds.epoch_batches(B, np.random.RandomState(23))))
                    return ds
            t, out = timed(first)
            if device:
                dd = out
            else:
                train_ds = out
            if rep:
                secs[device].append(t)
    assert len(dd) == len(train_ds) == len(s.dev_data), (len(dd), len(train_ds))
    if "a" in cli.parts:
        host_bytes = int(train_ds.src.nbytes + train_ds.dec.nbytes + train_ds.labels.nbytes)
        dev_bytes = int(sum(t.numel() * t.element_size() for t in (dd.seq_off, dd.seq_items, dd.win_start, dd.win_len, dd.order)))
        emit("search_startup", device_batches=False, host_array_bytes=host_bytes, **shape, **stats(secs[False], "seconds"))
        emit("search_startup", device_batches=True, host_array_bytes=0, device_resident_bytes=dev_bytes, **shape, **stats(secs[True], "seconds"))
    del dd

    # (b) one warm-up epoch of the supernet
    if "b" in cli.parts:
        data = s.dev_data
        steps = len(data) // B if cli.epoch_steps <= 0 else min(cli.epoch_steps, len(data) // B)

        def epoch(device, rep):
            rng = np.random.RandomState(100 + rep)
            s.trainer.set_choice(s.search_state.sample_random())

            def run():
                if device:
                    data.set_order(rng.permutation(len(data)))
                    for i in range(steps):
                        s.trainer.step_device(data.train_stage(i * B, B, seed, 0))
                else:
                    for i, (src, dec, lab) in enumerate(train_ds.epoch_batches(B, rng)):
                        if i == steps:
                            break
                        s.trainer.step(src, dec, lab)
            return steps * B / timed(run)[0]
        rates = {False: [], True: []}
        for rep in range(cli.reps + 1):
            for device in (False, True):
                r = epoch(device, rep)
                if rep:
                    rates[device].append(r)
        for device in (False, True):
            emit("warmup_epoch", device_batches=device, steps=steps, loss=float(s.trainer.loss()), **shape, **stats(rates[device], "sequences_per_sec"))
        emit("warmup_epoch_ratio", device_over_host=float(np.median(rates[True]) / np.median(rates[False])))
    del train_ds

    # (c) one evaluate_candidates call over the validation users
    if "c" in cli.parts:
        forms = [("host_batches_host_scores", False, False), ("device_batches_host_scores", True, False), ("device_batches_device_scores", True, True)]
        r = np.random.RandomState(2)
        for _ in s.val_ds.batches(EB):      # fills the sampler's cache, so that no timed pass samples
            pass
        for P in (16, 32):
            cands = [[float(x) for x in r.rand(2 * args.num_layers)] for _ in range(P)]
            secs, recs = {f[0]: [] for f in forms}, {}
            for rep in range(cli.reps + 1):
                for tag, db, dsc in forms:
                    t, recs[tag] = timed(lambda: s.evaluate_candidates(cands, group=cli.group, device_batches=db, device_scores=dsc))
                    if rep:
                        secs[tag].append(t)
            base = recs[forms[0][0]]
            for tag, db, dsc in forms:
                same_hr = all(a["V_HR"] == b["V_HR"] for a, b in zip(base, recs[tag]))
                worst = max(abs(a["V_AUC"] - b["V_AUC"]) / abs(a["V_AUC"]) for a, b in zip(base, recs[tag]))
                emit("evaluate_candidates", form=tag, candidates=P, group=cli.group, same_hr_as_host=bool(same_hr), worst_relative_auc_difference=float(worst), **shape,
                     **stats(secs[tag], "seconds"))
            emit("evaluate_candidates_ratio", candidates=P,
                 **{"host_over_" + tag: float(np.median(secs[forms[0][0]]) / np.median(secs[tag])) for tag, _, _ in forms[1:]})

    # (d), (e): main.py's trainer and data (the training sequences include the validation item there)
    if "d" in cli.parts or "e" in cli.parts:
        margs = templated(main_args(["--dataset", "ml-1m", "--data_dir", tmp, "--device_batches"]), cli)
        merged = {u: list(user_train[u]) + list(user_valid.get(u, [])) for u in user_train}
        dev = s.model.dev
        del s
        torch.cuda.empty_cache()
        dd = D.DeviceBertData(merged, usernum, itemnum, L, margs.mask_prob, dev, margs.dupe_factor, margs.prop_sliding_window)

        def eval_sets():
            sampler = D.PopularSampler(merged, user_valid, user_test, usernum, itemnum, margs.eval_negative_sample_size)
            return D.BertEvalDataset(merged, user_valid, user_test, usernum, itemnum, L, sampler, "val", margs.eval_set_size)

    if "e" in cli.parts:
        secs = {"host": [], "device": []}
        for rep in range(cli.reps + 1):
            for kind in ("host", "device"):
                ds = eval_sets()

                def add():
                    dd.add_eval(ds, candidates=kind)
                    if kind == "device":
                        dd.draw_eval("val", 23)
                t, _ = timed(add)
                if rep:
                    secs[kind].append(t)
        for kind in ("host", "device"):
            emit("add_eval", candidates=kind, val_users=len(ds), negatives=margs.eval_negative_sample_size, **stats(secs[kind], "seconds"))
        emit("add_eval_ratio", host_over_device_seconds=float(np.median(secs["host"]) / np.median(secs["device"])))

    if "d" in cli.parts:
        lambda1, lambda2 = U.get_lambda(margs.dataset, margs.topk)
        torch.manual_seed(23)
        trainer = FusedBertTrainer(BertModel(usernum, itemnum, margs), lambda1, lambda2, lr=margs.lr, weight_decay=margs.weight_decay, clip=margs.clip)
        dd.add_eval(eval_sets())
        secs, metrics = {False: [], True: []}, {}
        for rep in range(cli.reps + 1):
            for dsc in (False, True):
                t, metrics[dsc] = timed(lambda: trainer.evaluate(dd.eval_batches("val", EB), device_scores=dsc))
                if rep:
                    secs[dsc].append(t)
        for dsc in (False, True):
            emit("valid_pass", device_batches=True, device_scores=dsc, val_users=dd.eval_len("val"), **stats(secs[dsc], "seconds"))
        (nd0, hr0), auc0 = metrics[False]
        (nd1, hr1), auc1 = metrics[True]
        emit("valid_pass_ratio", host_over_device_scores_seconds=float(np.median(secs[False]) / np.median(secs[True])), same_hr=bool(hr0 == hr1),
             relative_auc_difference=float(abs(auc0 - auc1) / abs(auc0)), relative_ndcg10_difference=float(abs(nd0[10] - nd1[10]) / abs(nd0[10])))


if __name__ == "__main__":
    main()
