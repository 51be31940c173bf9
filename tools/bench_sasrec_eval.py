#!/usr/bin/env python3
"""Wall clock of SASRec-ADT's sampled evaluation in its three forms, at the ml-1m template shape on the synthetic
`ml1m` preset (6,040 users, 3,416 items, sample_size 100, L 200):

    host                            PopularSampler + EvalDataset(frozen) + evaluate_loader          (the path without the new flags)
    device_eval                     the same frozen candidates uploaded once; batches and scores on the device
    device_eval+device_negatives    the candidates drawn by adt_evalcand_draw as well

and of three things, in one run: start-up to the first evaluation batch (validation set), one scored validation pass (host clock around
the loop, ending in a synchronise), and one SearcherEvolution.evaluate_candidates pass of 32 candidates (the search's default supernet:
d 64, 2 heads, 2 layers).  The forms alternate, one warm-up of each, then --reps repetitions; one JSON line per (case, form) with the
median and the range.

    python tools/bench_sasrec_eval.py --data_dir data --out profiles/r17_sasrec_device_eval.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from adt_amd.sasrec import utils as U  # noqa: E402
from adt_amd.sasrec.device_eval import DeviceEvalData  # noqa: E402

FORMS = ("host", "device_eval", "device_eval+device_negatives")


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", default="data")
    ap.add_argument("--out", default="profiles/r17_sasrec_device_eval.jsonl")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    assert a.reps >= 3
    path = os.path.join(a.data_dir, "ml-1m.txt")
    if not os.path.exists(path):
        from adt_amd.sasrec import synth
        os.makedirs(a.data_dir, exist_ok=True)
        synth.write(path, synth.generate("ml1m", 23)[0])
    split = U.data_partition("ml-1m", a.data_dir)
    train, valid, test, usernum, itemnum = split
    from adt_amd.sasrec import main as M
    margs = M.parse_args(["--dataset", "ml-1m", "--train_dir", "bench"])      # the ml-1m template: d 256, H 2, L 200, 2 layers, S 100, eval batch 512
    margs.device = a.device
    S, L, EB = margs.sample_size, margs.maxlen, margs.eval_batch_size

    # ---- start-up to the first evaluation batch ---------------------------------------------------------------------------------------
    def startup(form):
        sampler = U.PopularSampler(train, valid, test, usernum, itemnum, S)
        ds = U.EvalDataset(train, valid, test, usernum, itemnum, L, sampler, "val", -1, form != FORMS[2])
        if form == FORMS[0]:
            (_, seq, items), _ = next(iter(ds.batches(EB)))
            return ds, None, (torch.from_numpy(seq).to(a.device), torch.from_numpy(items).to(a.device))
        data = DeviceEvalData.from_dataset(ds, a.device, upload=form == FORMS[1])
        if form == FORMS[2]:
            data.draw(23, 0)
        return ds, data, data.batch(0, min(EB, len(data)))

    # ---- one scored validation pass ---------------------------------------------------------------------------------------------------
    from adt_amd.sasrec.model_wide import SASRecADTWide
    torch.manual_seed(23)
    model = SASRecADTWide(usernum, itemnum, margs)
    for _, prm in model.named_parameters():
        if prm.dim() > 1:
            torch.nn.init.xavier_normal_(prm.data)
    model.push()
    model.eval()

    def valid_pass(form, ds, data):
        if form == FORMS[0]:
            return U.evaluate_loader(model, ds.batches(EB), None, "val", (5, 10))
        return U.evaluate_device(model, data, (5, 10), EB)

    # ---- one evaluate_candidates pass -------------------------------------------------------------------------------------------------
    from adt_amd.sasrec import evolution as ev
    eargs = ev.parse_args(["--dataset", "ml-1m", "--data_dir", a.data_dir, "--device", a.device])
    ev.set_rng_seed(eargs.seed)
    searcher = ev.SearcherEvolution(eargs)      # its own frozen validation set (the host form's)
    sdata = DeviceEvalData.from_dataset(searcher.val_ds, a.device)      # the search's own candidates on the device: the host form's records
    cands = [[float(x) for x in np.random.RandomState(1).rand(2 * eargs.num_layers)] for _ in range(a.candidates)]

    def search_pass(form, data):
        searcher.val_dev = None if form == FORMS[0] else data
        return searcher.evaluate_candidates(cands, group=32)

    times = {(c, f): [] for c in ("startup", "valid_pass", "evaluate_candidates") for f in FORMS}
    results = {}
    for rep in range(a.reps + 1):      # repetition 0 is the warm-up of each form
        for form in FORMS:
            t, (ds, data, _) = clock(lambda: startup(form))
            t2, res = clock(lambda: valid_pass(form, ds, data))
            t3, recs = clock(lambda: search_pass(form, data if form == FORMS[2] else (None if form == FORMS[0] else sdata)))
            results[form] = (res, recs)
            if rep:
                for case, x in (("startup", t), ("valid_pass", t2), ("evaluate_candidates", t3)):
                    times[(case, form)].append(x)
    # the two forms with the host's candidates agree; say so in the file
    (h_res, h_recs), (d_res, d_recs) = results[FORMS[0]], results[FORMS[1]]
    agree = abs(h_res[1] - d_res[1]) <= len(valid) * 2.0 ** -52 and all(abs(x["auc"] - y["auc"]) <= 1e-12 for x, y in zip(h_recs, d_recs))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for (case, form), ts in times.items():
            rec = {"case": case, "form": form, "median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts),
                   "users": usernum, "items": itemnum, "sample_size": S, "maxlen": L, "eval_batch_size": EB,
                   "model": "SASRecADTWide d %d H %d, %d layers, %s" % (margs.hidden_units, margs.num_heads, margs.num_layers, margs.precision)
                   if case == "valid_pass" else ("SuperSASRecModel d %d H %d, %d layers, %d candidates" % (
                       eargs.hidden_units, eargs.num_heads, eargs.num_layers, a.candidates) if case == "evaluate_candidates" else None),
                   "host_and_device_eval_agree": bool(agree), "device": torch.cuda.get_device_name(0)}
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
