#!/usr/bin/env python3
"""Wall clock of SASRec-ADT's full-catalogue evaluation on the host and on the device, on the synthetic `ml1m`
preset (6,040 users, 3,416 items), evaluation batch 512:

    valid_pass            one validation pass of the flagship model (SASRecADT d 64, 2 heads, 2 blocks, L 200, bf16):
                            host    evaluate_full         sequences and seen CSR built in Python and uploaded per batch, ranks read back
                            device  evaluate_full_device  batches from the resident DeviceEvalData, one histogram and one sum read back
    evaluate_candidates   one SearcherEvolution.evaluate_candidates pass of 32 candidates (the search's default supernet):
                            sampled --device_eval true    1 + 100 sampled items per user (adt_cand_rank_hist)
                            full    --eval_full true      the whole catalogue (adt_full_rank_groups + adt_full_rank_stats)

Host clock around each pass, ending in a synchronise.  The two forms of a case alternate: one warm-up round, then --reps timed rounds.
One JSON line per (case, form) with the median and the range, APPENDED to --out; the valid_pass lines carry the ratio, the bytes read
back per pass and whether the device median lies within the larger spread of the host median.

    python tools/bench_sasrec_full_eval.py --data_dir data --out profiles/r31_full_eval_device.jsonl
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

KS = (5, 10)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(forms, reps):
    """{name: (times, last result)}: one call of each form per round, in the given order; round 0 is the warm-up."""
    out = {k: ([], None) for k in forms}
    for rep in range(reps + 1):
        for k, fn in forms.items():
            t, res = clock(fn)
            out[k] = (out[k][0] + ([t] if rep else []), res)
    return out


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "reps": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", default="data")
    ap.add_argument("--out", default="profiles/r31_full_eval_device.jsonl")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--candidates", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    path = os.path.join(a.data_dir, "ml-1m.txt")
    if not os.path.exists(path):
        from adt_amd.sasrec import synth
        os.makedirs(a.data_dir, exist_ok=True)
        synth.write(path, synth.generate("ml1m", 23)[0])
    train, valid, test, usernum, itemnum = U.data_partition("ml-1m", a.data_dir)
    from adt_amd.sasrec import main as M
    from adt_amd.sasrec.model import SASRecADT
    margs = M.parse_args(["--dataset", "ml-1m", "--train_dir", "bench", "--no_template", "--hidden_units", "64", "--num_heads", "2", "--maxlen", "200",
                          "--num_layers", "2", "--device", a.device])
    EB = margs.eval_batch_size
    torch.manual_seed(23)
    model = SASRecADT(usernum, itemnum, margs).to(a.device)
    for _, prm in model.named_parameters():
        try:
            torch.nn.init.xavier_normal_(prm.data)
        except Exception:
            pass
    model.eval()
    sampler = U.PopularSampler(train, valid, test, usernum, itemnum, margs.sample_size)
    ds = U.EvalDataset(train, valid, test, usernum, itemnum, margs.maxlen, sampler, "val", -1, False)
    data = DeviceEvalData.from_dataset(ds, a.device, upload=False)
    common = {"users": len(ds.users), "items": itemnum, "eval_batch_size": EB, "device_name": torch.cuda.get_device_name(0)}
    lines = []

    # ---- one validation pass ------------------------------------------------------------------------------------------------------------
    res = alternate({"host": lambda: U.evaluate_full(model, ds, "val", KS, EB), "device": lambda: U.evaluate_full_device(model, data, KS, EB)}, a.reps)
    (h_t, ((h_nd, h_hr), h_auc)), (d_t, ((d_nd, d_hr), d_auc)) = res["host"], res["device"]
    tol = len(ds.users) * 2.0 ** -52
    agree = all(h_hr[k] == d_hr[k] and abs(h_nd[k] - d_nd[k]) <= tol * abs(h_nd[k]) for k in KS) and abs(h_auc - d_auc) <= tol * abs(h_auc)
    hs, dv = stats(h_t), stats(d_t)
    spread = max(hs["max_s"] - hs["min_s"], dv["max_s"] - dv["min_s"])
    model_name = "SASRecADT d %d H %d, %d blocks, L %d, %s" % (margs.hidden_units, margs.num_heads, margs.num_layers, margs.maxlen, margs.precision)
    for form, st, back in (("host", hs, 8 * len(ds.users)), ("device", dv, 8 * (max(KS) + 1) + 8)):      # rank + n_elig int32 per user | one histogram, one sum
        lines.append(dict(common, case="valid_pass", form=form, model=model_name, bytes_read_back=back, device_over_host=dv["median_s"] / hs["median_s"],
                          host_and_device_agree=bool(agree), accepted=bool(dv["median_s"] <= hs["median_s"] + spread), **st))

    # ---- one evaluate_candidates pass ---------------------------------------------------------------------------------------------------
    from adt_amd.sasrec import evolution as ev
    eargs = ev.parse_args(["--dataset", "ml-1m", "--data_dir", a.data_dir, "--device", a.device, "--device_eval", "true", "--eval_full", "true"])
    ev.set_rng_seed(eargs.seed)
    searcher = ev.SearcherEvolution(eargs)
    cands = [[float(x) for x in np.random.RandomState(1).rand(2 * eargs.num_layers)] for _ in range(a.candidates)]

    def search_pass(full):
        searcher.eval_full = full
        return searcher.evaluate_candidates(cands, group=32)
    res = alternate({"sampled": lambda: search_pass(False), "full": lambda: search_pass(True)}, a.reps)
    super_name = "SuperSASRecModel d %d H %d, %d layers, L %d, %d candidates" % (eargs.hidden_units, eargs.num_heads, eargs.num_layers, eargs.maxlen,
                                                                               a.candidates)
    ratio = float(np.median(res["full"][0]) / np.median(res["sampled"][0]))
    for form in ("sampled", "full"):
        back = a.candidates * (8 * (1 + eargs.sample_size) if form == "sampled" else 8 * 11 + 8)
        lines.append(dict(common, case="evaluate_candidates", form=form, model=super_name, bytes_read_back=back, full_over_sampled=ratio,
                          sample_size=eargs.sample_size, **stats(res[form][0])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
