#!/usr/bin/env python3
"""The lambda searches at a padded width, one JSON line per measurement.

  python tools/bench_super_lanes.py [--parts kp] [--out profiles/r30_super_lanes.jsonl]

  (k) the grouped KL full sort at the Beauty shape (12,103 items, E 512, eight stacked groups): adt_kldist_full_groups_lanes at 50 / 1
      (rows of 64 lanes) against its tiled twin adt_kldist_full_groups at d 64 and against eight adt_kldist_full_lanes calls, the only
      correct padded route without it; the three alternate inside every round (device events, 3 warm-up rounds, 5 timed), and the item
      packs are timed alone.
  (p) the cost of padding: one warm-up step and one batched candidate evaluation pass (8 candidates) of each supernet at 50 / 1 against
      64 / 1 -- the same d_pad, so the difference is the lane-aware row kernels, the copy of the trained ranges and the split
      projection + activation passes.  One layer, L 50, batch 128, evaluation batch 256, bf16; host clock around work that ends in a
      synchronise, 3 warm-up steps and 10 timed, the two widths alternating in 5 rounds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adt_amd import ops  # noqa: E402
from adt_amd.supersearch import cand_to_block, get_shared  # noqa: E402
from tools.bench_fullrank import timed_alternating  # noqa: E402

REC = [0, 0.0001, 0.0005, 0.001, 0.005, 0.01]
IND = [0, 0.0001, 0.0005, 0.001, 0.0015, 0.002]


class Args:
    pass


def kernel_lines(dev):
    V, E, P = 12103, 512, 8
    lanes, d = (1, 50, 64), 50
    g = torch.Generator(device="cpu").manual_seed(V + P)
    pad = lambda x: torch.nn.functional.pad(x, (0, 64 - x.shape[1]))
    Em, Ec = 0.3 * torch.randn(V, 64, generator=g), 0.3 * torch.randn(V, 64, generator=g)
    sm, sc = 0.3 * torch.randn(P * E, 64, generator=g), torch.exp(0.2 * torch.randn(P * E, 64, generator=g))
    tEm, tEc, tsm, tsc = (x.to(dev) for x in (Em, Ec, sm, sc))                                  # the tiled twin: all 64 columns live
    pEm, pEc, psm, psc = (pad(x[:, :d]).contiguous().to(dev) for x in (Em, Ec, sm, sc))         # 50 live lanes, +0.0 pads
    timg, limg = ops.kldist_pack(tEm, tEc), ops.kldist_pack_lanes(pEm, pEc, lanes)

    def tiled():
        return ops.kldist_full_groups(tsm, tsc, timg[0], timg[1], E, V)

    def lane_groups():
        return ops.kldist_full_groups_lanes(psm, psc, limg[0], limg[1], E, V, lanes)

    def lane_loop():
        return [ops.kldist_full_lanes(psm[k * E:(k + 1) * E], psc[k * E:(k + 1) * E], pEm, pEc, V, lanes) for k in range(P)]

    a, b = torch.cat(lane_loop()), lane_groups()
    agree = float((a - b).abs().max() / a.abs().max())
    del a, b
    rec = {"part": "kernel", "V": V, "E": E, "candidates": P, "lanes": list(lanes), "groups_lanes_vs_loop_max_diff_over_max": agree}
    rec.update(timed_alternating({"groups_tiled_d64": tiled, "groups_lanes_50": lane_groups, "loop_full_lanes_50": lane_loop,
                                  "pack_tiled_d64": lambda: ops.kldist_pack(tEm, tEc), "pack_lanes_50": lambda: ops.kldist_pack_lanes(pEm, pEc, lanes)}))
    rec["lanes_over_tiled"] = rec["groups_lanes_50"]["median_ms"] / rec["groups_tiled_d64"]["median_ms"]
    rec["loop_over_lanes"] = rec["loop_full_lanes_50"]["median_ms"] / rec["groups_lanes_50"]["median_ms"]
    spread = max(rec[k]["max_ms"] - rec[k]["min_ms"] for k in ("groups_tiled_d64", "groups_lanes_50"))
    rec["accepted"] = bool(rec["groups_lanes_50"]["median_ms"] <= rec["groups_tiled_d64"]["median_ms"] + spread)
    return [rec]


def _timed(fn, warm, n):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def _sasrec(d, r, B, EB, L, V):
    from adt_amd.sasrec.supersasrec import SuperSASRecModel, SuperTrainer
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = "cuda:0", 1, L, 1, d, 0.5, "bf16"
    m = SuperSASRecModel(1, V, REC, IND, a, allow_lanes=True)
    tr = SuperTrainer(m, lr=1e-3, weight_decay=1e-3)
    seq = r.randint(1, V + 1, size=(B, L)).astype(np.int32)
    seq[:, :5] = 0
    dec, pos, neg = np.roll(seq, 1, 1), np.where(seq > 0, r.randint(1, V + 1, size=(B, L)), 0), np.where(seq > 0, r.randint(1, V + 1, size=(B, L)), 0)
    eseq, items = np.tile(seq, (EB // B, 1)), r.randint(1, V + 1, size=(EB, 101)).astype(np.int32)
    return m, tr, lambda: tr.step(seq, dec, pos, neg), lambda sh: m.predict_rank_candidates(eseq, items, sh)


def _bert(d, r, B, EB, L, V):
    from adt_amd.bert4rec.superbert import SuperBertModel, SuperBertTrainer
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", L, 1, 1, d, 4 * d
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = 0.2, 0.2, 2, "bf16"
    m = SuperBertModel(1, V, REC, IND, a, allow_lanes=True)
    tr = SuperBertTrainer(m)
    items = r.randint(1, V + 1, size=(B, L))
    mask = r.rand(B, L) < 0.2
    mask[:, -1] = True
    src, lab = np.where(mask, V + 1, items), np.where(mask, items, 0)
    eseq, cand = np.tile(src, (EB // B, 1)), r.randint(1, V + 1, size=(EB, 101)).astype(np.int32)
    return m, tr, lambda: tr.step(src, items, lab), lambda sh: m.predict_rank_candidates(eseq, cand, sh)


def _stosa(metric):
    def make(d, r, B, EB, L, V):
        from adt_amd.stosa.supernet import DisenDistSASupernet, SuperStosaTrainer
        a = Args()
        a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = "cuda:0", V + 2, L, d, 1, 1, 4
        a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.5, 0.5, 0.005, "bf16", metric
        m = DisenDistSASupernet(a, REC, REC, allow_kl=True, allow_lanes=True)
        tr = SuperStosaTrainer(m)
        inp = r.randint(1, V + 1, size=(B, L))
        inp[:, :5] = 0
        pos, neg = np.where(inp > 0, r.randint(1, V + 1, size=(B, L)), 0), np.where(inp > 0, r.randint(1, V + 1, size=(B, L)), 0)
        dec = np.concatenate([np.zeros((B, 1), int), inp[:, :-1]], 1)
        einp = np.tile(inp, (EB // B, 1))
        return m, tr, lambda: tr.step(inp, dec, pos, neg), lambda sh: m.predict_full_candidates(einp, sh)
    return make


def padding_lines():
    B, EB, L, V, ncand = 128, 256, 50, 12101, 8
    lines = []
    for name, make, rc, ic in (("sasrec", _sasrec, REC, IND), ("bert4rec", _bert, REC, IND), ("stosa", _stosa("wasserstein"), REC, REC),
                               ("stosa_kl", _stosa("kl"), REC, REC)):
        r = np.random.RandomState(3)
        cands = [[float(x) for x in r.rand(2)] for _ in range(ncand)]
        shared = [get_shared(rc, ic, cand_to_block(rc, ic, c)[0]) for c in cands]
        built = {}
        for d in (50, 64):
            torch.manual_seed(1)
            m, tr, step, evaluate = make(d, np.random.RandomState(5), B, EB, L, V)
            tr.set_choice(cands[0])
            built[d] = (m, step, lambda ev=evaluate: ev(shared))
        ms = {(d, k): [] for d in built for k in ("step", "eval")}
        for _ in range(5):
            for d, (m, step, ev) in built.items():
                ms[(d, "step")].append(_timed(step, 3, 10))
                ms[(d, "eval")].append(_timed(ev, 1, 3))
        rec = {"part": "padding", "supernet": name, "batch": B, "eval_batch": EB, "maxlen": L, "items": V, "candidates": ncand}
        for (d, k), v in ms.items():
            rec["%s_ms_%d" % (k, d)] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
        rec["step_50_over_64"] = rec["step_ms_50"]["median"] / rec["step_ms_64"]["median"]
        rec["eval_50_over_64"] = rec["eval_ms_50"]["median"] / rec["eval_ms_64"]["median"]
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        del built
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_super_lanes.py measures on the GPU: no device found")
    lines = []
    if "k" in a.parts:
        lines += kernel_lines(torch.device("cuda:0"))
        print(json.dumps(lines[-1]), flush=True)
    if "p" in a.parts:
        lines += padding_lines()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
