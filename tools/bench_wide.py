#!/usr/bin/env python3
"""Step-time measurement of the BERT4Rec-ADT and STOSA-ADT training steps (BASELINE.json configs[2] and configs[4] shapes,
one GPU, synthetic ids, HIP graph).  Not the driver's bench (bench.py measures configs[1]); results go to profiles/.

    python tools/bench_wide.py bert  [--steps 20] [--batch 256] [--maxlen 200] [--bert_template ml-20m|beauty] [--fused_head]
    python tools/bench_wide.py stosa [--steps 20] [--metric wasserstein|kl] [--stosa_maxlen 100] [--stosa_heads 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class Args:
    pass


def bert_batch(r, B, L, V, mask_prob):
    src = np.zeros((B, L), np.int32)
    dec = np.zeros((B, L), np.int32)
    lab = np.zeros((B, L), np.int32)
    lens = np.clip(np.exp(r.normal(4.6, 0.95, size=B)), 20, L).astype(int)
    for b in range(B):
        n = int(lens[b])
        items = r.randint(1, V + 1, size=n)
        m = r.rand(n) < mask_prob
        m[-1] = True
        dec[b, L - n:] = items
        src[b, L - n:] = np.where(m, V + 1, items)
        lab[b, L - n:] = np.where(m, items, 0)
    return src, dec, lab


def run_bert(args):
    import torch
    from adt_amd.bert4rec.model import BertModel
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    a = Args()
    L = args.maxlen
    beauty = args.bert_template == "beauty"       # templates/beauty.json: d 64, H 2, mask_prob 0.6, 12,101 items; else the ml-1m / ml-20m width
    d, H, pa, mask_prob, mcap = (64, 2, 0.2, 0.6, 1.0) if beauty else (256, 4, 0.5, 0.2, args.mcap)
    d, H = (d if args.hidden_units is None else args.hidden_units), (H if args.num_heads is None else args.num_heads)      # e.g. 50 / 1: a padded width
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", L, H, 2, d, 1024
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision, a.fused_head = 0.5, pa, 2, "bf16", args.fused_head
    V = 12101 if beauty and args.items == 26744 else args.items
    torch.manual_seed(23)
    m = BertModel(1, V, a)
    tr = FusedBertTrainer(m, [0.1, 0.05], [0.1, 0.05], weight_decay=1e-4, use_graph=not args.no_graph, seed=23, mcap_frac=mcap)
    r = np.random.RandomState(1)
    staged = [tr.stage(*bert_batch(r, args.batch, L, V, mask_prob)) for _ in range(4)]
    for i in range(args.warmup):
        tr.step_staged(staged[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        tr.step_staged(staged[i % 4])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    M = float(np.mean([s["M_host"] for s in staged]))
    flops_logits = 3 * 2 * M * d * (V + 100)
    what = "Beauty template" if beauty else "ml-20m shape"
    print(json.dumps({"workload": "BERT4Rec-ADT %s: d=%d H=%d inner=1024 L=%d 2+2 layers V+100=%d, batch %d, dropout 0.5, full train step%s"
                                  % (what, d, H, L, V + 100, args.batch, ", fused head" if m.fused_head else ""),
                      "ms_per_step": round(dt / args.steps * 1e3, 3), "sequences_per_s": round(args.batch * args.steps / dt, 1), "masked_rows": M, "lanes": list(m.lanes) if m.lanes else None,
                      "drn": ("fused" if m.drn_fused else "two-pass") if m.lanes else None,
                      "logits_gemm_tflops_per_step": round(flops_logits / 1e12, 3), "loss": round(float(tr.loss()), 4), "dtype": "bf16",
                      "max_memory_allocated_MB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}))


def run_stosa(args):
    import torch
    from adt_amd.stosa.models import DisenDistSAModel
    from adt_amd.stosa.trainer import FusedStosaTrainer
    a = Args()
    d, H = args.hidden_units or 64, args.num_heads or args.stosa_heads          # e.g. 50 / 1: a padded width
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = "cuda:0", 12103, args.stosa_maxlen, d, H, 1, 22364
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.3, 0.3, 0.005, "bf16", args.metric
    torch.manual_seed(42)
    m = DisenDistSAModel(a, allow_kl_lanes=True, allow_wide_heads=True)
    tr = FusedStosaTrainer(m, [0.1], [0.1], use_graph=not args.no_graph, seed=42)
    r = np.random.RandomState(2)
    B, L, V = args.batch, a.maxlen, a.item_size

    def batch():
        inp = np.zeros((B, L), np.int32)
        pos = np.zeros((B, L), np.int32)
        neg = np.zeros((B, L), np.int32)
        dec = np.zeros((B, L), np.int32)
        lens = np.clip(r.geometric(0.12, size=B) + 3, 4, L)
        for b in range(B):
            n = int(lens[b])
            it = r.randint(1, V, size=n + 1)
            inp[b, L - n:], pos[b, L - n:], neg[b, L - n:] = it[:-1], it[1:], r.randint(1, V, size=n)
            dec[b, 1:] = inp[b, :-1]
        return inp, dec, pos, neg
    staged = [tr.stage(*batch()) for _ in range(4)]
    for i in range(args.warmup):
        tr.step_staged(staged[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        tr.step_staged(staged[i % 4])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kl = args.metric == "kl"
    print(json.dumps({"workload": "STOSA-ADT Beauty shape: d=%d H=%d L=%d 1+1 layers item_size=12103, batch %d, dropout 0.3, full train step%s"
                      % (d, a.num_heads, L, B, ", distance_metric kl" if kl else ""), "lanes": list(m.lanes) if getattr(m, "lanes", None) else None,
                      "ms_per_step": round(dt / args.steps * 1e3, 3), "sequences_per_s": round(B * args.steps / dt, 1), "loss": round(float(tr.loss()), 4),
                      "steps": args.steps, "warmup": args.warmup,
                      "dtype": "bf16 MFMA operands (dense layers and %s attention), fp32 accumulation, statistics and losses" % ("KL" if kl else "Wasserstein")}))


def run_sasrec256(args):
    """SASRec-ADT at the shipped ml-1m template width (sasrec/templates/ml-1m.json: hidden_units 256, 2 heads, maxlen 200)."""
    import torch
    import bench
    from adt_amd.sasrec.model_wide import SASRecADTWide, WideSasrecTrainer
    a = Args()
    d, H, L, nl = args.hidden_units or 256, args.num_heads or 2, args.maxlen, args.num_layers        # defaults: the template shape
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = "cuda:0", H, L, nl, d, 0.5, "bf16"
    torch.manual_seed(23)
    m = SASRecADTWide(6040, 3416, a)
    for _, p in m.named_parameters():
        try:
            torch.nn.init.xavier_normal_(p.data)
        except Exception:
            pass
    lam1, lam2 = ([lam[i % len(lam)] for i in range(nl)] for lam in (bench.CFG["lambdas1"], bench.CFG["lambdas2"]))   # one pair per layer
    tr = WideSasrecTrainer(m, lam1, lam2, weight_decay=1e-3, use_graph=not args.no_graph, seed=23)
    batches = bench.synth_batches(4, args.batch, L, 3416, seed=100)
    for i in range(args.warmup):
        tr.step(*batches[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        tr.step(*batches[i % 4])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    what = "ml-1m TEMPLATE width: d=256 H=2 (head size 128) L=200 2+2 layers" if (d, H, L, nl) == (256, 2, 200, 2) else \
        "wide path: d=%d H=%d (head size %d, computed as d_pad=%d) L=%d %d+%d layers" % (d, H, d // H, m.dp, L, nl, nl)
    print(json.dumps({"workload": "SASRec-ADT %s V=3416, batch %d, dropout 0.5, full train step (H2D of ids included)" % (what, args.batch),
                      "ms_per_step": round(dt / args.steps * 1e3, 3), "sequences_per_s": round(args.batch * args.steps / dt, 1), "loss": round(float(tr.loss()), 4),
                      "dtype": "bf16"}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=["bert", "stosa", "sasrec256"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--items", type=int, default=26744)
    ap.add_argument("--mcap", type=float, default=0.3)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--metric", default="wasserstein", choices=["wasserstein", "kl"], help="stosa: distance_metric")
    ap.add_argument("--stosa_maxlen", type=int, default=100, help="stosa: maxlen (the Beauty template's 100; up to 1024)")
    ap.add_argument("--stosa_heads", type=int, default=4, help="stosa: heads of the 64-wide model (4: Beauty / Tools, 1: Home / Office / Toys)")
    ap.add_argument("--hidden_units", type=int, default=None, help="bert, sasrec256: width (default: the template's; sasrec256: 256)")
    ap.add_argument("--num_heads", type=int, default=None, help="bert, sasrec256: heads (default: the template's; sasrec256: 2)")
    ap.add_argument("--maxlen", type=int, default=200, help="bert, sasrec256: maxlen (up to 1024)")
    ap.add_argument("--bert_template", default="ml-20m", choices=["ml-20m", "beauty"], help="bert: the d 256 / H 4 shape or templates/beauty.json's")
    ap.add_argument("--fused_head", action="store_true", help="bert at d 64: the fused logits + cross-entropy head (adt_lce_fwd_bwd)")
    ap.add_argument("--num_layers", type=int, default=2)
    args = ap.parse_args()
    {"bert": run_bert, "stosa": run_stosa, "sasrec256": run_sasrec256}[args.which](args)
