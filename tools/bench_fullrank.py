"""Full-catalogue ranking: the fused adt_full_rank call against the two-pass form available before it -- predict(full=True)'s logit
kernel (adt_score_rank without candidates: a (B, V + 1) fp32 matrix in HBM), negated, then adt_topk_masked with the same seen CSR.

  python tools/bench_fullrank.py [--out profiles/r07_fullrank_bench.jsonl]

HIP-event timing: 3 warm-up calls, then 5 timed repetitions per form; the median and the spread (min .. max) are reported, one JSON
line per shape (ml-1m: V 3,416, d 64; ml-20m: V 26,744, d 256; B 512, K 10, 100 seen items per user; the fused call also with 1,000 and with none)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adt_amd import ops  # noqa: E402

SHAPES = (("ml-1m", 3416, 64), ("ml-20m", 26744, 256))
B, K, SEEN, WARMUP, REPS = 512, 10, 100, 3, 5


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r07_fullrank_bench.jsonl"))
    args = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for name, V, d in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(V)
        F = torch.randn(B, d, generator=g).to(dev)
        E = torch.randn(V + 1, d, generator=g).to(dev)
        r = np.random.RandomState(V)
        target = torch.from_numpy(r.randint(1, V + 1, B).astype(np.int32)).to(dev)
        indptr = torch.arange(0, (B + 1) * SEEN, SEEN, dtype=torch.int32, device=dev)
        indices = torch.from_numpy(r.randint(1, V + 1, B * SEEN).astype(np.int32)).to(dev)

        def fused():
            return ops.full_rank(F, d, E, V, target, None, indptr, indices, K)

        def two_pass():
            logits, _ = ops.score_rank(F, d, E, None, B, V + 1, want_rank=False)
            return ops.topk_masked(-logits, K, indptr, indices, want_val=True)

        # the two forms agree on what they both compute: the same K items per user (item 0 can enter the two-pass list: it has no
        # notion of the padding row), scores equal to fp32 rounding
        ti = fused()[2].cpu().numpy()
        tp = two_pass()[0].cpu().numpy()
        same = float(np.mean([len(set(ti[b]) & set(tp[b])) for b in range(B)])) / K
        table, logit = (V + 1) * d * 4, B * (V + 1) * 4
        rec = {"shape": name, "V": V, "d": d, "B": B, "K": K, "seen_per_user": SEEN, "fused": timed(fused), "two_pass": timed(two_pass),
               "topk_overlap": same,
               "hbm_bytes_fused": table + B * d * 4,                              # the table and the features, once
               "hbm_bytes_two_pass": table + B * d * 4 + 4 * logit}               # + logits written, read and re-written negated, read by the selection
        # the seen lists are re-read once per split and 4,096-item block: the same call with ten times longer histories
        indptr_l = torch.arange(0, (B + 1) * SEEN * 10, SEEN * 10, dtype=torch.int32, device=dev)
        indices_l = torch.from_numpy(r.randint(1, V + 1, B * SEEN * 10).astype(np.int32)).to(dev)
        rec["fused_seen_x10"] = timed(lambda: ops.full_rank(F, d, E, V, target, None, indptr_l, indices_l, K))
        rec["fused_no_seen"] = timed(lambda: ops.full_rank(F, d, E, V, target, None, None, None, K))
        rec["fused_over_two_pass"] = rec["fused"]["median_ms"] / rec["two_pass"]["median_ms"]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
