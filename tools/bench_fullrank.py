"""Full-catalogue ranking: the fused adt_full_rank call against the two-pass form available before it -- predict(full=True)'s logit
kernel (adt_score_rank without candidates: a (B, V + 1) fp32 matrix in HBM), negated, then adt_topk_masked with the same seen CSR.

  python tools/bench_fullrank.py [--out profiles/r07_fullrank_bench.jsonl]

HIP-event timing: 3 warm-up calls, then 5 timed repetitions per form; the median and the spread (min .. max) are reported, one JSON
line per shape (ml-1m: V 3,416, d 64; ml-20m: V 26,744, d 256; B 512, K 10, 100 seen items per user; the fused call also with 1,000 and with none).

  python tools/bench_fullrank.py --stosa [--out profiles/r08_stosa_fullrank.jsonl]

STOSA-ADT (Wasserstein) at the Beauty shape: item_size 12,103, d 64 (image width 128), B 512 (stosa/main.py's eval_batch_size; the
template does not override it), K 40, 100 seen items per user, item 0 competing (first_id = 0, as full_sort(fused=True) runs it).
Same timing scheme; one JSON line for one model (P = 1) and one for P = 8 stacked candidates: (a) two_pass = adt_wdist_full +
adt_topk_masked, (b) fused = the user-state pack + adt_full_rank_from with a pre-packed item image, (c) pack = the item pack alone.

  python tools/bench_fullrank.py --stosa --metric kl [--out profiles/r18_stosa_kl_full.jsonl]

STOSA-ADT (KL) full-sort distances at the same shape, E = B = 512, one line for P = 1 and one for P = 8 stacked candidates: (a) loop =
P adt_kldist_full calls, one per candidate (the only correct route without the group rule), (b) groups = one adt_kldist_full_groups
call on a pre-packed image, (c) pack = adt_kldist_pack alone.  Inputs have trained magnitudes (tables 0.3 N(0, 1), covariances
exp(0.2 N(0, 1))).  The forms ALTERNATE inside every repetition (loop, groups, pack, loop, ...), so a drift of the clocks falls on
all of them alike; 3 warm-up rounds, 5 timed ones.

  python tools/bench_fullrank.py --stosa --metric kl --rowwise [--out profiles/r20_stosa_kl_rowwise.jsonl]

STOSA-ADT (KL) ranked by the ROW-WISE divergence at the same shape (K 40, 100 seen items per user, first_id = 0), P = 1 and 8, the same
inputs and the same alternating scheme: (a) rowwise = the user-state pack (adt_klrow_pack, items = 0) + adt_full_rank_from on a
pre-packed image, (b) pack = the item pack alone (items = 1), (c) matrix = adt_kldist_full_groups + adt_topk_masked, for context only:
it ranks by kl_predict_full's batch-dependent score, a different function.

  python tools/bench_fullrank.py --groups [--out profiles/r31_full_eval_device.jsonl]

The group-aware call at the two dot-product shapes, R = 512 users, P = 8 and P = 32 stacked candidates, K 0 (the
search reads ranks only): (a) groups = ONE adt_full_rank_groups call on the P * R rows and the resident int64 CSR of the R users,
(b) loop = P adt_full_rank calls, one per candidate, on the int32 CSR.  The same alternating scheme; the two forms' ranks are compared
bit for bit first.  One JSON line per (shape, P)."""
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


def timed_alternating(fns):
    """{name: stats} of the callables of `fns`, one call of each per round, in the given order: WARMUP rounds, then REPS timed ones."""
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ms.items()}


def stosa_kl_lines(dev):
    V, d, E = 12103, 64, B
    lines = []
    for P in (1, 8):
        rows = P * E
        g = torch.Generator(device="cpu").manual_seed(V + P)
        Em, Ec = (0.3 * torch.randn(V, d, generator=g)).to(dev), (0.3 * torch.randn(V, d, generator=g)).to(dev)
        sm, sc = (0.3 * torch.randn(rows, d, generator=g)).to(dev), torch.exp(0.2 * torch.randn(rows, d, generator=g)).to(dev)
        image = ops.kldist_pack(Em, Ec)

        def loop():
            return [ops.kldist_full(sm[k * E:(k + 1) * E], sc[k * E:(k + 1) * E], Em, Ec, V) for k in range(P)]

        def groups():
            return ops.kldist_full_groups(sm, sc, image[0], image[1], E, V)

        a, b = torch.cat(loop()), groups()
        agree = float((a - b).abs().max() / a.abs().max())
        del a, b
        rec = {"shape": "stosa-beauty", "metric": "kl", "V": V, "d": d, "E": E, "candidates": P, "max_diff_over_max": agree}
        rec.update(timed_alternating({"loop": loop, "groups": groups, "pack": lambda: ops.kldist_pack(Em, Ec)}))
        rec["hbm_bytes_dist"] = rows * V * 4
        rec["groups_over_loop"] = rec["groups"]["median_ms"] / rec["loop"]["median_ms"]
        spread = max(rec[k]["max_ms"] - rec[k]["min_ms"] for k in ("loop", "groups"))
        rec["accepted"] = bool(rec["groups"]["median_ms"] <= rec["loop"]["median_ms"] + spread)      # not above the loop by more than the larger spread
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    return lines


def stosa_kl_rowwise_lines(dev):
    V, d, E, K = 12103, 64, B, 40
    lines = []
    for P in (1, 8):
        rows = P * E
        g = torch.Generator(device="cpu").manual_seed(V + P)
        Em, Ec = (0.3 * torch.randn(V, d, generator=g)).to(dev), (0.3 * torch.randn(V, d, generator=g)).to(dev)
        sm, sc = (0.3 * torch.randn(rows, d, generator=g)).to(dev), torch.exp(0.2 * torch.randn(rows, d, generator=g)).to(dev)
        r = np.random.RandomState(V + P)
        indptr = torch.arange(0, (rows + 1) * SEEN, SEEN, dtype=torch.int32, device=dev)
        indices = torch.from_numpy(r.randint(0, V, rows * SEEN).astype(np.int32)).to(dev)
        image = ops.klrow_pack(Em, Ec, True)
        kl_image = ops.kldist_pack(Em, Ec)

        def rowwise():
            A, nu = ops.klrow_pack(sm, sc, False)
            return ops.full_rank(A, 2 * d, image[0], V - 1, None, image[1], indptr, indices, K, first_id=0)

        def matrix():      # for context only: kl_predict_full's matrix and its selection -- a DIFFERENT, batch-dependent score
            return ops.topk_masked(ops.kldist_full_groups(sm, sc, kl_image[0], kl_image[1], E, V), K, indptr, indices, want_val=True)

        rec = {"shape": "stosa-beauty", "metric": "kl", "rowwise": True, "V": V, "d": d, "B": B, "candidates": P, "K": K, "seen_per_user": SEEN,
               "first_id": 0}
        rec.update(timed_alternating({"rowwise": rowwise, "pack": lambda: ops.klrow_pack(Em, Ec, True), "matrix": matrix}))
        rec["hbm_bytes_rowwise"] = V * (2 * d + 1) * 4 + 3 * rows * 2 * d * 4      # the image and bias; the states read, their image written and read
        rec["hbm_bytes_pack"] = 2 * V * d * 4 + V * (2 * d + 1) * 4
        rec["hbm_bytes_matrix"] = V * (2 * d + 1) * 4 + rows * 2 * d * 4 + 2 * rows * V * 4
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    return lines


def groups_lines(dev):
    R, lines = B, []
    for name, V, d in SHAPES:
        for P in (8, 32):
            g = torch.Generator(device="cpu").manual_seed(V + P)
            F = torch.randn(P * R, d, generator=g).to(dev)
            E = torch.randn(V + 1, d, generator=g).to(dev)
            r = np.random.RandomState(V)
            target = torch.from_numpy(r.randint(1, V + 1, R).astype(np.int32)).to(dev)
            indptr = torch.arange(0, (R + 1) * SEEN, SEEN, dtype=torch.int32, device=dev)
            indices = torch.from_numpy(r.randint(1, V + 1, R * SEEN).astype(np.int32)).to(dev)
            off = indptr.long()

            def groups():
                return ops.full_rank_groups(F, d, E, V, target, off, indices, P * R, R)

            def loop():
                return [ops.full_rank(F[p * R:(p + 1) * R], d, E, V, target, None, indptr, indices, 0) for p in range(P)]

            a, b = groups(), loop()
            same = all(torch.equal(a[i], torch.cat([x[i] for x in b])) for i in (0, 1))
            del a, b
            rec = {"shape": name, "V": V, "d": d, "R": R, "candidates": P, "K": 0, "seen_per_user": SEEN, "bit_equal": bool(same)}
            rec.update(timed_alternating({"loop": loop, "groups": groups}))
            rec["groups_over_loop"] = rec["groups"]["median_ms"] / rec["loop"]["median_ms"]
            spread = max(rec[k]["max_ms"] - rec[k]["min_ms"] for k in ("loop", "groups"))
            rec["accepted"] = bool(rec["groups"]["median_ms"] <= rec["loop"]["median_ms"] + spread)      # not above the loop by more than the larger spread
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    return lines


def stosa_lines(dev):
    V, d, K = 12103, 64, 40
    lines = []
    for P in (1, 8):
        rows = P * B
        g = torch.Generator(device="cpu").manual_seed(V + P)
        Em, Ec = (0.5 * torch.randn(V, d, generator=g)).to(dev), torch.randn(V, d, generator=g).to(dev)
        sm, sc = torch.randn(rows, d, generator=g).to(dev), (0.05 + 2.0 * torch.rand(rows, d, generator=g)).to(dev)
        r = np.random.RandomState(V + P)
        indptr = torch.arange(0, (rows + 1) * SEEN, SEEN, dtype=torch.int32, device=dev)
        indices = torch.from_numpy(r.randint(0, V, rows * SEEN).astype(np.int32)).to(dev)
        image = ops.wdist_pack(Em, Ec, True, -0.5)

        def fused():
            A, na = ops.wdist_pack(sm, sc, False, 1.0)
            return ops.full_rank(A, 2 * d, image[0], V - 1, None, image[1], indptr, indices, K, first_id=0)

        def two_pass():
            return ops.topk_masked(ops.wdist_full(sm, sc, Em, Ec, V), K, indptr, indices, want_val=True)

        ti = fused()[2].cpu().numpy()
        tp = two_pass()[0].cpu().numpy()
        same = float(np.mean([len(set(ti[b]) & set(tp[b])) for b in range(rows)])) / K
        tables, dist = 2 * V * d * 4, rows * V * 4
        rec = {"shape": "stosa-beauty", "V": V, "d": d, "B": B, "candidates": P, "K": K, "seen_per_user": SEEN, "first_id": 0,
               "two_pass": timed(two_pass), "fused": timed(fused), "pack": timed(lambda: ops.wdist_pack(Em, Ec, True, -0.5)),
               "topk_overlap": same,
               "hbm_bytes_fused": V * (2 * d + 1) * 4 + 3 * rows * 2 * d * 4,     # the image and bias; the states read, their image written and read
               "hbm_bytes_pack": tables + V * (2 * d + 1) * 4,
               "hbm_bytes_two_pass": tables + rows * 2 * d * 4 + 2 * dist}      # + the distance matrix written, then read by the selection
        rec["fused_over_two_pass"] = rec["fused"]["median_ms"] / rec["two_pass"]["median_ms"]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stosa", action="store_true", help="the STOSA-ADT (Wasserstein) Beauty shape instead of the dot-product shapes")
    ap.add_argument("--metric", default="wasserstein", choices=["wasserstein", "kl"], help="with --stosa: kl = the grouped KL full sort against P adt_kldist_full calls")
    ap.add_argument("--rowwise", action="store_true", help="with --stosa --metric kl: the ranking by the row-wise KL divergence (adt_klrow_pack + adt_full_rank_from)")
    ap.add_argument("--groups", action="store_true", help="one adt_full_rank_groups call against P adt_full_rank calls at the dot-product shapes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.groups and (args.stosa or args.metric == "kl" or args.rowwise):
        ap.error("--groups runs alone")
    kl = args.stosa and args.metric == "kl"
    if args.metric == "kl" and not args.stosa:
        ap.error("--metric kl goes with --stosa")
    if args.rowwise and not kl:
        ap.error("--rowwise goes with --stosa --metric kl")
    if args.out is None:
        args.out = os.path.join("profiles", "r20_stosa_kl_rowwise.jsonl" if args.rowwise else "r18_stosa_kl_full.jsonl" if kl else
                                "r08_stosa_fullrank.jsonl" if args.stosa else "r31_full_eval_device.jsonl" if args.groups else "r07_fullrank_bench.jsonl")
    dev = "cuda:0"
    lines = stosa_kl_rowwise_lines(dev) if args.rowwise else stosa_kl_lines(dev) if kl else stosa_lines(dev) if args.stosa else \
        groups_lines(dev) if args.groups else []
    for name, V, d in (() if args.stosa or args.groups else SHAPES):
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
