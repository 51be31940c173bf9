#!/usr/bin/env python3
"""Stand-alone timing of the masked / general attention kernels (adt_attn_masked_fwd/bwd) at the BERT ml-20m and SASRec d=256 shapes,
with and without dropout (the backward regenerates the dropout hash in both of its passes); head size 256 (d = 256, one head: the
reference's search default, adt_attn_long.cuh at 256 rows) next to head size 128 at the same L, with achieved TFLOP/s (causal: half the
score / PV work of the full L x L products is counted).  `python tools/bench_attn_gen.py long [out.jsonl]` times the entry points for
L up to 1024 (adt_attn_long_fwd/bwd) instead, next to the older ones at the longest L those take (main_long)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from adt_amd import ops  # noqa: E402
from tools.bench_dense import timeit  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    seed = torch.tensor([7], device=dev, dtype=torch.int32)
    shapes = [("bert ml-20m", 256, 4, 200, 64, False), ("sasrec d=256", 256, 2, 200, 128, True)]
    for L in (50, 200):
        shapes += [("hd128 L=%d" % L, 256, 2, L, 128, True), ("hd256 L=%d" % L, 256, 1, L, 256, True)]
    for name, B, H, L, hd, causal in shapes:
        d = H * hd
        T = B * L
        qkv = torch.randn(T, 3 * d, device=dev)
        Q, K, V = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        ids = torch.randint(1, 100, (T,), device=dev, dtype=torch.int32)
        dO = torch.randn(T, d, device=dev)
        for p in (0.0, 0.2):
            kid = None if causal else ids
            O, LSE = ops.attn_masked_fwd(ops.PREC_BF16, Q, K, V, B, H, L, causal, kid, -1e9, p, seed, 3, 0)
            t_f = timeit(lambda: ops.attn_masked_fwd(ops.PREC_BF16, Q, K, V, B, H, L, causal, kid, -1e9, p, seed, 3, 0))
            t_b = timeit(lambda: ops.attn_masked_bwd(ops.PREC_BF16, Q, K, V, O, LSE, dO, B, H, L, causal, kid, -1e9, p, seed, 3, 0))
            flop = 4.0 * B * H * L * L * hd * (0.5 if causal else 1.0)         # QK^T + PV; the backward does 2.5x that (S, dP, dQ, dK, dV)
            print("%-13s p=%.1f  fwd %7.1f us %6.1f TFLOP/s  bwd %7.1f us %6.1f TFLOP/s" % (name, p, t_f, flop / t_f * 1e-6, t_b, 2.5 * flop / t_b * 1e-6),
                  flush=True)


def main_long(jsonl=None):
    """python tools/bench_attn_gen.py long [out.jsonl]: the entry points for 1 <= L <= 1024 (adt_attn_long_fwd / _bwd; adt_attn_long.cuh) at B 64,
    causal with fill -inf (the SASRec call), bf16, p 0 / 0.2: (hd 32, H 2), (hd 128, H 2), (hd 256, H 1) at L 256, 512, 1024.  At the longest
    L the older entry points take (200 at hd 32, 256 above) both families are timed on the same tensors, alternating, three rounds each, the
    median reported: what the streamed kernels (and the delta pass every workgroup of a (b, h) repeats) cost at the boundary."""
    import json
    dev = torch.device("cuda:0")
    seed = torch.tensor([7], device=dev, dtype=torch.int32)
    B, fill = 64, float("-inf")
    out = open(jsonl, "w") if jsonl else None

    def pair(fwd, bwd, Q, K, V, dO, H, L, p):
        O, LSE = fwd(ops.PREC_BF16, Q, K, V, B, H, L, True, None, fill, p, seed, 3, 0)
        return (lambda: fwd(ops.PREC_BF16, Q, K, V, B, H, L, True, None, fill, p, seed, 3, 0),
                lambda: bwd(ops.PREC_BF16, Q, K, V, O, LSE, dO, B, H, L, True, None, fill, p, seed, 3, 0))

    for hd, H in ((32, 2), (128, 2), (256, 1)):
        d = H * hd
        lb = 200 if ops.attn_masked_max_len(hd) < 256 else 256      # the template length where 256 rows are not taken
        for L in sorted({lb, 256, 512, 1024}):
            qkv = torch.randn(B * L, 3 * d, device=dev)
            Q, K, V = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
            dO = torch.randn(B * L, d, device=dev)
            for p in (0.0, 0.2):
                fams = [("long", pair(ops.attn_long_fwd, ops.attn_long_bwd, Q, K, V, dO, H, L, p))]
                if L == lb:
                    fams.append(("masked", pair(ops.attn_masked_fwd, ops.attn_masked_bwd, Q, K, V, dO, H, L, p)))
                times = {nm: ([], []) for nm, _ in fams}
                for _ in range(3 if len(fams) > 1 else 1):
                    for nm, (f, b) in fams:
                        times[nm][0].append(timeit(f))
                        times[nm][1].append(timeit(b))
                flop = 4.0 * B * H * L * L * hd * 0.5
                for nm, _ in fams:
                    t_f, t_b = float(np.median(times[nm][0])), float(np.median(times[nm][1]))
                    rec = dict(kernel=nm, hd=hd, H=H, B=B, L=L, p=p, fwd_us=round(t_f, 1), fwd_tflops=round(flop / t_f * 1e-6, 1), bwd_us=round(t_b, 1),
                               bwd_tflops=round(2.5 * flop / t_b * 1e-6, 1))
                    print("%-6s hd%-3d H%d L=%-4d p=%.1f  fwd %8.1f us %6.1f TFLOP/s  bwd %8.1f us %6.1f TFLOP/s" % (nm, hd, H, L, p, t_f, rec["fwd_tflops"], t_b,
                                                                                                             rec["bwd_tflops"]), flush=True)
                    if out:
                        out.write(json.dumps(rec) + "\n")
                        out.flush()


if __name__ == "__main__":
    if sys.argv[1:2] == ["long"]:
        main_long(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main()
