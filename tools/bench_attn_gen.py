#!/usr/bin/env python3
"""Stand-alone timing of the masked / general attention kernels (adt_attn_masked_fwd/bwd) at the BERT ml-20m and SASRec d=256 shapes,
with and without dropout (the backward regenerates the dropout hash in both of its passes); head size 256 (d = 256, one head: the
reference's search default, adt_attn_stream.cuh) next to head size 128 at the same L, with achieved TFLOP/s (causal: half the
score / PV work of the full L x L products is counted)."""
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


if __name__ == "__main__":
    main()
