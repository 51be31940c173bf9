#!/usr/bin/env python3
"""Stand-alone timing of the STOSA-ADT distance attention: the streamed matrix-core kernels (ops.wattn_long_* / klattn_long_*,
adt_wattn_long.cuh) next to the existing entry points (ops.wattn_* / klattn_* with prec: the resident matrix-core kernels at head size
16 / 32 and L <= 128, the vector-ALU kernels elsewhere) on the same tensors, alternating, three rounds each, the median reported; then
the streamed kernels alone at L 512 and 1024.  B 256, every sequence with a padded prefix of L / 4 positions (queries without an attendable
key), attention dropout 0.2, both metrics, bf16 and fp32, forward and backward.

    python tools/bench_wattn_long.py [out.jsonl]
    python tools/bench_wattn_long.py --hd128 [out.jsonl]

--hd128: head size 128 (ops.wattn_hd128_* / klattn_hd128_*, adt_wattn_hd128.hip) at d 128 / one head next to its twin,
the streamed head-size-64 kernels at two heads on the same (T, 384) tensors -- the same score and context arithmetic per sequence -- at
L 100 and 512, alternating, three rounds, medians, and the ratio to the twin.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from adt_amd import ops  # noqa: E402
from tools.bench_dense import timeit  # noqa: E402

# (head size, heads, L, what the existing entry points run there)
BOTH = [(16, 4, 100, "resident mfma"), (64, 1, 100, "vector alu"), (32, 2, 128, "resident mfma"), (32, 2, 256, "vector alu")]
LONG_ONLY = [(hd, H, L, None) for L in (512, 1024) for hd, H in ((16, 4), (64, 1), (32, 2))]


def main(jsonl=None):
    dev = torch.device("cuda:0")
    seed = torch.tensor([7], device=dev, dtype=torch.int32)
    B, p = 256, 0.2
    out = open(jsonl, "w") if jsonl else None
    for hd, H, L, existing in BOTH + LONG_ONLY:
        d, T = H * hd, B * L
        g = torch.Generator(device=dev).manual_seed(hd * 1000 + L)
        m3 = torch.randn(T, 3 * d, device=dev, generator=g)
        c3 = torch.exp(0.5 * torch.randn(T, 3 * d, device=dev, generator=g))
        t6 = (m3[:, :d], c3[:, :d], m3[:, d:2 * d], c3[:, d:2 * d], m3[:, 2 * d:], c3[:, 2 * d:])      # the model's packed (T, 3d) projections
        ids = torch.randint(1, 100, (B, L), device=dev, dtype=torch.int32)
        ids[:, : L // 4] = 0
        kid = ids.view(-1)
        dOm, dOc = torch.randn(T, d, device=dev, generator=g), torch.randn(T, d, device=dev, generator=g)
        for metric in ("wasserstein", "kl"):
            lf, lb = (ops.klattn_long_fwd, ops.klattn_long_bwd) if metric == "kl" else (ops.wattn_long_fwd, ops.wattn_long_bwd)
            ef, eb = (ops.klattn_fwd, ops.klattn_bwd) if metric == "kl" else (ops.wattn_fwd, ops.wattn_bwd)
            for pname, prec in (("bf16", ops.PREC_BF16), ("f32", ops.PREC_F32)):
                def pair(fwd, bwd):
                    Om, Oc, LSE = fwd(*t6, kid, B, H, L, p, seed, 16, 0, prec=prec)
                    return (lambda: fwd(*t6, kid, B, H, L, p, seed, 16, 0, prec=prec),
                            lambda: bwd(*t6, kid, Om, Oc, LSE, dOm, dOc, B, H, L, p, seed, 16, 0, prec=prec))
                fams = [("long", pair(lf, lb))]
                if existing:
                    fams.append((existing, pair(ef, eb)))
                times = {nm: ([], []) for nm, _ in fams}
                for _ in range(3 if existing else 1):
                    for nm, (f, b) in fams:
                        times[nm][0].append(timeit(f))
                        times[nm][1].append(timeit(b))
                for nm, _ in fams:
                    rec = dict(kernel=nm, metric=metric, prec=pname, hd=hd, H=H, B=B, L=L, p=p, fwd_us=round(float(np.median(times[nm][0])), 1),
                               bwd_us=round(float(np.median(times[nm][1])), 1), fwd_rounds=[round(x, 1) for x in times[nm][0]],
                               bwd_rounds=[round(x, 1) for x in times[nm][1]])
                    print(json.dumps(rec), flush=True)
                    if out:
                        out.write(json.dumps(rec) + "\n")
                        out.flush()


def main_hd128(jsonl=None):
    dev = torch.device("cuda:0")
    seed = torch.tensor([7], device=dev, dtype=torch.int32)
    B, p, d = 256, 0.2, 128
    scaled = (1.0 / np.sqrt(128.0), 128)
    out = open(jsonl, "w") if jsonl else None
    for L in (100, 512):
        T = B * L
        g = torch.Generator(device=dev).manual_seed(128000 + L)
        m3 = torch.randn(T, 3 * d, device=dev, generator=g)
        c3 = torch.exp(0.5 * torch.randn(T, 3 * d, device=dev, generator=g))
        t6 = (m3[:, :d], c3[:, :d], m3[:, d:2 * d], c3[:, d:2 * d], m3[:, 2 * d:], c3[:, 2 * d:])
        ids = torch.randint(1, 100, (B, L), device=dev, dtype=torch.int32)
        ids[:, : L // 4] = 0
        kid = ids.view(-1)
        dOm, dOc = torch.randn(T, d, device=dev, generator=g), torch.randn(T, d, device=dev, generator=g)
        for metric in ("wasserstein", "kl"):
            nf, nb = (ops.klattn_hd128_fwd, ops.klattn_hd128_bwd) if metric == "kl" else (ops.wattn_hd128_fwd, ops.wattn_hd128_bwd)
            tf, tb = (ops.klattn_long_fwd, ops.klattn_long_bwd) if metric == "kl" else (ops.wattn_long_fwd, ops.wattn_long_bwd)
            for pname, prec in (("bf16", ops.PREC_BF16), ("f32", ops.PREC_F32)):
                def pair(fwd, bwd, H, extra):
                    Om, Oc, LSE = fwd(*t6, kid, B, H, L, *extra, p, seed, 16, 0, prec=prec)
                    return (lambda: fwd(*t6, kid, B, H, L, *extra, p, seed, 16, 0, prec=prec),
                            lambda: bwd(*t6, kid, Om, Oc, LSE, dOm, dOc, B, H, L, *extra, p, seed, 16, 0, prec=prec))
                fams = [("hd128 H1", 128, 1, pair(nf, nb, 1, scaled)), ("long hd64 H2 (twin)", 64, 2, pair(tf, tb, 2, ()))]
                times = {nm: ([], []) for nm, _, _, _ in fams}
                for _ in range(3):
                    for nm, _, _, (f, b) in fams:
                        times[nm][0].append(timeit(f))
                        times[nm][1].append(timeit(b))
                med = {nm: (float(np.median(times[nm][0])), float(np.median(times[nm][1]))) for nm in times}
                for nm, hd, H, _ in fams:
                    rec = dict(kernel=nm, metric=metric, prec=pname, hd=hd, H=H, B=B, L=L, p=p, fwd_us=round(med[nm][0], 1), bwd_us=round(med[nm][1], 1),
                               fwd_rounds=[round(x, 1) for x in times[nm][0]], bwd_rounds=[round(x, 1) for x in times[nm][1]])
                    if hd == 128:
                        twin = med[fams[1][0]]
                        rec["fwd_vs_twin"], rec["bwd_vs_twin"] = round(med[nm][0] / twin[0], 2), round(med[nm][1] / twin[1], 2)
                    print(json.dumps(rec), flush=True)
                    if out:
                        out.write(json.dumps(rec) + "\n")
                        out.flush()


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--hd128"]
    (main_hd128 if "--hd128" in sys.argv[1:] else main)(argv[0] if argv else None)
