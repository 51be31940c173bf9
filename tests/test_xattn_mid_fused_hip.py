"""The decoder's cross-attention backward and the mid chain behind it in one launch per sequence (adt_seqxattn_tt.cuh,
k_seqtt_xattn_mid_bwd) against the two launches it stands for (k_seq_attn_bwd + k_seqtt_mid_bwd): the fusion keeps dq2 / dk2 / dv2 in
registers with the rounding of the HBM hand-over and reorders no sum, so the standard is BIT equality of everything a training step
leaves behind, not a tolerance.

ADT_XATTN_FUSED is read once per process, so each arm is a fresh child process (ADT_ITEM_SORT=1: bit-reproducible table gradients;
ADT_SEQ_SPLIT=1: one workgroup per sequence at these small batches, the mapping the flagship batch runs with).  A child builds small
SASRecADT bf16 models, runs three FusedTrainer steps per case and reports the SHA-256 of the loss bits, the gradient, the gradient norm,
the weights and the Adam moments after every step, and how many fused launches the process has issued."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NITEMS, NSTEPS = 50, 3
# (H, L, B, layers, dropout)
CASES = [
    (2, 200, 3, 2, 0.5),     # the flagship's 13 tiles with the half-full last tile
    (2, 224, 2, 1, 0.5),     # the 14-tile limit
    (2, 132, 2, 2, 0.5),     # nine tiles; npair = 5, the first size past the npair <= 4 branch of sb_dw_product16
    (4, 40, 2, 1, 0.25),     # hd 16; L a multiple of neither 16 nor 32
    (1, 16, 2, 1, 0.0),      # hd 64, no dropout, one tile, every other wave idle
    # the three instantiations the cases above leave out (head size x dropout mode), each at a small odd shape
    (1, 40, 2, 1, 0.25),     # hd 64 with saved keep bits
    (2, 40, 2, 1, 0.0),      # hd 32 without dropout
    (4, 24, 2, 1, 0.0),      # hd 16 without dropout
]


def _batch(r, B, L):
    """Row 0 full length, row 1 left-padded to under a quarter of L, any further row in between; items from NITEMS ids."""
    seq, dec, pos, neg = (np.zeros((B, L), np.int32) for _ in range(4))
    for b in range(B):
        n = L if b == 0 else max(1, L // 4 - 1 - int(r.randint(0, max(1, L // 8)))) if b == 1 else int(r.randint(L // 4, L))
        items = r.randint(1, NITEMS + 1, size=n + 1)
        seq[b, L - n:] = items[:-1]
        pos[b, L - n:] = items[1:]
        neg[b, L - n:] = r.randint(1, NITEMS + 1, size=n)
        dec[b, 1:] = seq[b, :-1]
    assert np.count_nonzero(seq[0]) == L and 0 < np.count_nonzero(seq[1]) < L / 4
    return seq, dec, pos, neg


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _child(cases, out_path):
    """Runs in the child process: every case, three steps each; writes the hashes and the fused-launch count as JSON."""
    import ctypes
    import torch
    from adt_amd import _lib
    from adt_amd.sasrec.model import SASRecADT
    from adt_amd.sasrec.trainer import FusedTrainer

    lib = _lib.load()
    lib.adt_seq_xattn_fused_launches.restype = ctypes.c_ulonglong
    lib.adt_seq_xattn_fused_launches.argtypes = []
    result = {"cases": []}
    for ci, (H, L, B, NL, p) in enumerate(cases):
        class Args:
            device, maxlen, num_heads, num_layers, precision, hidden_units, dropout = "cuda:0", L, H, NL, "bf16", 64, p
        torch.manual_seed(100 + ci)
        m = SASRecADT(1, NITEMS, Args())
        assert m.lib.adt_seq_layer_supported(1, L, 64, 64 // H) == 1, (H, L)
        m.train()
        tr = FusedTrainer(m, [0.1] * NL, [0.05] * NL, weight_decay=1e-3, seed=7 + ci)
        r = np.random.RandomState(1000 + ci)
        steps = []
        for _ in range(NSTEPS):
            tr.step(*_batch(r, B, L))
            torch.cuda.synchronize()
            steps.append({"loss": _sha(tr.loss()), "grad": _sha(m.flat_grad), "grad_norm": _sha(tr.grad_norm()),
                          "weights": _sha(m.flat), "adam_m": _sha(tr.m), "adam_v": _sha(tr.v),
                          "finite": bool(torch.isfinite(m.flat_grad).all()) and bool(torch.isfinite(tr.loss()))})
        result["cases"].append(steps)
    result["fused_launches"] = int(lib.adt_seq_xattn_fused_launches())
    with open(out_path, "w") as f:
        json.dump(result, f)
    return True


def _run_arm(fused, cases, tmp_path, tag):
    out = os.path.join(str(tmp_path), "xattn_%s.json" % tag)
    env = dict(os.environ, ADT_ITEM_SORT="1", ADT_SEQ_SPLIT="1", ADT_XATTN_FUSED="1" if fused else "0")
    code = ("import sys; sys.path.insert(0, %r); from tests.test_xattn_mid_fused_hip import _child; assert _child(%r, %r); print('xattn-child-ok')"
            % (REPO, cases, out))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "xattn-child-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


def test_fused_launch_is_bit_equal_to_the_two_launches(tmp_path):
    """Every hash of every step of every case is equal between ADT_XATTN_FUSED=0 and the default, and the fused arm really took the fused
    launch (one per decoder layer and step: the counter), the other never."""
    two = _run_arm(False, CASES, tmp_path, "two")
    one = _run_arm(True, CASES, tmp_path, "fused")
    print("fused launches: %d (fused arm), %d (two-launch arm)" % (one["fused_launches"], two["fused_launches"]))
    assert two["fused_launches"] == 0
    assert one["fused_launches"] == sum(NSTEPS * c[3] for c in CASES), one["fused_launches"]
    for case, a, b in zip(CASES, two["cases"], one["cases"]):
        for k, (sa, sb) in enumerate(zip(a, b)):
            assert sa["finite"] and sb["finite"], (case, k)
            diff = [key for key in sa if sa[key] != sb[key]]
            assert not diff, "case %s step %d: %s differ between the two launches and the fused one" % (case, k + 1, diff)


def test_fused_launch_is_deterministic_run_to_run(tmp_path):
    """Case 1 twice in the fused arm, two processes: equal hashes."""
    a = _run_arm(True, CASES[:1], tmp_path, "run_a")
    b = _run_arm(True, CASES[:1], tmp_path, "run_b")
    assert a["fused_launches"] == b["fused_launches"] == NSTEPS * CASES[0][3]
    assert a["cases"] == b["cases"]
