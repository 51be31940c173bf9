"""dO handed from an out-projection reverse to the attention backward behind it as bf16 operand rows plus delta (adt_tt.cuh:
tt_head_delta, tt_head_delta_chunks; BwdChainArgs / SeqBwdArgs / AttnArgs::do_bf16) against the fp32 dO rows it replaces (ADT_DO_BF16=0).  The producer rounds
dO * drop.scale as the consumer would have and forms delta = rowsum(dO . O) per head with the consumer's own function, so the standard is
BIT equality of everything a training step leaves behind, not a tolerance.

ADT_DO_BF16 is read once per process, so each arm is a fresh child process (ADT_ITEM_SORT=1: bit-reproducible table gradients).  A child
builds small SASRecADT bf16 models, runs three FusedTrainer steps per case and reports the SHA-256 of the loss bits, the gradient, the
gradient norm, the weights and the Adam moments after every step, and how many launches of an attention backward took the hand-over."""
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
    (2, 200, 3, 2, 0.5),     # 13 tiles, two-tile waves, half-full last tile; two layers: every producer -> consumer pair occurs
    (2, 224, 2, 1, 0.5),     # the 14-tile limit
    (4, 40, 2, 1, 0.25),     # hd 16, where the handed-over rows are not yet the operand
    (1, 40, 2, 1, 0.25),     # hd 64, no head classifier
    (2, 40, 2, 1, 0.0),      # no dropout, scale 1
]
# (ADT_SEQ_SPLIT, ADT_XATTN_FUSED) -- None: left unset
SETTINGS = {
    "one_wg_fused": ("1", None),       # one workgroup per sequence, the mid chain inside k_seqtt_xattn_mid_bwd
    "one_wg_two_launches": ("1", "0"),  # one workgroup per sequence, stand-alone k_seq_attn_bwd + k_seqtt_mid_bwd
    "split": (None, None),             # several workgroups per sequence (these batches: 8), stand-alone pair, two-workgroup k_seqtt_attn_pre_bwd
}


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
    """Runs in the child process: every case, three steps each; writes the hashes and the hand-over launch count as JSON."""
    import ctypes
    import torch
    from adt_amd import _lib
    from adt_amd.sasrec.model import SASRecADT
    from adt_amd.sasrec.trainer import FusedTrainer

    lib = _lib.load()
    lib.adt_seq_do_handover_launches.restype = ctypes.c_ulonglong
    lib.adt_seq_do_handover_launches.argtypes = []
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
    result["handover_launches"] = int(lib.adt_seq_do_handover_launches())
    with open(out_path, "w") as f:
        json.dump(result, f)
    return True


def _run_arm(handover, setting, cases, tmp_path, tag):
    out = os.path.join(str(tmp_path), "do_%s.json" % tag)
    env = dict(os.environ, ADT_ITEM_SORT="1")
    for k in ("ADT_DO_BF16", "ADT_SEQ_SPLIT", "ADT_XATTN_FUSED"):
        env.pop(k, None)
    split, fused = SETTINGS[setting]
    if split is not None:
        env["ADT_SEQ_SPLIT"] = split
    if fused is not None:
        env["ADT_XATTN_FUSED"] = fused
    if not handover:
        env["ADT_DO_BF16"] = "0"
    code = ("import sys; sys.path.insert(0, %r); from tests.test_do_handover_hip import _child; assert _child(%r, %r); print('do-child-ok')"
            % (REPO, cases, out))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "do-child-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_handover_is_bit_equal_to_fp32_rows(setting, tmp_path):
    """Every hash of every step of every case is equal between ADT_DO_BF16=0 and the default, and the default arm really took the hand-over
    (three attention backwards per layer and step -- the encoder block, the decoder's cross-attention and its self-attention block: the
    counter), the other never."""
    off = _run_arm(False, setting, CASES, tmp_path, "off")
    on = _run_arm(True, setting, CASES, tmp_path, "on")
    print("hand-over launches: %d (default arm), %d (ADT_DO_BF16=0 arm)" % (on["handover_launches"], off["handover_launches"]))
    assert off["handover_launches"] == 0
    assert on["handover_launches"] == sum(NSTEPS * 3 * c[3] for c in CASES), on["handover_launches"]
    for case, a, b in zip(CASES, off["cases"], on["cases"]):
        for k, (sa, sb) in enumerate(zip(a, b)):
            assert sa["finite"] and sb["finite"], (case, k)
            diff = [key for key in sa if sa[key] != sb[key]]
            assert not diff, "case %s step %d: %s differ between fp32 dO rows and the hand-over" % (case, k + 1, diff)


def test_handover_is_deterministic_run_to_run(tmp_path):
    """Case 1 twice in the hand-over arm, two processes: equal hashes."""
    a = _run_arm(True, "one_wg_fused", CASES[:1], tmp_path, "run_a")
    b = _run_arm(True, "one_wg_fused", CASES[:1], tmp_path, "run_b")
    assert a["handover_launches"] == b["handover_launches"] == NSTEPS * 3 * CASES[0][3]
    assert a["cases"] == b["cases"]
