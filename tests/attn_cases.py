"""Shared by test_attn_cases_cpu.py and test_attn_branches_hip.py: the case table of the resident and chunked masked-attention kernels
(adt_amd/csrc/adt_attn_gen.cuh, named in adt_wide.hip: launch_attn, launch_attn_gen_l, launch_attn_gen_128), the inputs of a case and the
float64 reference.

A case is (prec, H, hd, L, mask, fill, p, scale).  mask: "causal" (no key ids), "keypad" (key ids, not causal), "both".  scale None is the
plain entry point (1 / sqrt(hd)); a number is the scaled entry point, and then the last hd - round(1 / scale^2) lanes of every head are zero
in Q, K, V and dO and the reference runs at the true head size.  Instead of a cross product over the masks, the mask modes and the two
dropout settings rotate over the lengths of one kernel instantiation; test_attn_cases_cpu.py proves that every instantiation still sees
every mode that can reach it, and dropout off and on.
"""
import math

import numpy as np

F32, BF16 = 0, 1
NINF = float("-inf")
B = 3
SEED, SITE, B_OFF = 99, 17, 5

# (mask, fill): the SASRec mask as the model code passes it, BERT's key padding, both
MODES = (("causal", NINF), ("keypad", -1e9), ("both", -1e9))
# head size 128 also: the causal tile skip (CSK) switched on by a finite fill <= -1e9, and off by a fill above it under the same mask
MODES_128 = MODES + (("causal", -1e9), ("causal", -1e4))

# lengths per instantiation: MAXKT 4 | 8 | 14 (fp32 hd 64 backward: chunked 16 / 2).  100 is there so that MAXKT 8 has three lengths for three modes.
LENGTHS = ((1, 16, 37, 64), (65, 100, 128), (129, 200, 224))
LENGTHS_128_SHORT = (1, 50, 64, 17, 33)          # both precisions: resident forward at MAXKT 4, one-chunk backward
LENGTHS_128_LONG = (65, 130, 200, 256, 97)       # bf16 only: five and seven tiles (last pair half empty), L % 4 = 2 and 1, LP completely full


def _rotate(prec, H, hd, lengths, modes, start):
    """One case per length; the mode advances with the length, dropout goes by the mode's position (modes 0 and 3, the two that switch CSK on,
    differ in it, and so do the three that leave it off)."""
    idx = [(start + i) % len(modes) for i in range(len(lengths))]
    return [(prec, H, hd, L) + modes[m] + (0.2 if (m + start) % 2 else 0.0, None) for m, L in zip(idx, lengths)]


def _table():
    cases = []
    for prec in (F32, BF16):
        for n, hd in enumerate((16, 32, 64)):
            for gi, group in enumerate(LENGTHS):
                cases += _rotate(prec, 2, hd, group, MODES, n + prec + gi)
        cases += _rotate(prec, 2, 128, LENGTHS_128_SHORT, MODES_128, prec)
    cases += _rotate(BF16, 2, 128, LENGTHS_128_LONG, MODES_128, 2)
    # the scaled entry points: heads padded with zero lanes keep 1 / sqrt(true head size)
    cases += [(F32, 2, 32, 37, "both", -1e9, 0.2, 1 / math.sqrt(25)), (BF16, 2, 32, 130, "causal", NINF, 0.0, 1 / math.sqrt(25)),
              (F32, 2, 64, 200, "causal", NINF, 0.2, 1 / math.sqrt(50)), (BF16, 2, 64, 65, "keypad", -1e9, 0.0, 1 / math.sqrt(50)),
              (F32, 2, 128, 50, "keypad", -1e9, 0.0, 1 / math.sqrt(100)), (BF16, 2, 128, 200, "causal", -1e9, 0.2, 1 / math.sqrt(100))]
    return cases


CASES = _table()

# (c) mask leaks: one length per backward instantiation, with an odd number of 16-row tiles and L % 4 != 0, dropout on
LEAK_CASES = [(prec, 2, hd, L) for prec in (F32, BF16) for hd in (16, 32, 64) for L in (37, 101, 203)]
LEAK_CASES += [(F32, 2, 128, 37), (BF16, 2, 128, 37), (BF16, 2, 128, 203)]

# (d) the instantiations only bf16 reaches (hd 128, L > 64): (L, mask, fill, p)
SHARP_CASES = [(256, "causal", -1e9, 0.2), (200, "causal", -1e4, 0.0), (130, "keypad", -1e9, 0.2), (65, "causal", NINF, 0.0)]


def case_id(case):
    prec, H, hd, L, mask, fill, p, scale = case
    return "%s-hd%d-L%d-%s%g-p%g%s" % ("bf16" if prec else "f32", hd, L, mask, fill, p, "" if scale is None else "-true%d" % true_hd(hd, scale))


def true_hd(hd, scale):
    return hd if scale is None else int(round(1.0 / (scale * scale)))


def flags(mask):
    """(causal, has key ids)"""
    return mask != "keypad", mask != "causal"


def inst_key(expect_attn, prec, hd, L, bwd, mask, fill):
    """The kernel instantiation a call gets: (direction, prec, hd, family, maxkt, nch, csk), from the plan's restatement (test_wide_plan_cpu.expect_attn)."""
    causal, kid = flags(mask)
    e = expect_attn(prec, hd, L, int(bwd), int(causal), int(kid), fill)
    assert not isinstance(e, str), e
    family, maxkt, nch, _kc, _waves, csk = e[:6]
    return ("bwd" if bwd else "fwd", prec, hd, family, maxkt, nch, int(csk))


def key_ids(r, L, mask):
    """(ids or None, valid): sequence 0 left-padded by L // 3, sequence 2 fully padded (finite fill only: with -inf the reference is NaN)."""
    if mask == "causal":
        return None, np.ones((B, L), bool)
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    ids[0, : L // 3] = 0
    ids[2, :] = 0
    return ids, ids > 0


def make_inputs(case):
    """(qkv (B L, 3 d), dO (B L, d), ids or None, valid (B, L)) of a case, float32; zero lanes at the end of every head of a scaled case."""
    prec, H, hd, L, mask, fill, p, scale = case
    d = H * hd
    r = np.random.RandomState(1000 * hd + 7 * L + 3 * prec + {"causal": 0, "keypad": 1, "both": 2}[mask])
    qkv = r.standard_normal((B * L, 3 * d)).astype(np.float32)
    dO = r.standard_normal((B * L, d)).astype(np.float32)
    t = true_hd(hd, scale)
    if t < hd:
        qkv.reshape(B * L, 3 * H, hd)[:, :, t:] = 0
        dO.reshape(B * L, H, hd)[:, :, t:] = 0
    ids, valid = key_ids(r, L, mask)
    return qkv, dO, ids, valid


def true_lanes(x, H, hd, t):
    """(T, H hd) -> (T, H t): the first t lanes of every head."""
    return np.ascontiguousarray(x.reshape(x.shape[0], H, hd)[:, :, :t]).reshape(x.shape[0], H * t)


def attn_mask(nB, H, L, valid, causal):
    mask = np.broadcast_to(~valid[:, None, None, :], (nB, H, L, L)).copy()
    if causal:
        mask |= np.triu(np.ones((L, L), bool), 1)[None, None]
    return mask


def ref64(q, k, v, dO, nB, H, L, valid, causal, fill, p, seed, site, b_off, scale):
    """test_wide_kernels.attn_oracle in float64 closed form, with the score scale as an argument: softmax(masked_fill(scale q k^T, mask, fill))
    -> dropout -> @ v and its gradients.  Returns a dict: o, dq, dk, dv (T, d); lse (nB, H, L), log L on rows whose every score is filled
    (the kernels use 0 instead of the fill there: the same uniform probabilities); w (nB, H, L, L), the dropped and rescaled probabilities;
    qk (nB, H, L), max over the keys of scale * sum |q_i| |k_i| (what bounds the score error of rounded operands)."""
    from oracle import rng, tape as tp
    d = q.shape[1]
    hd = d // H

    def split(x):
        return np.asarray(x, np.float64).reshape(nB, L, H, hd).transpose(0, 2, 1, 3)

    def merge(x):
        return x.transpose(0, 2, 1, 3).reshape(nB * L, d)
    Q, K, V, G = split(q), split(k), split(v), split(dO)
    KT = K.transpose(0, 1, 3, 2)
    mask = attn_mask(nB, H, L, valid, causal)
    s = np.where(mask, float(fill), (Q @ KT) * scale)
    m = s.max(-1, keepdims=True)
    assert np.isfinite(m).all(), "a fully masked row under an infinite fill"
    e = np.exp(s - m)
    z = e.sum(-1, keepdims=True)
    P = e / z
    lse = np.where(mask.all(-1), math.log(L), (m + np.log(z))[..., 0])
    ks = 1.0
    if p > 0.0:
        ks = rng.keep_mask(seed, site, tp.idx_attn(nB, H, L, b_off), p).astype(np.float64) / (1.0 - rng.drop_prob(p))
    W = P * ks
    dP = (G @ V.transpose(0, 1, 3, 2)) * ks
    dS = np.where(mask, 0.0, P * (dP - (dP * P).sum(-1, keepdims=True)))
    return dict(o=merge(W @ V), dq=merge(dS @ K) * scale, dk=merge(dS.transpose(0, 1, 3, 2) @ Q) * scale, dv=merge(W.transpose(0, 1, 3, 2) @ G),
                lse=lse, w=W, qk=(np.abs(Q) @ np.abs(KT)).max(-1) * scale)


def tape_oracle(q, k, v, dO, nB, H, L, valid, causal, fill, p, seed, site, b_off, scale=None):
    """test_wide_kernels.attn_oracle / test_attn_hd256_hip.attn_oracle (the float32 tape of oracle/tape.py), extended with the score scale."""
    from oracle import tape as tp
    d = q.shape[1]
    hd = d // H
    vq, vk, vv = tp.leaf(q), tp.leaf(k), tp.leaf(v)

    def split(x):
        return tp.transpose(tp.reshape(x, (nB, L, H, hd)), (0, 2, 1, 3))
    s = tp.matmul(split(vq), tp.transpose(split(vk), (0, 1, 3, 2)))
    s = tp.div_const(s, np.sqrt(hd)) if scale is None else tp.scale(s, scale)
    s = tp.masked_fill(s, attn_mask(nB, H, L, valid, causal), fill)
    w = tp.dropout(tp.softmax(s), p, seed, site, tp.idx_attn(nB, H, L, b_off))
    o = tp.reshape(tp.transpose(tp.matmul(w, split(vv)), (0, 2, 1, 3)), (nB * L, d))
    tp.backward(o, dO)
    return o.v, vq.g, vk.g, vv.g


def reference(case):
    """ref64 of a case's inputs, at the true head size."""
    prec, H, hd, L, mask, fill, p, scale = case
    qkv, dO, ids, valid = make_inputs(case)
    d, t = H * hd, true_hd(hd, scale)
    q, k, v = (true_lanes(qkv[:, i * d:(i + 1) * d], H, hd, t) for i in range(3))
    return ref64(q, k, v, true_lanes(dO, H, hd, t), B, H, L, valid, flags(mask)[0], fill, p, SEED, SITE, B_OFF, 1.0 / math.sqrt(hd) if scale is None else scale)
