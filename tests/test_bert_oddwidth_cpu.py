"""CPU: BERT4Rec-ADT at the widths the kernels pad (hidden_units 50, 100, 150) and at head sizes 128 / 256.

(a) The numpy oracle (oracle/bert_oracle.py) against tests/golden/bert_{w50_h1,w50_h2,w100_h2,w150_h3,hd128,hd256}.npz, recorded from the
imported reference (tools/gen_golden_wide.py bert_odd; compacted: a tensor above 2048 entries is its Frobenius norm plus 320 strided
samples), at the bounds of tests/test_oracle_wide.py: 2e-5 forward, 5e-5 gradients.  With one head the reference leaves head_classifier.*
at grad None (`gnone.<name>` keys): the oracle's gradient there is exactly zero.

(b) The padded parameter table (adt_amd/bert4rec/model.py:padded_tables + adt_amd/wide.py:lane_index), pure numpy: the lane map is
injective and in range, covers every reference element exactly once and puts it where an explicit per-tensor construction of the padded
layout puts it; q / k / v stay consecutive for the packed GEMM views."""
import os

import numpy as np
import pytest

from oracle import bert_oracle as bo
from tools.gen_golden_inputs import golden_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ["w50_h1", "w50_h2", "w100_h2", "w150_h3", "hd128", "hd256"]
K = 320          # samples per compacted tensor (tools/gen_golden_wide.py:BERT_ODD_COMPACT)


def load_case(tag):
    g = np.load(os.path.join(GOLD, "bert_%s.npz" % tag))
    V, L, d, H, nl, inner = [int(x) for x in g["cfg"]]
    cfg = bo.Cfg(V, L, d, H, nl, inner)
    P = bo.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:   # same perturbation as tools/gen_golden_wide.py:gen_bert
        if k.endswith("head_classifier.bias") or k == "mask_bias" or (k.endswith(".bias") and "layer_norm" not in k):
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


def test_fixtures_are_small():
    for tag in TAGS:
        assert os.path.getsize(os.path.join(GOLD, "bert_%s.npz" % tag)) <= os.path.getsize(os.path.join(GOLD, "bert_l272.npz")), tag


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_forward_matches_reference(tag):
    g, cfg, P = load_case(tag)
    logits, enc_in, dec_out, rec = bo.forward(P, cfg, g["src"], g["dec"], training=False)
    figs = {"logits": golden_err(logits, g, "logits", K), "predict": golden_err(bo.predict(P, cfg, g["src"], g["cand"]), g, "predict", K)}
    for i in range(cfg.num_layers):
        figs["enc_in_%d" % i] = golden_err(enc_in[i], g, "enc_in_%d" % i, K)
        figs["dec_out_%d" % i] = golden_err(dec_out[i], g, "dec_out_%d" % i, K)
        figs["rec_%d" % i] = golden_err(rec[i], g, "rec_%d" % i, K)
    print(tag, figs)
    for k, e in figs.items():
        assert e < 2e-5, (k, e)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_gradients_match_reference(tag):
    g, cfg, P = load_case(tag)
    lam1, lam2 = list(g["lambda1"]), list(g["lambda2"])
    loss, parts, G = bo.loss_and_grads(P, cfg, g["src"], g["dec"], g["labels"], lam1, lam2, training=True, seed=0)
    assert abs(loss - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    none = sorted(f[6:] for f in g.files if f.startswith("gnone."))
    assert none == (sorted(k for k in P if ".head_classifier." in k) if cfg.num_heads == 1 else [])
    figs = {}
    for k in P:
        if k in none:
            assert not np.any(G[k]), k          # exactly zero
        else:
            figs[k] = golden_err(G[k], g, "grad." + k, K)
    print(tag, "worst", max(figs.items(), key=lambda kv: kv[1]))
    for k, e in figs.items():
        assert e < 5e-5, (k, e)


# ---- the padded table ---------------------------------------------------------------------------------------------------------------
def _expand(name, a, chan, dp, hd_pad, inner_pad):
    """The padded tensor of reference tensor `a`, built per tensor kind (not through lane_index)."""
    def rows(x, idx, n):          # axis 0: x's rows to positions idx of n rows
        out = np.zeros((n,) + x.shape[1:], x.dtype)
        out[idx] = x
        return out

    def cols(x, idx, n):
        out = np.zeros(x.shape[:1] + (n,), x.dtype)
        out[:, idx] = x
        return out
    if name == "mask_bias" or name.endswith("head_classifier.bias"):
        return a
    if name.endswith("head_classifier.weight"):
        return cols(a, np.arange(a.shape[1]), hd_pad)
    if name.endswith("fc1.weight"):
        return rows(cols(a, chan, dp), np.arange(a.shape[0]), inner_pad)
    if name.endswith("fc1.bias"):
        return rows(a, np.arange(a.shape[0]), inner_pad)
    if name.endswith("fc2.weight"):
        return rows(cols(a, np.arange(a.shape[1]), inner_pad), chan, dp)
    if "_emb.weight" in name:
        return cols(a, chan, dp)
    if a.ndim == 1:               # LayerNorm scale / shift, Linear biases of width d
        return rows(a, chan, dp)
    return rows(cols(a, chan, dp), chan, dp)      # the (d, d) projections


@pytest.mark.parametrize("d,H,inner", [(50, 1, 100), (50, 2, 100), (100, 2, 200), (150, 3, 64), (50, 1, 50)])
def test_padded_table_lane_map(d, H, inner):
    from adt_amd.bert4rec.model import padded_tables
    from adt_amd.wide import lane_index, padded_layout
    V, L, nl = 17, 9, 2
    hd, hd_pad, dp = padded_layout(d, H)
    inner_pad = (inner + 3) // 4 * 4
    ref, pad, prefix = padded_tables(V, L, d, H, nl, inner, 2)
    assert [n for n, _ in ref] == [n for n, _ in pad]
    offs, off = {}, 0
    for name, shape in pad:        # FlatModule._build_flat: every tensor on a 16-byte boundary
        offs[name] = off
        off += (int(np.prod(shape)) + 3) // 4 * 4
    n_flat = off
    idx = lane_index(ref, pad, offs, d, H, prefix=prefix).astype(np.int64)
    n_ref = sum(int(np.prod(s)) for _, s in ref)
    assert idx.size == n_ref                                  # every reference element once ...
    assert idx.min() >= 0 and idx.max() < n_flat              # ... in range ...
    assert np.unique(idx).size == idx.size                    # ... and nowhere twice
    # where an explicit construction of the padded layout puts them
    chan = (np.arange(d) // hd) * hd_pad + np.arange(d) % hd
    r = np.random.RandomState(d * 7 + H)
    flat = np.zeros(n_flat, np.float64)
    vals = []
    for (name, shape), (_, pshape) in zip(ref, pad):
        a = r.standard_normal(shape) + 3.0                    # never 0: a pad position cannot pass for a live one
        p = _expand(name, a, chan, dp, hd_pad, inner_pad)
        assert p.shape == tuple(pshape), (name, p.shape, pshape)
        flat[offs[name]:offs[name] + p.size] = p.reshape(-1)
        vals.append(a.reshape(-1))
    assert np.array_equal(flat[idx], np.concatenate(vals))
    live = np.zeros(n_flat, bool)
    live[idx] = True
    assert not flat[~live].any()                              # everything else is a pad lane or an alignment gap
    # q / k / v weights, then their biases, are consecutive: the packed (3 d_pad, d_pad) and (2 d_pad, d_pad) GEMM views
    for p in ["encoder.encoder_layers.%d.multi_head_attention" % i for i in range(nl)] + \
             ["decoder.decoder_layers.%d.%s" % (i, a) for i in range(nl) for a in ("dec_multi_head_attention", "src_dec_attention")]:
        q = offs[p + ".query_transfer.weight"]
        assert offs[p + ".key_transfer.weight"] == q + dp * dp and offs[p + ".value_transfer.weight"] == q + 2 * dp * dp
        b = offs[p + ".query_transfer.bias"]
        assert b == q + 3 * dp * dp and offs[p + ".key_transfer.bias"] == b + dp and offs[p + ".value_transfer.bias"] == b + 2 * dp


def test_widths_the_kernels_tile_need_no_table():
    from adt_amd.wide import padded_layout
    assert padded_layout(64, 2) == (32, 32, 64) and padded_layout(128, 1) == (128, 128, 128) and padded_layout(256, 2) == (128, 128, 256)
    assert padded_layout(50, 1) == (50, 64, 64) and padded_layout(150, 3) == (50, 64, 192)
