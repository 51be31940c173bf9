"""The reference of test_seq_layer_hip.py checked without a GPU (tests/seq_layer_cases.py): the harness's one-layer layout and the four oracle
layer functions assemble to so.forward / so.backward, the float64 bf16-operand mode agrees with the fp32-accumulating one, and the bounds of
every case are non-zero and set by the reference (where they reach the caps and where they do not is recorded in that test)."""
import numpy as np
import pytest

import seq_layer_cases as sc
from oracle import sasrec_oracle as so


def _model(H, L, B, p, seed):
    cfg = so.Cfg(50, L, sc.D, H, 1, dropout=p)
    P = {k: v.astype(np.float64) for k, v in so.init_params(cfg, seed=seed).items()}
    r = np.random.RandomState(seed)
    ids = [r.randint(1, cfg.item_num + 1, size=(B, L)) for _ in range(4)]
    for a in ids:
        a[0, :L // 2] = 0
        a[1, :1] = 0
    return cfg, P, ids


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("H", [1, 2])
def test_one_layer_model_from_layer_functions_equals_model_oracle(H, p):
    """so.forward / so.backward of a one-layer model against the same model put together here from the harness's names (sc.ENC_NAMES / DEC_NAMES,
    read back through its flat layout) and the four layer functions the GPU test uses as reference.  float64; equal to rounding."""
    L, B, seed, boff = 12, 3, 11, 5
    cfg, P, (seq, dec, pos, neg) = _model(H, L, B, p, 3)
    out = so.forward(P, cfg, seq, dec, pos, neg, training=True, seed=seed, b_offset=boff)
    r = np.random.RandomState(5)
    seeds = (r.randn(B, L), r.randn(B, L), [r.randn(B, L, sc.D)], [r.randn(B, L, sc.D)], [0.1 * r.randn(B, L, H, H) if H > 1 else None])
    G = so.backward(P, cfg, out[5], seeds, add_wd=False)

    def through_layout(kind, pre):      # the layer's tensors laid into the flat buffer and read back: the names, offsets and shapes of the harness
        lay, n = sc.layout(kind, H)
        flat = np.zeros(n)
        offs = sorted(o for o, _ in lay.values())
        assert all(o % 64 == 0 for o in offs) and len(lay) == 14
        for k, (o, shp) in lay.items():
            assert P[pre + k].shape == shp
            flat[o:o + P[pre + k].size] = P[pre + k].ravel()
        return {k: flat[o:o + int(np.prod(shp))].reshape(shp) for k, (o, shp) in lay.items()}
    Pe, Pd = through_layout("enc", sc.ENC_PRE), through_layout("dec", sc.DEC_PRE)
    E, Pw = P["item_emb.weight"], P["pos_emb.weight"]
    x, ec = so.embed(seq, E, Pw, p, seed, so.SITE_EMB_SEQ, boff)
    y1, rec, ce = so.encoder_layer(x, ec[1], Pe, "", H, p, seed, so.enc_sites(0), boff)
    f, lnc = so.layer_norm(y1, P["last_layernorm.weight"], P["last_layernorm.bias"])
    xd, dc = so.embed(dec, E, Pw, p, seed, so.SITE_EMB_DEC, boff)
    y2, cd = so.decoder_layer(xd, f, dc[1], Pd, "", H, p, seed, so.dec_sites(0), boff)
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-12)
    close((f * E[pos]).sum(-1), out[0])
    close(x, out[2][0])
    close(y2, out[3][0])
    close(rec, out[4][0])
    d_pos, d_neg, d_enc, d_dec, d_rec = seeds
    Gd, Ge = {}, {}
    gxd, gf = so.decoder_layer_bwd(d_dec[0], cd, Pd, "", H, Gd)
    df = d_pos[..., None] * E[pos] + d_neg[..., None] * E[neg] + gf
    dy1, glw, glb = so.layer_norm_bwd(df, lnc, P["last_layernorm.weight"])
    so.encoder_layer_bwd(dy1, d_rec[0], ce, Pe, "", H, Ge)
    close(glw, G["last_layernorm.weight"])
    for k in sc.DEC_NAMES:
        close(Gd[k], G[sc.DEC_PRE + k])
    for k in sc.ENC_NAMES:
        if G[sc.ENC_PRE + k] is None:
            assert H == 1 and k in sc.CLS and Ge[k] is None
        else:
            close(Ge[k], G[sc.ENC_PRE + k])


def test_block_offsets_are_the_64x64_weights():
    for kind, n in (("enc", 6), ("dec", 10)):
        lay, total = sc.layout(kind, 2)
        offs = sc.block_offsets(kind, 2)
        assert len(offs) == len(set(offs)) == n and all(o % 64 == 0 and o + 4096 <= total for o in offs)
        big = sorted(o + j * 4096 for o, shp in lay.values() if int(np.prod(shp)) >= 4096 for j in range(int(np.prod(shp)) // 4096))
        assert sorted(offs) == big


@pytest.mark.parametrize("c", [sc.Case("enc", 2, 20, 3, 0.3, 5, "x"), sc.Case("dec", 4, 20, 3, 0.3, 5, "x")], ids=sc.case_id)
def test_float64_bf16_operand_mode_equals_fp32_accumulating_mode(c):
    """operands("bf16x64") against operands("bf16") on the same float64 inputs: the same rounded operands, float64 against fp32 accumulation.
    Contractions here are 64 (projections), L (attention) and B * L (weight gradients) long: relative 1e-5 of each tensor's scale covers
    sqrt(n) * 2^-24 accumulated over the dozen products of a layer with room to spare, and is three orders below one bf16 rounding."""
    inp = sc.make_inputs(c)
    a, b = sc.run_oracle(c, inp, "bf16x64", kernel_roundings=False), sc.run_oracle(c, inp, "bf16", kernel_roundings=False)
    assert set(a) == set(b)
    a.pop("_u"), b.pop("_u")
    gmax = sc.grad_scale(a)
    for k in a:
        assert sc.dist(k, b[k], a[k], gmax) < 1e-5, k
    with so.operands("bf16x64"):          # the option is off unless asked for: the modes compute what they always did
        dy, x, w = (np.random.RandomState(i).randn(n, 5) for i, n in enumerate((7, 7, 5)))
        assert np.array_equal(so.linear_bwd(dy, x, w)[2], dy.sum(0))
    with so.operands("bf16x64", bias_as_product=True):
        assert np.allclose(so.linear_bwd(dy, x, w)[2], so.bf16_round(dy).astype(np.float64).sum(0), rtol=1e-14, atol=0)
    plain = sc.run_oracle(c, inp, None)
    assert sc.dist("y", plain["y"], a["y"], gmax) > 1e-4          # and the mode does round


@pytest.mark.parametrize("c", sc.CASES + sc.CONTRACT, ids=sc.case_id)
def test_bounds_are_set_by_the_reference(c):
    """Every compared tensor of every case has a bound that the reference itself sets: D_k > 0 (one pass of bf16 operand rounding moves it), the
    bound is min(2 D_k, cap), and for the activations (y, rec, the eval y) D_k is under the cap of 1e-2.

    For the GRADIENTS D_k is not under the cap of 0.05 everywhere, and the test records that instead of asserting it: measured over the table
    D_k is 0.02 - 0.03 in the median and 0.05 - 0.15 for 103 of 805 tensors (worst: dec H 4 L 4, three live rows, 0.149).  The cause is the
    ReLU of the feed-forward, not the arithmetic: operand rounding moves about 0.3 % of the pre-activations across zero, each such gate
    changes one element of the upstream gradient by all of itself, and a fraction f of changed elements is a relative Frobenius distance of
    sqrt(f), about 0.05.  The GPU test compares the backward at the gates the kernel saved (seq_layer_cases.py: the ReLU gate), so the kernels
    do not inherit this; where 2 D_k exceeds 0.05 the cap is the bound, which is tighter, never looser.  D_k stays under 0.15, the bound the project holds
    for fp32-operand against bf16-operand gradients (test_lean_step_with_dropout_vs_oracle), which is the comparison D_k is.
    Every bias gradient is the column sum of the rounded dY in the rounded run (so.operands(..., bias_as_product=True)), so the one tensor
    with no matrix product upstream, the second feed-forward bias, has D_k > 0 as well."""
    inp, want, Dk, bound, _ = sc.reference(c)
    expect = {"y", "gx"} | {"g." + k for k in sc.names(c.kind) if not (c.H == 1 and k in sc.CLS)}
    expect |= {"gfeats"} if c.kind == "dec" else {"y_eval"}
    if c.kind == "enc" and c.H > 1:
        expect |= {"rec", "n.gx"} | {"n.g." + k for k in sc.ENC_NAMES if k not in sc.CLS}
    assert set(want) == expect
    for k in want:
        assert np.isfinite(want[k]).all(), k
        cap = sc.CAP_ACT if sc.is_act(k) else sc.CAP_GRAD
        assert Dk[k] > 0.0 and bound[k] == min(sc.FACTOR * Dk[k], cap), (k, Dk[k])
        assert Dk[k] < (cap if sc.is_act(k) else 0.15), (k, Dk[k])


def test_pad_prefixes_cover_the_tile_edges_and_an_interior_zero():
    """Over the shape group: every prefix of {0, 1, 15, 16, 17, L - 1, L} at an L that does not clip it, and an interior zero id in every case
    that has a sequence with three live positions."""
    seen = set()
    for c in sc.CASES:
        ids = sc.make_inputs(c)["ids"]
        pre = sc.pad_prefixes(ids)
        seen |= {(p if p < c.L - 1 else ("L-1" if p == c.L - 1 else "L")) for p in pre if c.L >= 20}
        interior = any((row[p:] == 0).any() for row, p in zip(ids, pre))
        assert interior or all(c.L - p < 3 for p in pre), c
        assert (sc.make_inputs(c)["x"][ids == 0] == 0).all()
    assert seen >= {0, 1, 15, 16, 17, "L-1", "L"}, seen


def test_shard_reference_is_the_slice_of_the_full_batch():
    for c in sc.SHARD:
        inp = sc.make_inputs(c)
        full = sc.run_oracle(c, inp, "bf16x64", 0, (2, 5))
        cs = c._replace(B=3)
        part = dict(inp, ids=inp["ids"][2:5], x=inp["x"][2:5], gy=inp["gy"][2:5])
        if c.kind == "enc":
            part["drec"] = so.rec_reference_order(so.rec_token_order(inp["drec"])[2:5])
        else:
            part["feats"] = inp["feats"][2:5]
        alone = sc.run_oracle(cs, part, "bf16x64", 2)
        for k in ("y", "gx", "_u") + (("rec",) if c.kind == "enc" else ("gfeats",)):
            np.testing.assert_allclose(alone[k], full[k], rtol=1e-12, atol=1e-14, err_msg=k)
