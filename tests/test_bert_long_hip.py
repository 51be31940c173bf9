"""GPU: BERT4Rec-ADT past the length the resident masked-attention kernels hold (224 rows): BertModel._attn_drn hands its three attention
sites to the streamed kernels (ops.attn_long_fwd / _bwd) up to maxlen 1024.

Against (a) tests/golden/bert_l272.npz, recorded from the imported reference at L 272 (tools/gen_golden_wide.py bert_long; compacted: a
tensor above 2048 entries is its norm plus 512 strided samples), and (b) the numpy oracle with dropout on (shared hash RNG).  The helpers
and every bound are tests/test_bert_hip.py's: activations 1e-4 (fp32) / 3e-2 (bf16), fp32 gradients 3e-4, dropout-step gradients 5e-4, bf16
gradients relative Frobenius 0.1, graph against eager 1e-5 on the loss and 5e-4 on the weights.

The oracle cases draw the head classifier's bias at scale 0.3, not 0.02: its gradient is a sum over B L H rows that cancels down to about
lambda2 (b_i - b_j) / 4, and at B L of a thousand a 0.02 draw leaves a value of the size of the fp32 summation error of either side."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import bert_oracle as bo  # noqa: E402
from tests.test_bert_hip import Args, build, load_case, rel  # noqa: E402
from tests.test_bert_long_cpu import K, entries  # noqa: E402
from tools.gen_golden_inputs import golden_err  # noqa: E402

LAM1, LAM2 = [0.2], [0.1]


def gerr(t, g, key):
    return golden_err(t.detach().cpu().numpy() if hasattr(t, "detach") else t, g, key, K)


def oracle_case(d, H, L, seed, V=40, inner=96, dead_src=True):
    """Weights as tools/gen_golden_wide.py:gen_bert perturbs them (head classifier bias: see the module docstring) and a batch of three:
    row 0 without padding, row 1 with more than 200 pad positions, row 2 with every src id 0 and a non-empty dec (no attendable key in the
    encoder and in the cross-attention: the dead-row rule)."""
    cfg = bo.Cfg(V, L, d, H, 1, inner)
    P = bo.init_params(cfg, seed)
    r = np.random.RandomState(seed + 1)
    for k in P:
        if k.endswith("head_classifier.bias"):
            P[k] = (0.3 * r.standard_normal(P[k].shape)).astype(np.float32)
        elif k == "mask_bias" or (k.endswith(".bias") and "layer_norm" not in k):
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    src, dec, lab = (np.zeros((3, L), np.int64) for _ in range(3))
    for b, n in enumerate((L, L - 205, 40)):
        items = r.randint(1, V + 1, size=n)
        m = r.rand(n) < 0.3
        m[-1] = True
        dec[b, L - n:] = items
        src[b, L - n:] = np.where(m, V + 1, items)
        lab[b, L - n:] = np.where(m, items, 0)
    if dead_src:
        src[2] = 0
    return cfg, P, src, dec, lab


def grads_of(m, cfg, src, dec, lab, b_offset=0, n_valid=None, B_global=None):
    st = m.stage(src, dec, lab, n_valid_global=n_valid)
    B, L = (B_global or src.shape[0]), src.shape[1]
    norms = torch.tensor([0.0, B * L * cfg.hidden_units, B * L * cfg.num_heads], device="cuda:0")
    slots = torch.zeros(1 + 2 * cfg.num_layers, 64, device="cuda:0")
    m.flat_grad.zero_()
    m.loss_forward_backward(st, LAM1, LAM2, norms, slots, b_offset=b_offset)
    torch.cuda.synchronize()
    return slots


# ---- the reference's own numbers at L 272 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_l272_forward_and_predict_match_reference(prec):
    g, cfg, P = load_case("l272")
    assert cfg.maxlen == 272
    m = build(cfg, P, prec)
    m.eval()
    logits, enc_in, dec_out, rec = m(g["src"], g["dec"])
    tol = 1e-4 if prec == "f32" else 3e-2
    figs = {"logits": gerr(logits, g, "logits"), "enc_in_0": gerr(enc_in[0], g, "enc_in_0"), "dec_out_0": gerr(dec_out[0], g, "dec_out_0"),
            "rec_0": gerr(rec[0], g, "rec_0"), "predict": gerr(m.predict(None, g["src"], None, None, g["cand"]), g, "predict")}
    print(prec, figs)
    for k, e in figs.items():
        assert e < tol, (k, e)
    sd = m.state_dict()
    assert set(sd) == set(P) and all(tuple(sd[k].shape) == P[k].shape for k in P)


def test_l272_train_steps_match_reference_fp32():
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    g, cfg, P = load_case("l272")
    m = build(cfg, P, "f32")
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    tr = FusedBertTrainer(m, lam1, lam2, lr=float(g["lr"]), weight_decay=float(g["wd"]), clip=float(g["clip"]))
    tr.step(g["src"], g["dec"], g["labels"])
    torch.cuda.synchronize()
    print("loss %.7f (ref %.7f) grad norm %.7f (ref %.7f)" % (float(tr.loss()), float(g["loss"]), float(tr.grad_norm()), float(g["grad_norm"])))
    assert abs(float(tr.loss()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    assert abs(float(tr.grad_norm()) - float(g["grad_norm"])) < 3e-4 * float(g["grad_norm"])
    w1 = {k: rel(*entries(m.P(k).cpu().numpy(), g, "w1." + k)) for k in P}
    print("w1 worst", max(w1.items(), key=lambda kv: kv[1]))
    for k, e in w1.items():
        assert e < 2e-4, (k, e)
    tr.step(g["src"], g["dec"], g["labels"])
    tr.step(g["src"], g["dec"], g["labels"])
    w3 = {k: rel(*entries(m.P(k).cpu().numpy(), g, "w3." + k)) for k in P}
    print("w3 worst", max(w3.items(), key=lambda kv: kv[1]))
    for k, e in w3.items():
        assert e < 1e-3, (k, e)


# ---- the oracle, dropout on --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,L", [(64, 2, 225), (64, 4, 272), (128, 2, 300)])
def test_training_step_with_dropout_matches_oracle(d, H, L):
    """L 225: the first length past the bound, L & 3 != 0 (the other keep-mask path); 272: 17 tiles, the last group of four holds one; 300: a
    ragged last tile."""
    cfg, P, src, dec, lab = oracle_case(d, H, L, seed=d + H + L)
    cfg.dropout, cfg.attention_dropout = 0.2, 0.2
    m = build(cfg, P, "f32", 0.2, 0.2)
    m.train()
    m.set_seed(4242)
    slots = grads_of(m, cfg, src, dec, lab)
    loss, parts, G = bo.loss_and_grads(P, cfg, src, dec, lab, LAM1, LAM2, training=True, seed=4242)
    w = np.array([1.0] + LAM1 + LAM2)
    got = float((slots.sum(1).cpu().numpy() * w).sum())
    figs = {k: rel(m.G(k).cpu().numpy(), G[k]) for k in P}
    print("loss %.7f (oracle %.7f); worst gradient %s" % (got, loss, max(figs.items(), key=lambda kv: kv[1])))
    assert abs(got - loss) < 1e-4 * abs(loss)
    for k, e in figs.items():
        assert e < 5e-4, (k, e)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_l272_gradients_match_oracle(prec):
    cfg, P, src, dec, lab = oracle_case(64, 2, 272, seed=7)
    m = build(cfg, P, prec)
    m.train()
    grads_of(m, cfg, src, dec, lab)
    _, _, G = bo.loss_and_grads(P, cfg, src, dec, lab, LAM1, LAM2, training=True, seed=0)
    gmax = max(float(np.abs(G[k]).max()) for k in P)
    worst = (0.0, None)
    for k in P:
        got, want = m.G(k).cpu().numpy(), G[k]
        if prec == "f32":
            worst = max(worst, (rel(got, want), k))
            assert rel(got, want) < 3e-4, (k, rel(got, want))
        elif "key_transfer.bias" in k:
            assert np.abs(got).max() < 1e-3 * gmax, k
        else:
            fro = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-6)
            worst = max(worst, (fro, k))
            assert fro < 0.1, (k, fro)
    print(prec, "worst", worst)


def test_l272_dp_shard_equals_slice_of_global_batch():
    cfg, P, src, dec, lab = oracle_case(64, 2, 272, seed=8)
    cfg.dropout, cfg.attention_dropout = 0.2, 0.2
    B = src.shape[0]
    nv = int((lab != 0).sum())
    grads = []
    for lo, hi in ((0, B), (0, 1), (1, B)):          # the second shard starts at b_offset 1
        m = build(cfg, P, "f32", 0.2, 0.2)
        m.train()
        m.set_seed(777)
        grads_of(m, cfg, src[lo:hi], dec[lo:hi], lab[lo:hi], b_offset=lo, n_valid=nv, B_global=B)
        grads.append(m.flat_grad.cpu().numpy().copy())
    print("shards against the global batch", rel(grads[1] + grads[2], grads[0]))
    assert rel(grads[1] + grads[2], grads[0]) < 1e-4


def test_l272_graph_replay_equals_eager():
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    cfg, P, src, dec, lab = oracle_case(64, 2, 272, seed=9)
    outs = []
    for use_graph in (False, True):
        m = build(cfg, P, "bf16", 0.3, 0.2)
        tr = FusedBertTrainer(m, LAM1, LAM2, weight_decay=1e-4, use_graph=use_graph, seed=5)
        for _ in range(4):
            tr.step(src, dec, lab)
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().copy()))
    print("loss %.7f / %.7f, weights %.3g" % (outs[0][0], outs[1][0], rel(outs[1][1], outs[0][1])))
    assert abs(outs[0][0] - outs[1][0]) < 1e-5 * abs(outs[0][0])
    assert rel(outs[1][1], outs[0][1]) < 5e-4


# ---- ranking -----------------------------------------------------------------------------------------------------------------------
def test_l260_rank_full_recommend_and_evaluate_full():
    """tests/test_fullrank_hip.py::test_model_rank_full_and_recommend at maxlen 260: rank_full and recommend against the model's own
    materialised logits at the [MASK] position; evaluate_full's metrics against the ones computed from those logits on the host."""
    from adt_amd import ops
    from adt_amd.bert4rec.model import BertModel
    from tests.test_fullrank_hip import check_bracket, eligibility
    V, L, B, k = 200, 260, 9, 10
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", L, 2, 1, 64, 128
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = 0.0, 0.0, 2, "f32"
    torch.manual_seed(13)
    m = BertModel(1, V, a).eval()
    m.P("mask_bias").copy_(torch.randn(m.vocab) * 0.05)
    r = np.random.RandomState(5)
    seqs = r.randint(1, V + 1, size=(B, L)).astype(np.int32)
    seqs[:, :5] = 0
    seqs[1, :230] = 0
    seqs[:, -1] = V + 1
    target = r.randint(1, V + 1, B).astype(np.int32)
    dense = (r.rand(B, V + 1) < 0.1).astype(np.int8)
    dense[3] = 0
    dense[4, target[4]] = 1
    logits = m.predict(None, seqs, candidates=np.tile(np.arange(V + 1, dtype=np.int32), (B, 1))).cpu().numpy().astype(np.float64)
    F, E, n_items, bias = m._full_rank_operands(seqs)
    F64, E64 = F.cpu().numpy().astype(np.float64), E.cpu().numpy().astype(np.float64)[:V + 1]
    tol = 2.0 * F64.shape[1] * 2.0 ** -24 * (np.abs(F64) @ np.abs(E64).T)
    r_ip, r_ix = ops.seen_csr_host(dense, B)
    elig = eligibility(B, V, target, r_ip, r_ix)
    rank, nel, ti, tv = m.rank_full(seqs, target, dense, topk=k)
    assert np.array_equal(nel.cpu().numpy(), [(elig[b] & (np.arange(V + 1) != target[b])).sum() for b in range(B)])
    check_bracket(logits, tol, elig, target, k, rank.cpu().numpy(), ti.cpu().numpy(), tv.cpu().numpy().astype(np.float64), "bert L 260")
    rec_ids, rec_val = m.recommend(seqs, k, seen=dense)
    check_bracket(logits, tol, eligibility(B, V, np.zeros(B, np.int32), r_ip, r_ix), None, k, None, rec_ids.cpu().numpy(),
                  rec_val.cpu().numpy().astype(np.float64), "bert L 260 recommend")

    # evaluate_full on a data set of B users whose sequences, targets and seen items are the ones above
    from adt_amd.sasrec import utils as U

    class DS:
        mode, users = "test", list(range(B))
        user_train = {u: [int(i) for i in np.nonzero(dense[u])[0]] for u in range(B)}
        user_val, user_test = {}, {u: [int(target[u])] for u in range(B)}
        sequence = staticmethod(lambda u: seqs[u])
    (ndcg, ht), _ = U.evaluate_full(m, DS, "test", (5, 10), batch_size=4)
    want = U.metrics_from_stats(U.full_rank_stats(rank.cpu().numpy(), nel.cpu().numpy(), (5, 10)), (5, 10))[0]
    assert ndcg == want[0] and ht == want[1]


# ---- constructor, supernet ---------------------------------------------------------------------------------------------------------
def test_constructor_takes_1024_and_refuses_0_and_1025():
    from adt_amd._lib import AdtError
    from adt_amd.bert4rec.model import BertModel

    def make(L):
        a = Args()
        a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", L, 2, 1, 64, 96
        a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = 0.0, 0.0, 2, "bf16"
        return BertModel(1, 20, a)
    assert make(1024).maxlen == 1024 and make(1).maxlen == 1
    for L in (0, 1025):
        with pytest.raises(AdtError, match=r"d=64 H=2 L=%d" % L):
            make(L)


def test_supernet_smoke_at_maxlen_272():
    """SuperBertModel inherits the dispatch: one warm-up step and predict_rank_candidates at L 272, finite outputs (the search itself is not
    measured past 224)."""
    from adt_amd.bert4rec.superbert import SuperBertModel, SuperBertTrainer
    from adt_amd.supersearch import get_shared
    V, L, B = 40, 272, 2
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", L, 2, 1, 64, 256
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = 0.2, 0.2, 2, "bf16"
    torch.manual_seed(3)
    rec_choice, ind_choice = [0.1, 0.2], [0.05, 0.1]
    m = SuperBertModel(1, V, rec_choice, ind_choice, a)
    tr = SuperBertTrainer(m)
    cand = [0.15, 0.07]
    tr.set_choice(cand)
    _, _, src, dec, lab = oracle_case(64, 2, L, seed=4, V=V, dead_src=False)
    tr.step(src[:B], dec[:B], lab[:B])
    torch.cuda.synchronize()
    assert np.isfinite(float(tr.loss())) and bool(torch.isfinite(m.flat).all())
    cands = np.concatenate([lab[:B, -1:], np.random.RandomState(1).randint(1, V + 1, size=(B, 10))], 1)
    shared = [get_shared(m.rec_choice, m.ind_choice, np.asarray(c, np.float64)) for c in (cand, [0.1, 0.05])]
    rank = m.predict_rank_candidates(src[:B], cands, shared)
    assert tuple(rank.shape) == (2, B) and int(rank.min()) >= 0 and int(rank.max()) <= 10


# ---- the command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--eval_full", "1"], ["--device_batches"], ["--device_batches", "--fused_head"]],
                         ids=["host_batches", "device_batches", "device_batches_fused_head"])
def test_main_at_maxlen_300_end_to_end(tmp_path, capsys, extra):
    from adt_amd.bert4rec.main import main
    main(["--dataset", "ml-1m", "--data_dir", str(tmp_path), "--synthetic", "tiny", "--template", "0", "--num_epochs", "1", "--maxlen", "300",
          "--batch_size", "32", "--eval_batch_size", "24", "--eval_negative_sample_size", "10", "--dupe_factor", "2", "--prop_sliding_window", "0.5",
          "--hidden_units", "64", "--inner_units", "96"] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["epoch"] == 1 and lines[0]["sequences_per_sec"] > 0
    assert np.isfinite(lines[0]["loss"])
    for split in ("valid", "test"):
        assert 0.0 <= lines[0][split]["ndcg10"] <= 1.0 and 0.0 <= lines[0][split]["hr10"] <= 1.0 and 0.0 <= lines[0][split]["auc"] <= 1.0
