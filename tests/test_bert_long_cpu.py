"""CPU: oracle/bert_oracle.py reproduces the L = 272 fixture recorded from the imported reference (tools/gen_golden_wide.py bert_long;
tests/golden/bert_l272.npz: 40 items, d 64, two heads, one layer, inner 96, B 2 -- row 0 with 250 real items, row 1 with 31 behind 241
pad positions), at the bounds tests/test_oracle_wide.py uses for the existing BERT fixtures: forward fields, predict, the loss and the clip
norm 2e-5, gradients 5e-5, weights after one and three Adam steps in units of lr (its _adam_close).  The fixture is compacted: a tensor above
2048 entries is its Frobenius norm plus 512 strided samples (tools/gen_golden_inputs.py:compact), and golden_err checks both."""
import os

import numpy as np
import pytest

from oracle import bert_oracle as bo
from tools.gen_golden_inputs import golden_err, sample_idx

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 512         # samples per compacted tensor


def load_case():
    g = np.load(os.path.join(GOLD, "bert_l272.npz"))
    V, L, d, H, nl, inner = [int(x) for x in g["cfg"]]
    cfg = bo.Cfg(V, L, d, H, nl, inner)
    P = bo.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:   # same perturbation as tools/gen_golden_wide.py:gen_bert
        if k.endswith("head_classifier.bias") or k == "mask_bias" or (k.endswith(".bias") and "layer_norm" not in k):
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


def entries(a, g, key):
    """(got, want) on the entries the fixture stores: the whole tensor, or the compacted fixture's strided samples."""
    a = np.asarray(a, np.float64)
    if key in g.files:
        return a, np.asarray(g[key], np.float64)
    t = a.reshape(-1)
    return t[sample_idx(t.size, K)], np.asarray(g[key + "@sample"], np.float64)


@pytest.fixture(scope="module")
def run():
    """One forward, one loss / gradient pass and three training steps of the oracle, shared by the tests below."""
    g, cfg, P = load_case()
    lam1, lam2 = list(g["lambda1"]), list(g["lambda2"])
    fwd = bo.forward(P, cfg, g["src"], g["dec"], training=False)
    pred = bo.predict(P, cfg, g["src"], g["cand"])
    lg = bo.loss_and_grads(P, cfg, g["src"], g["dec"], g["labels"], lam1, lam2, training=True, seed=0)
    state, Pw, steps = {}, {k: v.copy() for k, v in P.items()}, []
    for step in range(3):
        _, tn = bo.train_step(Pw, cfg, state, g["src"], g["dec"], g["labels"], lam1, lam2, lr=float(g["lr"]), weight_decay=float(g["wd"]),
                              clip=float(g["clip"]), training=True, seed=0)
        steps.append((tn, {k: v.copy() for k, v in Pw.items()}))
    return g, cfg, P, fwd, pred, lg, steps


def test_fixture_shape(run):
    g, cfg = run[0], run[1]
    assert (cfg.item_num, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.inner_units) == (40, 272, 64, 2, 1, 96)
    assert g["src"].shape == (2, 272)
    assert int((g["dec"][0] > 0).sum()) > 224 and int((g["dec"][1] == 0).sum()) > 224 and g["src"][1, -1] > 0
    assert "w1.mask_bias" in g.files and "w3.mask_bias" in g.files
    assert os.path.getsize(os.path.join(GOLD, "bert_l272.npz")) < 300 * 1024


def test_forward_and_predict_match_reference(run):
    g, cfg, P, (logits, enc_in, dec_out, rec), pred, _, _ = run
    figs = {"logits": golden_err(logits, g, "logits", K), "enc_in_0": golden_err(enc_in[0], g, "enc_in_0", K),
            "dec_out_0": golden_err(dec_out[0], g, "dec_out_0", K), "rec_0": golden_err(rec[0], g, "rec_0", K),
            "predict": golden_err(pred, g, "predict", K)}
    print(figs)
    for k, e in figs.items():
        assert e < 2e-5, (k, e)


def test_loss_and_gradients_match_reference(run):
    g, cfg, P, _, _, (loss, parts, G), steps = run
    assert abs(loss - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    assert abs(steps[0][0] - float(g["grad_norm"])) < 2e-5 * float(g["grad_norm"])
    figs = {k: golden_err(G[k], g, "grad." + k, K) for k in P}
    print("largest gradient error", max(figs.values()))
    for k, e in figs.items():
        assert e < 5e-5, (k, e)


def test_weights_after_the_recorded_steps_match_reference(run):
    """tests/test_oracle_wide.py:_adam_close on the stored entries: after the first step entries with |g| > 1e-6 within 0.02 lr and all
    within lr; after the third all within 0.3 lr."""
    g, cfg, P, _, _, _, steps = run
    lr = float(g["lr"])
    for k in P:
        got, want = entries(steps[0][1][k], g, "w1." + k)
        gref = entries(np.zeros(P[k].shape), g, "grad." + k)[1]
        diff = np.abs(got - want)
        big = np.abs(gref) > 1e-6
        assert (diff[big].max() if big.any() else 0.0) < 0.02 * lr, (k, diff[big].max() / lr)
        assert diff.max() < lr, k
        got, want = entries(steps[2][1][k], g, "w3." + k)
        assert np.abs(got - want).max() < 0.3 * lr, (k, np.abs(got - want).max() / lr)


def test_fused_head_flag_parses():
    from adt_amd.bert4rec.main import parse_args
    assert parse_args([]).fused_head is False and parse_args(["--fused_head"]).fused_head is True
