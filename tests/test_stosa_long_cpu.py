"""CPU: oracle/stosa_oracle.py reproduces the two L = 272 fixtures recorded from the imported reference (tools/gen_golden_stosa.py:main_long;
tests/golden/stosa_l272.npz, stosa_kl_l272.npz: d 64, one head, one layer, B 2, row 1 with a padded prefix of 72 positions), at the bounds
tests/test_oracle_wide.py uses for the STOSA fixtures: outputs, full-sort distances and the loss 2e-5, gradients 1e-4 (its bound for whole
tensors; 2e-4 is what it allows compacted ones).  The KL fixture runs the oracle with the reference's kl_distance / kl_distance_matmul
(stosa/modules.py:45-70) swapped in on oracle/tape.py variables, as tests/test_stosa_kl_hip.py does."""
import contextlib
import os

import numpy as np
import pytest

from oracle import stosa_oracle as so, tape as tp
from tools.gen_golden_inputs import golden_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(metric):
    g = np.load(os.path.join(GOLD, ("stosa_kl_l272.npz" if metric == "kl" else "stosa_l272.npz")))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:   # same perturbation as tools/gen_golden_stosa.py:reference_model
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


def _recip(a):
    r = (np.float32(1) / a.v).astype(np.float32)
    out = tp.Var(r, (a,))
    out.vjp = lambda gr: a.acc(-gr * r * r)
    return out


def _tpose(x):
    return tp.transpose(x, tuple(range(x.v.ndim - 2)) + (x.v.ndim - 1, x.v.ndim - 2))


def tape_kl_distance(m1, c1, m2, c2):
    """stosa/modules.py:45-50 on oracle/tape.py variables (log(prod) as sum(log))."""
    ic2 = _recip(c2)
    df = tp.sub(m2, m1)
    s = tp.add(tp.sum_(tp.mul(c1, ic2), axis=-1), tp.sum_(tp.mul(tp.mul(df, ic2), df), axis=-1))
    det = tp.sub(tp.sum_(tp.log(c2), axis=-1), tp.sum_(tp.log(c1), axis=-1))
    return tp.scale(tp.add(tp.add_const(s, -float(m1.v.shape[1])), det), 0.5)


def tape_kl_distance_matmul(m1, c1, m2, c2):
    """stosa/modules.py:52-70 on oracle/tape.py variables."""
    ic2 = _recip(c2)
    logdet = tp.sub(_tpose(tp.sum_(tp.log(c2), axis=-1, keepdims=True)), tp.sum_(tp.log(c1), axis=-1, keepdims=True))
    mean = tp.matmul(tp.square(tp.sub(m1, m2)), _tpose(ic2))
    trace = tp.matmul(ic2, _tpose(c1))
    return tp.scale(tp.add_const(tp.add(tp.add(logdet, mean), trace), -float(m1.v.shape[-1])), 0.5)


@contextlib.contextmanager
def oracle_for(metric):
    """oracle.stosa_oracle, with its two distance functions replaced for the duration of the call under KL (the module is not edited)."""
    saved = so.wasserstein_distance, so.wasserstein_distance_matmul
    if metric == "kl":
        so.wasserstein_distance, so.wasserstein_distance_matmul = tape_kl_distance, tape_kl_distance_matmul
    try:
        yield so
    finally:
        so.wasserstein_distance, so.wasserstein_distance_matmul = saved


def kl_predict_full(sm, sc, Em, Ec):
    """kl_predict_full (stosa/trainer.py:481-511): the items padded to a multiple of E = len(sm) and scored in chunks of E by
    kl_distance_matmul, whose (m1 - m2) is elementwise over the chunk."""
    E, V, d = sm.shape[0], Em.shape[0], Em.shape[1]
    pad = E - V % E
    cm = np.concatenate((Em, np.zeros((pad, d), np.float32)))
    cc = np.concatenate((np.where(Ec > 0, Ec, np.exp(np.minimum(Ec, 0)) - 1) + 1, np.ones((pad, d), np.float32))).astype(np.float32)
    out = [tape_kl_distance_matmul(tp.const(sm), tp.const(sc), tp.const(cm[s0:s0 + E]), tp.const(cc[s0:s0 + E])).v for s0 in range(0, len(cm), E)]
    return np.concatenate(out, 1)[:, :V]


@pytest.fixture(scope="module", params=["wasserstein", "kl"])
def run(request):
    """One forward and one loss / gradient pass of the oracle per metric, shared by the tests below."""
    metric = request.param
    g, cfg, P = load_case(metric)
    lam1, lam2 = list(g["lambda1"]), list(g["lambda2"])
    with oracle_for(metric):
        fin = so.finetune(P, cfg, g["input_ids"], g["dec_ids"], training=False)
        if metric == "kl":
            full = kl_predict_full(fin[0][:, -1, :], fin[1][:, -1, :], P["item_mean_embeddings.weight"], P["item_cov_embeddings.weight"])
        else:
            full = so.predict_full(P, cfg, g["input_ids"], g["dec_ids"])
        lg = so.loss_and_grads(P, cfg, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, training=True, seed=0)
    return metric, g, cfg, P, fin, full, lg


def test_fixture_shape(run):
    metric, g, cfg, P, _, _, _ = run
    assert (cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers) == (272, 64, 1, 1) and g["input_ids"].shape == (2, 272)
    assert (g["input_ids"][0] > 0).all() and int((g["input_ids"][1] == 0).sum()) >= 40 and g["input_ids"][1, -1] > 0
    assert os.path.getsize(os.path.join(GOLD, "stosa_kl_l272.npz" if metric == "kl" else "stosa_l272.npz")) < 300 * 1024


def test_finetune_and_full_sort_match_reference(run):
    metric, g, cfg, P, (m, c, enc_in, enc_rec, dec_out), full, _ = run
    figs = {"mean_out": golden_err(m, g, "mean_out"), "cov_out": golden_err(c, g, "cov_out"),
            "enc_in_mean_0": golden_err(enc_in[0][0], g, "enc_in_mean_0"), "enc_in_cov_0": golden_err(enc_in[0][1], g, "enc_in_cov_0"),
            "rec_mean_0": golden_err(enc_rec[0][0], g, "rec_mean_0"), "rec_cov_0": golden_err(enc_rec[0][1], g, "rec_cov_0"),
            "dec_out_mean_0": golden_err(dec_out[0][0], g, "dec_out_mean_0"), "dec_out_cov_0": golden_err(dec_out[0][1], g, "dec_out_cov_0"),
            "full_dist": golden_err(full, g, "full_dist")}
    print(metric, figs)
    for k, e in figs.items():
        assert e < 2e-5, (k, e)


def test_loss_and_gradients_match_reference(run):
    metric, g, cfg, P, _, _, (loss, parts, G) = run
    assert abs(loss - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    assert abs(parts["bpr"] - float(g["bpr"])) < 2e-5 * abs(float(g["bpr"])) and abs(parts["auc"] - float(g["auc"])) < 1e-6
    assert abs(parts["pvn"] - float(g["pvn"])) < 2e-5 * max(abs(float(g["pvn"])), 1e-6)
    assert sorted(k for k in P if G[k] is None) == sorted(str(x) for x in g["grad_none"])
    figs = {k: golden_err(G[k], g, "grad." + k) for k in P if G[k] is not None}
    print(metric, "largest gradient error", max(figs.values()))
    for k, e in figs.items():
        assert e < 1e-4, (k, e)
