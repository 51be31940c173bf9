"""CPU: STOSA-ADT under distance_metric='kl' at widths the kernels pad -- the numpy oracle with the KL distances
swapped in (tests/test_stosa_kl_hip.py:kl_oracle) against the three fixtures recorded from the reference
(tests/golden/stosa_kl_{w50_h1,w100_h2,w48_h4}.npz; tools/gen_golden_stosa.py --metric stosa_kl_odd, compacted: 320 samples per large
tensor), with the bounds of tests/test_stosa_oddwidth_cpu.py; and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

from oracle import stosa_oracle as so
from tests.test_stosa_kl_hip import kl_full_ref, kl_oracle
from tests.test_stosa_oddwidth_cpu import K, stored
from tools.gen_golden_inputs import golden_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ["w50_h1", "w100_h2", "w48_h4"]


def load_case(tag):
    g = np.load(os.path.join(GOLD, "stosa_kl_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:   # same perturbation as tools/gen_golden_stosa.py:gen_stosa
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_shapes_are_small_and_left_padded(tag):
    g, cfg, _ = load_case(tag)
    B, L = g["input_ids"].shape
    assert L <= 20 and B <= 4 and cfg.hidden_units % 64 != 0
    assert (g["input_ids"][:, 0] == 0).any() and (g["input_ids"][0] > 0).all()          # a left-padded row, and the full one
    assert os.path.getsize(os.path.join(GOLD, "stosa_kl_%s.npz" % tag)) < (1 << 20)


@pytest.mark.parametrize("tag", TAGS)
def test_kl_oracle_finetune_matches_reference(tag):
    g, cfg, P = load_case(tag)
    with kl_oracle():
        m, c, enc_in, enc_rec, dec_out = so.finetune(P, cfg, g["input_ids"], g["dec_ids"], training=False)
    # kl_predict_full pads the item table to a multiple of the batch and chunks it (tests/test_stosa_kl_hip.py:kl_full_ref, float64): the
    # oracle's predict_full is one matmul over all items, which the KL broadcasts do not take; its last states are the oracle's
    full = kl_full_ref(m[:, -1, :], c[:, -1, :], P["item_mean_embeddings.weight"], P["item_cov_embeddings.weight"])
    figs = {"mean_out": golden_err(m, g, "mean_out", K), "cov_out": golden_err(c, g, "cov_out", K)}
    for i in range(cfg.num_layers):
        for nm, pair in (("enc_in", enc_in[i]), ("rec", enc_rec[i]), ("dec_out", dec_out[i])):
            figs["%s_mean_%d" % (nm, i)] = golden_err(pair[0], g, "%s_mean_%d" % (nm, i), K)
            figs["%s_cov_%d" % (nm, i)] = golden_err(pair[1], g, "%s_cov_%d" % (nm, i), K)
    figs["full_dist"] = golden_err(full, g, "full_dist", K)
    print(tag, figs)
    for k, e in figs.items():
        assert e < 2e-5, (k, e)


@pytest.mark.parametrize("tag", TAGS)
def test_kl_oracle_train_steps_match_reference(tag):
    g, cfg, P = load_case(tag)
    lam1, lam2, lr = list(g["lambda1"]), list(g["lambda2"]), float(g["lr"])
    with kl_oracle():
        loss, parts, G = so.loss_and_grads(P, cfg, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, training=True, seed=0)
    print(tag, "loss rel err %.3g" % (abs(loss - float(g["loss"])) / abs(float(g["loss"]))))
    assert abs(loss - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    assert abs(parts["bpr"] - float(g["bpr"])) < 2e-5 * abs(float(g["bpr"])) and abs(parts["auc"] - float(g["auc"])) < 1e-6
    assert abs(parts["pvn"] - float(g["pvn"])) < 2e-5 * max(abs(float(g["pvn"])), 1e-6)
    assert sorted(k for k in P if G[k] is None) == sorted(str(x) for x in g["grad_none"])
    assert sorted(k for k in P if G[k] is None) == sorted(k for k in P if so.is_unused(k))
    worst = 0.0
    for k in P:
        if G[k] is not None:
            e = golden_err(G[k], g, "grad." + k, K)
            worst = max(worst, e)
            assert e < 1e-4, (k, e)
    print(tag, "worst gradient err %.3g" % worst)
    state = {}
    Pw = {k: v.copy() for k, v in P.items()}
    for step in range(3):
        with kl_oracle():
            so.train_step(Pw, cfg, state, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, lr=lr, training=True, seed=0)
        if step not in (0, 2):
            continue
        for k in P:
            got, want = stored(g, "w%d." % (step + 1) + k, Pw[k])
            diff = np.abs(got - want)
            if step == 0 and G[k] is not None:          # tests/test_stosa_oddwidth_cpu.py, first step
                big = np.abs(stored(g, "grad." + k, G[k])[1]) > 1e-6
                assert (diff[big].max() if big.any() else 0.0) < 0.02 * lr, k
                assert diff.max() < lr, k
            else:
                assert diff.max() < 0.3 * lr, k


def test_new_entry_points_are_declared_and_bound():
    """The nine new symbols stand in include/adt_hip.h and in _lib.SIGNATURES with the argument counts of their Wasserstein counterparts."""
    from adt_amd import _lib
    text = open(os.path.join(ROOT, "include", "adt_hip.h")).read()
    for kl, w in (("adt_klattn_scaled_fwd", "adt_wattn_scaled_fwd"), ("adt_klattn_scaled_bwd", "adt_wattn_scaled_bwd"),
                  ("adt_klattn_mfma_scaled_fwd", "adt_wattn_mfma_scaled_fwd"), ("adt_klattn_mfma_scaled_bwd", "adt_wattn_mfma_scaled_bwd"),
                  ("adt_klattn_long_scaled_fwd", "adt_wattn_long_scaled_fwd"), ("adt_klattn_long_scaled_bwd", "adt_wattn_long_scaled_bwd"),
                  ("adt_kldist_bpr_lanes", "adt_wdist_bpr_lanes"), ("adt_kldist_full_lanes", "adt_wdist_full_lanes")):
        assert re.search(r"\bint %s\(" % kl, text), kl
        assert _lib.SIGNATURES[kl] == _lib.SIGNATURES[w], kl
    assert re.search(r"\bint adt_klrow_pack_lanes\(", text)
    assert len(_lib.SIGNATURES["adt_klrow_pack_lanes"][1]) == len(_lib.SIGNATURES["adt_klrow_pack"][1]) + 2          # d -> H, hd, hd_pad


def test_main_passes_the_flag_and_the_constructor_documents_it():
    import inspect
    from adt_amd.stosa import main as stosa_main
    from adt_amd.stosa.models import DisenDistSAModel
    sig = inspect.signature(DisenDistSAModel.__init__)
    assert sig.parameters["allow_kl_lanes"].default is False
    assert list(sig.parameters)[:4] == ["self", "args", "block", "dec_layernorm"]
    assert "allow_kl_lanes=True" in inspect.getsource(stosa_main.main)
