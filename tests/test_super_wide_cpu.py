"""The wide SASRec-ADT supernet fixtures (tests/golden/super_d256h1 / d256h2 / d128h1.npz, recorded from the imported reference by
tools/gen_golden_super.py wide, compacted) are reproduced by the numpy restatement oracle/super_oracle.py: forward under both block
choices, predict, the warm-up loss and every gradient, and the weights after one and two Adam steps -- all within fp64-vs-fp32
rounding.  The check that the fixtures and the oracle agree before any GPU sees them."""
import os

import numpy as np
import pytest

from oracle import super_oracle as su
from tools.gen_golden_inputs import golden_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 96
TAGS = ["d256h1", "d256h2", "d128h1"]


def load_case(tag):
    g = np.load(os.path.join(GOLD, "super_%s.npz" % tag))
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    cfg = su.Cfg(V, L, d, H, nl, g["rec_choice"], g["ind_choice"])
    return g, cfg, su.init_params(cfg, int(g["seed"]))


def has(g, key):
    return key in g.files or key + "@sample" in g.files


def weights_close(got, g, key, lr, nsteps):
    """Post-step weights in units of lr (oracle_wide._adam_close): entries whose gradient is rounding noise move by a rounding-dependent
    fraction of lr per step; most entries must agree far closer."""
    t = np.asarray(got, np.float64).reshape(-1)
    if key in g.files:
        want, s = np.asarray(g[key], np.float64).reshape(-1), t
    else:
        from tools.gen_golden_inputs import sample_idx
        want, s = np.asarray(g[key + "@sample"], np.float64), t[sample_idx(t.size, K)]
        norm = float(g[key + "@norm"])
        assert abs(np.sqrt((t ** 2).sum()) - norm) < 1e-4 * norm, key
    diff = np.abs(s - want)
    assert diff.max() < 1.01 * nsteps * lr, "%s: %.3g lr" % (key, diff.max() / lr)
    assert np.median(diff) < 0.05 * lr, "%s: median %.3g lr" % (key, np.median(diff) / lr)


def rec_close(a, b, H, tol):
    a, b = np.asarray(a, np.float64).reshape(-1, H * H), np.asarray(b, np.float64).reshape(-1, H * H)
    a, b = a[np.lexsort(a.T)], b[np.lexsort(b.T)]      # reference rows are permuted (sasrec/modules.py:518)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6) < tol


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_reproduces_wide_super_fixtures(tag):
    g, cfg, P = load_case(tag)
    cand, cand2 = [float(x) for x in g["cand"]], [float(x) for x in g["cand2"]]
    block = su.cand_to_block(cfg, cand)[0]
    shared = su.get_shared(cfg, block)
    assert [list(s[0]) for s in shared] == g["shared_idx"].tolist()
    pl, nl, ei, do, rc = su.forward(P, cfg, block, g["seq"], g["dec"], g["pos"], g["neg"])
    assert golden_err(pl, g, "pos_logits", K) < 2e-5 and golden_err(nl, g, "neg_logits", K) < 2e-5
    for i in range(cfg.num_layers):
        assert golden_err(ei[i], g, "enc_in_%d" % i, K) < 2e-5 and golden_err(do[i], g, "dec_out_%d" % i, K) < 2e-5
        assert rec_close(rc[i], g["rec_%d" % i], cfg.num_heads, 2e-5)
    assert golden_err(su.predict(P, cfg, block, g["seq"], g["items"]), g, "predict", K) < 2e-5
    block2 = su.cand_to_block(cfg, cand2)[0]
    pl2, nl2 = su.forward(P, cfg, block2, g["seq"], g["dec"], g["pos"], g["neg"])[:2]
    assert golden_err(pl2, g, "pos_logits2", K) < 2e-5 and golden_err(nl2, g, "neg_logits2", K) < 2e-5
    assert golden_err(su.predict(P, cfg, block2, g["seq"], g["items"]), g, "predict2", K) < 2e-5
    loss, G = su.loss_and_grads(P, cfg, cand, g["seq"], g["dec"], g["pos"], g["neg"], training=True, seed=0)
    assert abs(loss - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    none = set(str(x) for x in g["grad_none"])
    assert set(k for k in P if G[k] is None) == none
    for k in P:
        if G[k] is not None:
            assert golden_err(G[k], g, "grad." + k, K) < 1e-4, k
    state = {}
    Pw = {k: v.copy() for k, v in P.items()}
    lr = float(g["lr"])
    for step in (1, 2):
        _, tn = su.train_step(Pw, cfg, state, cand, g["seq"], g["dec"], g["pos"], g["neg"], lr=lr, weight_decay=float(g["wd"]),
                              clip=float(g["clip"]), training=True, seed=0)
        if step == 1:
            assert abs(tn - float(g["grad_norm"])) < 2e-5 * float(g["grad_norm"])
        keys = sorted({f.split("@")[0][3:] for f in g.files if f.startswith("w%d." % step)})
        assert len(keys) > 10
        for k in keys:
            weights_close(Pw[k], g, "w%d.%s" % (step, k), lr, step)
    for k in none:
        assert np.array_equal(Pw[k], P[k])
