"""CPU: STOSA-ADT at widths the kernels pad -- the numpy oracle against the four odd-width fixtures recorded from
the reference (tests/golden/stosa_{w50_h1,w100_h2,w48_h4,w150_h3}.npz, compacted: 320 samples per large tensor), with the bounds
tests/test_oracle_wide.py uses for the STOSA fixtures; the reference-shaped <-> padded index map of the STOSA parameter table; and the
shapes padded_layout refuses."""
import os

import numpy as np
import pytest

from oracle import stosa_oracle as so
from tools.gen_golden_inputs import golden_err, sample_idx

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ["w50_h1", "w100_h2", "w48_h4", "w150_h3"]
K = 320          # samples per compacted tensor (tools/gen_golden_stosa.py:STOSA_ODD_COMPACT)


def load_case(tag):
    g = np.load(os.path.join(GOLD, "stosa_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:   # same perturbation as tools/gen_golden_stosa.py:gen_stosa
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


def stored(g, key, got):
    """(got, want) on the entries the fixture stores for `key`: all of them, or the strided samples of a compacted tensor."""
    got = np.asarray(got, np.float64)
    if key in g.files:
        return got.reshape(-1), np.asarray(g[key], np.float64).reshape(-1)
    return got.reshape(-1)[sample_idx(got.size, K)], np.asarray(g[key + "@sample"], np.float64)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_shapes_are_small_and_left_padded(tag):
    g, cfg, _ = load_case(tag)
    B, L = g["input_ids"].shape
    assert cfg.item_size <= 42 and L <= 20 and B <= 4 and cfg.num_layers in (1, 2)
    assert (g["input_ids"][:, 0] == 0).any() and (g["input_ids"][0] > 0).all()          # a left-padded row, and the full one
    assert os.path.getsize(os.path.join(GOLD, "stosa_%s.npz" % tag)) < (1 << 20)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_finetune_matches_reference(tag):
    g, cfg, P = load_case(tag)
    m, c, enc_in, enc_rec, dec_out = so.finetune(P, cfg, g["input_ids"], g["dec_ids"], training=False)
    figs = {"mean_out": golden_err(m, g, "mean_out", K), "cov_out": golden_err(c, g, "cov_out", K)}
    for i in range(cfg.num_layers):
        for nm, pair in (("enc_in", enc_in[i]), ("rec", enc_rec[i]), ("dec_out", dec_out[i])):
            figs["%s_mean_%d" % (nm, i)] = golden_err(pair[0], g, "%s_mean_%d" % (nm, i), K)
            figs["%s_cov_%d" % (nm, i)] = golden_err(pair[1], g, "%s_cov_%d" % (nm, i), K)
    figs["full_dist"] = golden_err(so.predict_full(P, cfg, g["input_ids"], g["dec_ids"]), g, "full_dist", K)
    print(tag, figs)
    for k, e in figs.items():
        assert e < 2e-5, (k, e)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_train_steps_match_reference(tag):
    g, cfg, P = load_case(tag)
    lam1, lam2, lr = list(g["lambda1"]), list(g["lambda2"]), float(g["lr"])
    loss, parts, G = so.loss_and_grads(P, cfg, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, training=True, seed=0)
    assert abs(loss - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    assert abs(parts["bpr"] - float(g["bpr"])) < 2e-5 * abs(float(g["bpr"])) and abs(parts["auc"] - float(g["auc"])) < 1e-6
    assert abs(parts["pvn"] - float(g["pvn"])) < 2e-5 * max(abs(float(g["pvn"])), 1e-6)
    assert sorted(k for k in P if G[k] is None) == sorted(str(x) for x in g["grad_none"])
    for k in P:
        if G[k] is not None:
            assert golden_err(G[k], g, "grad." + k, K) < 1e-4, k
    state = {}
    Pw = {k: v.copy() for k, v in P.items()}
    for step in range(3):
        so.train_step(Pw, cfg, state, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, lr=lr, training=True, seed=0)
        if step not in (0, 2):
            continue
        for k in P:
            got, want = stored(g, "w%d." % (step + 1) + k, Pw[k])
            diff = np.abs(got - want)
            if step == 0 and G[k] is not None:          # tests/test_oracle_wide.py:_adam_close, first step
                big = np.abs(stored(g, "grad." + k, G[k])[1]) > 1e-6
                assert (diff[big].max() if big.any() else 0.0) < 0.02 * lr, k
                assert diff.max() < lr, k
            else:
                assert diff.max() < 0.3 * lr, k


@pytest.mark.parametrize("d,H", [(50, 1), (100, 2), (48, 4)])
def test_lane_index_of_the_stosa_table(d, H):
    """Every reference element has its own place in the padded flat buffer, on a live lane; the (4d, d) / (d, 4d) intermediates keep
    their 4d inner channels as a zero-tailed prefix of 4 * d_pad; the head classifiers pad (H, hd) to (H, hd_pad)."""
    from adt_amd.stosa.models import padded_tables, param_table
    from adt_amd.wide import lane_index, padded_layout
    hd, hd_pad, dp = padded_layout(d, H)
    nl, V, L, nu = 2, 42, 12, 4
    ref, pad, prefix, n_trained = padded_tables(V, L, d, H, nl, nu)
    assert ref == param_table(V, L, d, H, nl, nu)[0] and [n for n, _ in ref] == [n for n, _ in pad]
    off, o = {}, 0
    for n, s in pad:
        off[n] = o
        o += (int(np.prod(s)) + 3) // 4 * 4
    idx = lane_index(ref, pad, off, d, H, prefix=prefix)
    assert idx.size == sum(int(np.prod(s)) for _, s in ref) and np.unique(idx).size == idx.size and 0 <= idx.min() and idx.max() < o
    chan = (np.arange(d) // hd) * hd_pad + np.arange(d) % hd
    pos = 0
    pshape = dict(pad)
    for name, shape in ref:
        n = int(np.prod(shape))
        local = (idx[pos:pos + n] - off[name]).reshape(shape)
        pos += n
        q = pshape[name]
        assert local.max() < int(np.prod(q)), name
        coords = np.unravel_index(local, q)
        if name.endswith(".dense_1.weight"):
            assert q == (4 * dp, dp) and np.array_equal(coords[0], np.arange(4 * d)[:, None].repeat(d, 1)) and np.array_equal(coords[1][0], chan)
        elif name.endswith(".dense_1.bias"):
            assert q == (4 * dp,) and np.array_equal(coords[0], np.arange(4 * d))
        elif name.endswith(".dense_2.weight"):
            assert q == (dp, 4 * dp) and np.array_equal(coords[1], np.arange(4 * d)[None, :].repeat(d, 0)) and np.array_equal(coords[0][:, 0], chan)
        elif name.endswith("_independence_layer.weight"):
            assert q == (H, hd_pad) and np.array_equal(coords[1], np.arange(hd)[None, :].repeat(H, 0))
        elif "_embeddings." in name:
            assert q == (shape[0], dp) and np.array_equal(coords[1][0], chan) and np.array_equal(coords[0][:, 0], np.arange(shape[0]))
        elif shape == (d, d):
            assert q == (dp, dp) and np.array_equal(coords[0][:, 0], chan) and np.array_equal(coords[1][0], chan)
        elif shape == (d,):
            assert q == (dp,) and np.array_equal(coords[0], chan)
        else:
            assert q == shape, name          # user_margins, the head classifiers' biases
        for ax, size in enumerate(q):        # live lanes only: a dimension of size d_pad is only ever hit at a live column
            if size == dp and shape[ax] == d:
                assert ((coords[ax] % hd_pad) < hd).all(), (name, ax)


def test_shapes_the_padded_layout_refuses():
    from adt_amd._lib import AdtError
    from adt_amd.wide import padded_layout
    assert padded_layout(50, 1) == (50, 64, 64) and padded_layout(100, 2) == (50, 64, 128) and padded_layout(48, 4) == (12, 16, 64)
    assert padded_layout(150, 3) == (50, 64, 192)
    for d, H, why in ((50, 3, "multiple"), (300, 1, "exceeds"), (50, 5, "not supported"), (330, 5, "not supported"), (20, 2, "not supported")):
        with pytest.raises(AdtError, match=why):          # 50 / 3 no integer head; head 300 > 256; 5 x 16 = 80, 5 x 128 = 640, 2 x 16 = 32
            padded_layout(d, H)
