"""CPU: the supernet fixtures at the padded widths and past the resident attention's length (tests/golden/super_w50h1 / w100h2 / l272.npz,
tools/gen_golden_super.py lanes) are reproduced by oracle/super_oracle.py at the bounds of tests/test_super_wide_cpu.py, and the padded
tables of the three supernets map every reference element to a distinct live lane, in ascending order, with each
candidate layer contiguous in both layouts -- what lets a warm-up step copy only the ranges it trains.  The BERT4Rec-ADT / STOSA-ADT numpy
oracles restate the plain models, not their supernets: those fixtures are checked against the reference on the GPU only."""
import os

import numpy as np
import pytest

from oracle import super_oracle as su
from tools.gen_golden_inputs import golden_err, sample_idx

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 96
TAGS = ["w50h1", "w100h2", "l272"]


def load_case(tag):
    g = np.load(os.path.join(GOLD, "super_%s.npz" % tag))
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    cfg = su.Cfg(V, L, d, H, nl, g["rec_choice"], g["ind_choice"])
    return g, cfg, su.init_params(cfg, int(g["seed"]))


def weights_close(got, g, key, lr, nsteps):
    """tests/test_super_wide_cpu.py: post-step weights in units of lr."""
    t = np.asarray(got, np.float64).reshape(-1)
    if key in g.files:
        want, s = np.asarray(g[key], np.float64).reshape(-1), t
    else:
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
def test_oracle_reproduces_lane_super_fixtures(tag):
    g, cfg, P = load_case(tag)
    cand, cand2 = [float(x) for x in g["cand"]], [float(x) for x in g["cand2"]]
    block = su.cand_to_block(cfg, cand)[0]
    assert [list(s[0]) for s in su.get_shared(cfg, block)] == g["shared_idx"].tolist()
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


# ---- the padded tables ---------------------------------------------------------------------------------------------------------------
def _offsets(table):
    off, out = 0, {}
    for name, shape in table:
        out[name] = off
        off += (int(np.prod(shape)) + 3) // 4 * 4
    return out, off


def _tables(kind, d, H, nl, block):
    """(ref_table, padded table, prefix, candidate-layer name prefixes)."""
    from adt_amd.wide import padded_layout
    _, _, dp = padded_layout(d, H)
    if kind == "sasrec":
        from adt_amd.sasrec.supersasrec import param_table
        ref, pad, prefix = param_table(30, 12, d, H, nl, block), param_table(30, 12, dp, H, nl, block), ()
        layers = ["%s.%s_layers.%d.%d." % (k, k, i, c) for k in ("encoder", "decoder") for i in range(nl) for c in range(block)]
    elif kind == "bert":
        from adt_amd.bert4rec.model import padded_tables
        ref, pad, prefix = padded_tables(30, 12, d, H, nl, 4 * d, 2, 32, block)
        layers = ["%s.%s_layers.%d.%d." % (k, k, i, c) for k in ("encoder", "decoder") for i in range(nl) for c in range(block)]
    else:
        from adt_amd.stosa.models import padded_tables
        ref, pad, prefix, _ = padded_tables(42, 12, d, H, nl, 3, False, block)
        layers = ["item_%s.layer.%d.%d." % (k, i, c) for k in ("encoder", "decoder") for i in range(nl) for c in range(block)]
    return ref, pad, prefix, layers


@pytest.mark.parametrize("kind", ["sasrec", "bert", "stosa"])
@pytest.mark.parametrize("d,H", [(50, 1), (100, 2), (48, 4), (100, 1)])
def test_padded_supernet_tables(kind, d, H):
    from adt_amd.wide import lane_index, padded_layout
    hd, hd_pad, dp = padded_layout(d, H)
    nl, block = 2, 4
    ref, pad, prefix, layers = _tables(kind, d, H, nl, block)
    assert [n for n, _ in ref] == [n for n, _ in pad]
    assert any(n.startswith(layers[-1]) for n, _ in ref) and len(ref) == len(dict(ref))
    off, n_flat = _offsets(pad)
    idx = lane_index(ref, pad, off, d, H, prefix=prefix).astype(np.int64)
    n_ref = sum(int(np.prod(s)) for _, s in ref)
    assert idx.size == n_ref and idx.min() >= 0 and idx.max() < n_flat
    assert np.all(np.diff(idx) > 0)            # distinct, and ascending: a padded range holds one contiguous run of reference elements
    # every element lands inside its own tensor, on a live lane of every padded axis
    pshape, o = dict(pad), 0
    for name, shape in ref:
        n = int(np.prod(shape))
        local = idx[o:o + n] - off[name]
        assert local.min() >= 0 and local.max() < int(np.prod(pshape[name])), name
        coords = np.unravel_index(local, pshape[name])
        for ax, (r, q) in enumerate(zip(shape, pshape[name])):
            c = coords[ax]
            if r == q:
                continue
            if (name, ax) in prefix or q == hd_pad and r == hd:
                assert c.max() < r, (name, ax)                      # a zero-filled tail: element j stays at j
            else:
                assert ((c % hd_pad) < hd).all(), (name, ax)        # head h at [h * hd_pad, h * hd_pad + hd)
        o += n
    # candidate layers: contiguous in both layouts, in the same order, nothing between two layers of a stack
    ref_off, o = {}, 0
    for name, shape in ref:
        ref_off[name] = o
        o += int(np.prod(shape))
    if kind == "stosa":      # a decoder layer's dec_attention lives in the untrained tail: the trained part is what a step copies
        member = lambda n, p: n.startswith(p) and ".dec_attention." not in n
    else:
        member = lambda n, p: n.startswith(p)
    for p in layers:
        names = [n for n, _ in ref if member(n, p)]
        pos = [i for i, (n, _) in enumerate(ref) if member(n, p)]
        assert pos == list(range(pos[0], pos[0] + len(pos))), p
        lo, hi = off[names[0]], off[names[-1]] + (int(np.prod(pshape[names[-1]])) + 3) // 4 * 4
        r0, r1 = int(np.searchsorted(idx, lo)), int(np.searchsorted(idx, hi))
        assert r0 == ref_off[names[0]] and r1 == ref_off[names[-1]] + int(np.prod(dict(ref)[names[-1]])), p
