"""GPU: BERT4Rec-ADT at widths the kernels pad -- hidden_units 50 (one head: 64 lanes; two heads of 25: 2 x 32), 100 (2 x 64), 150
(3 x 64 = 192) -- and at head sizes 128 / 256, on the HIP path (adt_amd/bert4rec/model.py, adt_amd/csrc/adt_lanes.cuh).

Reference parity against tests/golden/bert_{w50_h1,w50_h2,w100_h2,w150_h3,hd128,hd256}.npz with the tolerances of tests/test_bert_hip.py,
dropout-on parity against the numpy oracle (fused drop-residual-normalise and, with ADT_DRN_LANES=0, the two-pass form), the fused
kernels alone against float64 with the keep mask of oracle/rng.py, and the properties of the padded layout: pad lanes stay exactly zero,
checkpoints and parameters show the reference's shapes only."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import bert_oracle as bo, rng  # noqa: E402
from tools.gen_golden_inputs import golden_err, sample_idx  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
TAGS = ["w50_h1", "w50_h2", "w100_h2", "w150_h3", "hd128", "hd256"]
K = 320          # samples per compacted tensor (tools/gen_golden_wide.py:BERT_ODD_COMPACT)
DEV = "cuda:0"


class Args:
    pass


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


def close(a, b, tol, what):
    err = rel(a, b)
    print("%s: rel err %.3g (bound %.3g)" % (what, err, tol))
    assert err < tol, "%s: rel err %.3g" % (what, err)


def perturb(P, seed):
    """tools/gen_golden_wide.py:gen_bert: head classifier / mask bias / Linear biases away from their zero init."""
    r = np.random.RandomState(seed + 1)
    for k in P:
        if k.endswith("head_classifier.bias") or k == "mask_bias" or (k.endswith(".bias") and "layer_norm" not in k):
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return P


def load_case(tag):
    g = np.load(os.path.join(GOLD, "bert_%s.npz" % tag))
    V, L, d, H, nl, inner = [int(x) for x in g["cfg"]]
    cfg = bo.Cfg(V, L, d, H, nl, inner)
    return g, cfg, perturb(bo.init_params(cfg, int(g["seed"])), int(g["seed"]))


def make_case(d, H, nl, inner, V=40, L=12, B=3, seed=5, lens=None):
    """A seeded model and masked-item batch (left-padded; row 0 full), as the fixtures' generator draws them."""
    cfg = bo.Cfg(V, L, d, H, nl, inner)
    P = perturb(bo.init_params(cfg, seed), seed)
    r = np.random.RandomState(seed + 7)
    src, dec, lab = (np.zeros((B, L), np.int64) for _ in range(3))
    for b in range(B):
        n = (L if b == 0 else int(r.randint(2, L + 1))) if lens is None else lens[b]
        items = r.randint(1, V + 1, size=n)
        m = r.rand(n) < 0.3
        m[-1] = True
        dec[b, L - n:] = items
        src[b, L - n:] = np.where(m, V + 1, items)
        lab[b, L - n:] = np.where(m, items, 0)
    return cfg, P, src, dec, lab


def build(cfg, P, prec, dropout=0.0, attention_dropout=0.0, fused_head=None):
    from adt_amd.bert4rec.model import BertModel
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = DEV, cfg.maxlen, cfg.num_heads, cfg.num_layers, cfg.hidden_units, cfg.inner_units
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = dropout, attention_dropout, 2, prec
    if fused_head is not None:
        a.fused_head = fused_head
    m = BertModel(1, cfg.item_num, a)
    if P is not None:
        m.load_numpy(P)
    return m


def pad_mask(m):
    """True on every float of the flat layout that no reference element maps to (pad lanes and alignment gaps)."""
    mask = torch.ones(m.n_flat, dtype=torch.bool, device=m.dev)
    mask[m.lane_idx.long()] = False
    return mask


def grads_of(m, cfg, batch, lam1, lam2, b_offset=0, n_valid=None, B_global=None, seed=None):
    src, dec, lab = batch
    B, L = (len(src) if B_global is None else B_global), cfg.maxlen
    m.train()
    if seed is not None:
        m.set_seed(seed)
    st = m.stage(src, dec, lab, n_valid_global=n_valid)
    norms = torch.tensor([0.0, B * L * cfg.hidden_units, B * L * cfg.num_heads], device=DEV)       # the TRUE d
    slots = torch.zeros(1 + 2 * cfg.num_layers, 64, device=DEV)
    m.flat_grad.zero_()
    m.loss_forward_backward(st, lam1, lam2, norms, slots, b_offset=b_offset)
    torch.cuda.synchronize()
    return float((slots.sum(1).cpu().numpy() * np.array([1.0] + list(lam1) + list(lam2))).sum())


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_predict_match_reference(tag, prec):
    from adt_amd.wide import padded_layout
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    d, H = cfg.hidden_units, cfg.num_heads
    assert (m.lanes is not None) == (padded_layout(d, H)[2] != d) and m.hidden_units == d and m.dp == padded_layout(d, H)[2]
    m.eval()
    logits, enc_in, dec_out, rec = m(g["src"], g["dec"])
    B, L = g["src"].shape
    tol = 1e-4 if prec == "f32" else 3e-2
    figs = {"logits": golden_err(logits.cpu().numpy(), g, "logits", K)}
    for i in range(cfg.num_layers):
        assert tuple(enc_in[i].shape) == (B, L, d) and tuple(dec_out[i].shape) == (B, L, d) and tuple(rec[i].shape) == (B, L, H, H)
        figs["enc_in_%d" % i] = golden_err(enc_in[i].cpu().numpy(), g, "enc_in_%d" % i, K)
        figs["dec_out_%d" % i] = golden_err(dec_out[i].cpu().numpy(), g, "dec_out_%d" % i, K)
        figs["rec_%d" % i] = golden_err(rec[i].cpu().numpy(), g, "rec_%d" % i, K)
    figs["predict"] = golden_err(m.predict(None, g["src"], None, None, g["cand"]).cpu().numpy(), g, "predict", K)
    print(tag, prec, figs)
    for k, e in figs.items():
        assert e < tol, (k, e)
    sd = m.state_dict()          # state_dict names and shapes are the reference's
    assert set(sd) == set(P) and all(tuple(sd[k].shape) == P[k].shape for k in P)


def _stored(g, key, got):
    """(got, want) on the entries the fixture stores for `key`: all of them, or the strided samples of a compacted tensor."""
    got = np.asarray(got, np.float64)
    if key in g.files:
        return got.reshape(-1), np.asarray(g[key], np.float64).reshape(-1)
    return got.reshape(-1)[sample_idx(got.size, K)], np.asarray(g[key + "@sample"], np.float64)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_training_step_matches_reference(tag, prec):
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    grads_of(m, cfg, (g["src"], g["dec"], g["labels"]), lam1, lam2)
    none = [f[6:] for f in g.files if f.startswith("gnone.")]
    assert sorted(none) == (sorted(k for k in P if ".head_classifier." in k) if cfg.num_heads == 1 else [])
    gmax = max(float(np.abs(_stored(g, "grad." + k, np.zeros(P[k].shape))[1]).max()) for k in P if k not in none)
    figs = {}
    for k in P:
        got = m.GR(k).cpu().numpy()
        assert got.shape == P[k].shape, k          # the reference's shape
        if k in none:
            assert not np.any(got), k              # grad None in the reference: exactly zero here
        elif prec == "f32":
            figs[k] = golden_err(got, g, "grad." + k, K)
        elif "key_transfer.bias" in k:
            # softmax is invariant to a shift of all keys' scores: this gradient is 0 up to rounding in the reference too
            assert np.abs(got).max() < 1e-3 * gmax, k
        else:
            a, b = _stored(g, "grad." + k, got)
            figs[k] = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-6)
    print(tag, prec, "worst", max(figs.items(), key=lambda kv: kv[1]))
    for k, e in figs.items():
        assert e < (3e-4 if prec == "f32" else 0.1), (k, e)
    if m.lanes is not None:
        assert float(m.flat_grad[pad_mask(m)].abs().max()) == 0.0
    if prec != "f32":
        return
    tr = FusedBertTrainer(m, lam1, lam2, lr=float(g["lr"]), weight_decay=float(g["wd"]), clip=float(g["clip"]))
    tr.step(g["src"], g["dec"], g["labels"])
    torch.cuda.synchronize()
    print("loss %.7f (ref %.7f) grad norm %.7f (ref %.7f)" % (float(tr.loss()), float(g["loss"]), float(tr.grad_norm()), float(g["grad_norm"])))
    assert abs(float(tr.loss()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    assert abs(float(tr.grad_norm()) - float(g["grad_norm"])) < 3e-4 * float(g["grad_norm"])


# ---- dropout on: every site indexes the counter RNG at the TRUE width ---------------------------------------------------------------
def _drn_calls(monkeypatch):
    from adt_amd import ops
    n = {"fused": 0}
    fwd = ops.drn_lanes_fwd

    def spy(*a, **k):
        n["fused"] += 1
        return fwd(*a, **k)
    monkeypatch.setattr(ops, "drn_lanes_fwd", spy)
    return n


def _dropout_step(d, H, p, monkeypatch, fused):
    """tests/test_bert_hip.py::test_training_step_with_dropout_matches_oracle at a padded width, its bounds.  d = 50 is where a register
    quad straddles two rows: an index computed with the padded row length shows up here."""
    nl, inner = (2, 100) if d == 50 else (1, 64)
    cfg, P, src, dec, lab = make_case(d, H, nl, inner)
    cfg.dropout, cfg.attention_dropout = p, p
    n = _drn_calls(monkeypatch)
    m = build(cfg, P, "f32", p, p)
    assert m.lanes is not None and m.drn_fused == fused
    lam1, lam2 = [0.3, 0.2][:nl], [0.2, 0.1][:nl]
    got = grads_of(m, cfg, (src, dec, lab), lam1, lam2, seed=4242)
    assert n["fused"] == (5 * nl if fused else 0)          # five drop-residual-normalise sites per encoder / decoder layer pair
    loss, parts, G = bo.loss_and_grads(P, cfg, src, dec, lab, lam1, lam2, training=True, seed=4242)
    print("loss %.7f (oracle %.7f)" % (got, loss))
    assert abs(got - loss) < 1e-4 * abs(loss)
    errs = {k: rel(m.GR(k).cpu().numpy(), G[k]) for k in P}
    print("worst", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    for k, e in errs.items():
        assert e < 5e-4, (k, e)
    assert float(m.flat_grad[pad_mask(m)].abs().max()) == 0.0


@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("d,H", [(50, 1), (50, 2), (150, 3)])
def test_dropout_step_matches_oracle(d, H, p, monkeypatch):
    monkeypatch.delenv("ADT_DRN_LANES", raising=False)
    _dropout_step(d, H, p, monkeypatch, True)


def test_dropout_step_matches_oracle_two_pass(monkeypatch):
    """ADT_DRN_LANES=0 (read when the model is constructed): adt_drop_lanes + adt_layernorm_lanes_* instead of the fused pass."""
    monkeypatch.setenv("ADT_DRN_LANES", "0")
    _dropout_step(50, 2, 0.5, monkeypatch, False)


# ---- the fused kernels alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [77, 1])                     # 77 rows: not a multiple of the 16-row tile
@pytest.mark.parametrize("H,hd,hd_pad", [(1, 50, 64), (2, 25, 32), (2, 50, 64), (3, 50, 64), (1, 100, 128), (1, 200, 256)])
def test_drn_lanes_against_float64(H, hd, hd_pad, T):
    """adt_drn_lanes_fwd / _bwd (all four d_pad) with the bounds of tests/test_sasrec_oddwidth_hip.py::test_layernorm_lanes_against_float64:
    y 2e-6, dZ / dS 1e-5, dgamma / dbeta 1e-5.  Output buffers start as NaN: every pad lane must come back as +0.0."""
    from adt_amd import ops
    d, dp, eps, seed, site = H * hd, H * hd_pad, 1e-5, 4242, 19
    lanes = (H, hd, hd_pad)
    col = np.arange(dp)
    live = (col % hd_pad) < hd
    tcol = ((col // hd_pad) * hd + col % hd_pad)[live]
    r = np.random.RandomState(H * 1000 + hd + T)
    S, R, dY = (np.zeros((T, dp), np.float32) for _ in range(3))
    gam, bet = np.zeros(dp, np.float32), np.zeros(dp, np.float32)
    S[:, live], R[:, live], dY[:, live] = r.randn(T, d) * 2, r.randn(T, d) + 0.5, r.randn(T, d)
    gam[live], bet[live] = 1 + 0.3 * r.randn(d), 0.2 * r.randn(d)
    tS, tR, tdY, tg, tb = (torch.from_numpy(a).to(DEV) for a in (S, R, dY, gam, bet))
    tseed = torch.tensor([seed], device=DEV, dtype=torch.int32)
    nan = float("nan")
    for p in (0.0, 0.5):
        for row_offset in (0, 5):
            if p == 0.0:
                keep, scale = np.ones((T, d), bool), 1.0
            else:
                keep = rng.keep_mask(seed, site, (np.arange(T)[:, None] + row_offset) * d + tcol[None, :], p)
                scale = 1.0 / (1.0 - rng.drop_prob(p))
                assert 0.3 < keep.mean() < 0.7 or T == 1
            what = "p %g offset %d" % (p, row_offset)
            tZ, tY = torch.full((T, dp), nan, device=DEV), torch.full((T, dp), nan, device=DEV)
            ops.drn_lanes_fwd(tS, tR, tg, tb, eps, lanes, p, tseed, site, row_offset, Z=tZ, Y=tY)
            Z, Y = tZ.cpu().numpy(), tY.cpu().numpy()
            s, x0, dy, gm = S[:, live].astype(np.float64), R[:, live].astype(np.float64), dY[:, live].astype(np.float64), gam[live].astype(np.float64)
            z = x0 + keep * scale * s
            mu = z.mean(1, keepdims=True)
            rstd = 1.0 / np.sqrt(((z - mu) ** 2).mean(1, keepdims=True) + eps)
            xh = (z - mu) * rstd
            close(Z[:, live], z, 2e-6, what + " z")
            close(Y[:, live], xh * gm + bet[live], 2e-6, what + " y")
            assert np.array_equal(Z[:, live][~keep], R[:, live][~keep]), what            # dropped: the residual alone, bit for bit
            dxh = dy * gm
            dz = rstd * (dxh - dxh.mean(1, keepdims=True) - xh * (dxh * xh).mean(1, keepdims=True))
            for acc in (False, True):
                dR0 = np.full((T, dp), nan, np.float32)
                if acc:
                    dR0[:, live] = 0.1 * r.randn(T, d)              # pad lanes stay NaN: they are written, not added to
                tdR, tdS = torch.from_numpy(dR0).to(DEV), torch.full((T, dp), nan, device=DEV)
                tdg, tdb = torch.full((dp,), 7.0, device=DEV), torch.full((dp,), -3.0, device=DEV)
                tdg[torch.from_numpy(live).to(DEV)] = 0.0
                tdb[torch.from_numpy(live).to(DEV)] = 0.0
                ops.drn_lanes_bwd(tdY, tZ, tg, eps, lanes, p, tseed, site, row_offset, tdR, acc, tdS, tdg, tdb)
                torch.cuda.synchronize()
                dR, dS, dg, db = tdR.cpu().numpy(), tdS.cpu().numpy(), tdg.cpu().numpy(), tdb.cpu().numpy()
                close(dR[:, live], dz + (dR0[:, live] if acc else 0.0), 1e-5, what + " dZ acc %d" % acc)
                close(dS[:, live], keep * scale * dz, 1e-5, what + " dS")
                assert not np.any(dS[:, live][~keep]), what                              # dropped: exactly zero
                close(dg[live], (dy * xh).sum(0), 1e-5, what + " dgamma")
                close(db[live], dy.sum(0), 1e-5, what + " dbeta")
                for nm, t in (("z", Z), ("y", Y), ("dR", dR), ("dS", dS)):
                    assert (t[:, ~live].view(np.uint32) == 0).all(), (what, nm)          # bit-exact +0.0
                assert (dg[~live] == 7.0).all() and (db[~live] == -3.0).all(), what      # pad entries untouched


# ---- the padded layout through training, checkpoints and data parallelism -------------------------------------------------------------
def _trainer(d, H, inner, seed, prec="bf16", p=0.3, use_graph=False, clip=0.25, V=60, L=12, nl=1):
    from adt_amd.bert4rec.trainer import FusedBertTrainer
    torch.manual_seed(seed)
    cfg = bo.Cfg(V, L, d, H, nl, inner)
    m = build(cfg, None, prec, p, p)
    return m, FusedBertTrainer(m, [0.2] * nl, [0.1] * nl, lr=1e-3, weight_decay=1e-3, clip=clip, use_graph=use_graph, seed=5)


def _batches(n, B=8, V=60, L=12):
    out = []
    for i in range(n):
        _, _, src, dec, lab = make_case(64, 1, 1, 64, V=V, L=L, B=B, seed=100 + i)
        out.append((src, dec, lab))
    return out


@pytest.mark.parametrize("d,H,inner", [(50, 1, 50), (50, 2, 100), (150, 3, 64)])
def test_pad_lanes_stay_zero_through_training(d, H, inner):
    """Five graph-replayed steps with dropout, coupled weight decay and an active clip: every float of the weights, the gradient and both
    Adam moments that is not a reference element is bit-zero (inner 50 also pads the feed-forward width to 52), and the weights moved."""
    m, tr = _trainer(d, H, inner, 3, use_graph=True)
    w0 = m.ref_flat.clone()
    pads = pad_mask(m)
    assert int(pads.sum()) > 0
    for b in _batches(5):
        tr.step(*b)
        assert float(tr.grad_norm()) > 0.25       # the clip is active
    torch.cuda.synchronize()
    for nm, t in (("flat", m.flat), ("flat_grad", m.flat_grad), ("exp_avg", tr.m), ("exp_avg_sq", tr.v)):
        assert (t[pads].view(torch.int32) == 0).all(), nm
    assert float((m.ref_flat - w0).abs().max()) > 1e-3
    assert torch.equal(m.compact(m.flat), m.ref_flat)


def test_padding_is_invisible_in_checkpoints(tmp_path):
    from adt_amd import checkpoint as ck
    from adt_amd.bert4rec.model import param_table
    d, H, inner = 50, 2, 50
    m1, tr1 = _trainer(d, H, inner, 11)
    ref = dict(param_table(60, 12, d, H, 1, inner, 2))
    sd = m1.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in ref.items()}
    assert [n for n, _ in m1.named_parameters()] == list(sd.keys())
    batches = _batches(3)
    for b in batches[:2]:
        tr1.step(*b)
    path = os.path.join(tmp_path, "ck.pt")
    ck.save(path, m1, tr1)
    saved = torch.load(path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == {k: tuple(s) for k, s in ref.items()}
    m2, tr2 = _trainer(d, H, inner, 99)            # different init: everything must come from the file
    assert not torch.equal(m2.ref_flat, m1.ref_flat)
    ck.load(path, m2, tr2)
    torch.cuda.synchronize()
    # the resumed state is the saved one bit for bit: weights (reference-shaped and padded), both moments, step count, dropout stream
    assert torch.equal(m2.ref_flat, m1.ref_flat) and torch.equal(m2.flat, m1.flat)
    assert torch.equal(tr2.m, tr1.m) and torch.equal(tr2.v, tr1.v) and torch.equal(m2._seed, m1._seed)
    assert tr2.nstep == 2 and float(tr2.scal[2]) == 2.0
    tr1.step(*batches[2])
    tr2.step(*batches[2])
    torch.cuda.synchronize()
    dlt = (m2.ref_flat - m1.ref_flat).abs()        # the bound of tests/test_checkpoint_hip.py::test_resume_equals_uninterrupted (float atomics)
    assert float((dlt > 1e-5).float().mean()) < 1e-3 and float(dlt.max()) <= 4e-3
    # torch.optim.Adam state: reference shapes out, and back in bit for bit
    osd = ck.to_torch_adam_state(tr1, skip_untrained=False)
    params = list(m1.parameters())
    assert [tuple(osd["state"][i]["exp_avg"].shape) for i in range(len(params))] == [tuple(q.shape) for q in params]
    m0, v0 = tr1.m.clone(), tr1.v.clone()
    ck.from_torch_adam_state(tr1, osd)
    torch.cuda.synchronize()
    assert torch.equal(tr1.m, m0) and torch.equal(tr1.v, v0)


def test_two_shards_equal_the_whole_batch():
    """The data-parallel decomposition at (50, 1): a global batch of 4 split 2 + 2 with global normalisers and global dropout indices
    (b_offset).  The two shards' gradients, summed -- what the flat all-reduce computes, pads (zeros) included -- equal the whole
    batch's, within tests/test_sasrec_oddwidth_hip.py's 5e-5."""
    cfg, P, src, dec, lab = make_case(50, 1, 2, 100, B=4)
    p = 0.5
    m = build(cfg, P, "f32", p, p)
    nv = int((lab != 0).sum())

    def run(lo, hi):
        grads_of(m, cfg, (src[lo:hi], dec[lo:hi], lab[lo:hi]), [0.3, 0.2], [0.2, 0.1], b_offset=lo, n_valid=nv, B_global=4, seed=777)
        return m.flat_grad.clone()
    g, g0, g1 = run(0, 4), run(0, 2), run(2, 4)
    err = float((g0 + g1 - g).abs().max()) / float(g.abs().max())
    print("shards against the whole batch: %.3g" % err)
    assert err <= 5e-5
    assert float((g0 + g1)[pad_mask(m)].abs().max()) == 0.0


def test_streamed_attention_with_an_explicit_scale():
    """d 50, one head, L 272 (past the resident kernels' 224 rows at the padded head size 64), lens [250, 31]: the streamed kernels with
    scale = 1 / sqrt(50), forward against the oracle."""
    cfg, P, src, dec, lab = make_case(50, 1, 1, 100, L=272, B=2, lens=[250, 31])
    m = build(cfg, P, "f32")
    m.eval()
    logits, enc_in, dec_out, rec = m(src, dec)
    want = bo.forward(P, cfg, src, dec, training=False)
    close(logits.cpu().numpy(), want[0], 1e-4, "logits")
    close(enc_in[0].cpu().numpy(), want[1][0], 1e-4, "enc_in")
    close(dec_out[0].cpu().numpy(), want[2][0], 1e-4, "dec_out")


def test_ranking_and_fused_head_at_d50(monkeypatch):
    """rank_full / recommend on the padded table equal ranks computed from the dense logits; --fused_head runs at d_pad 64."""
    cfg, P, src, dec, lab = make_case(50, 1, 1, 100, V=300, B=4)
    V = cfg.item_num
    m = build(cfg, P, "f32")
    m.eval()
    tgt = np.array([3, 17, 200, 299])
    rank, n_elig, top_idx, top_val = m.rank_full(src, tgt, None, 5)
    scores = m.predict(None, src, None, None, np.tile(np.arange(1, V + 1), (4, 1))).cpu().numpy()          # items 1..V, dense
    want_rank = (scores > scores[np.arange(4), tgt - 1][:, None]).sum(1)
    assert list(rank.cpu().numpy()) == list(want_rank) and list(n_elig.cpu().numpy()) == [V - 1] * 4
    order = np.argsort(-scores, axis=1, kind="stable")[:, :5] + 1
    assert np.array_equal(top_idx.cpu().numpy(), order)
    ids, vals = m.recommend(src, 5)
    assert np.array_equal(ids.cpu().numpy(), order)
    close(vals.cpu().numpy(), np.take_along_axis(scores, order - 1, 1), 1e-5, "top-5 scores")
    # the fused all-item logits + cross-entropy head against the unfused one, bf16 (the loss bound of tests/test_bert_fused_head_hip.py)
    from adt_amd import ops
    calls, lce = [], ops.lce_fwd_bwd

    def spy(h, *a, **k):
        calls.append(tuple(h.shape))
        return lce(h, *a, **k)
    monkeypatch.setattr(ops, "lce_fwd_bwd", spy)
    losses = {}
    for fused in (False, True):
        mm = build(cfg, P, "bf16", fused_head=fused)
        assert mm.dp == 64 and mm.fused_head == fused
        losses[fused] = grads_of(mm, cfg, (src, dec, lab), [0.2], [0.1])
        assert len(calls) == int(fused)                    # the fused head ran for the flagged model only ...
    assert calls[0][1] == 64                               # ... on the padded rows
    print("loss unfused %.6f fused %.6f" % (losses[False], losses[True]))
    assert abs(losses[True] - losses[False]) < 3e-2 * abs(losses[False])


def test_tiled_widths_are_untouched_and_unsupported_uses_raise():
    from adt_amd._lib import AdtError
    from adt_amd.bert4rec.model import param_table
    from adt_amd.bert4rec.superbert import SuperBertModel
    cfg = bo.Cfg(40, 12, 64, 2, 1, 96)
    m = build(cfg, None, "bf16")
    assert m.lanes is None and m.ref_flat is None and m.master is m.flat and m.dp == 64
    assert m.n_flat == sum((int(np.prod(s)) + 3) // 4 * 4 for _, s in param_table(40, 12, 64, 2, 1, 96, 2))
    assert m.P("item_emb.word_emb.weight").data_ptr() == m.item_emb.word_emb.weight.data_ptr()
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = DEV, 12, 1, 1, 50, 100
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = 0.0, 0.0, 2, "bf16"
    with pytest.raises(AdtError, match="supernet"):
        SuperBertModel(1, 40, [0.0, 0.5], [0.0, 0.5], a)
    cfg50, P, src, dec, lab = make_case(50, 1, 1, 100)
    m50 = build(cfg50, P, "f32")
    m50.train()
    with pytest.raises(AdtError, match="FusedBertTrainer"):
        m50(src, dec)


def test_main_at_hidden_units_50_end_to_end(tmp_path, capsys):
    from adt_amd.bert4rec.main import main
    main(["--dataset", "ml-1m", "--data_dir", str(tmp_path), "--synthetic", "tiny", "--template", "0", "--num_epochs", "2", "--eval_interval", "2",
          "--maxlen", "16", "--batch_size", "32", "--eval_batch_size", "24", "--eval_negative_sample_size", "10", "--dupe_factor", "2",
          "--prop_sliding_window", "0.5", "--hidden_units", "50", "--num_heads", "1", "--inner_units", "96"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["epoch"] == 2 and np.isfinite(lines[0]["loss"])
    for split in ("valid", "test"):
        assert 0.0 <= lines[0][split]["ndcg10"] <= 1.0 and 0.0 <= lines[0][split]["hr10"] <= 1.0 and 0.0 <= lines[0][split]["auc"] <= 1.0
