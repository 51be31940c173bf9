"""GPU: STOSA-ADT at widths the kernels pad -- hidden_units 50 (one head: 64 lanes), 100 (2 x 64), 48 (4 heads of 12: 4 x 16), 150
(3 x 64 = 192) -- under the Wasserstein distance (adt_amd/stosa/models.py).

Reference parity against tests/golden/stosa_{w50_h1,w100_h2,w48_h4,w150_h3}.npz with the bounds of tests/test_stosa_hip.py, dropout-on
parity against the numpy oracle, every new kernel alone against float64 with the keep mask of oracle/rng.py (the lane activation pass, the
lane-aware distances, the attention entry points that take the score scale), and the properties of the padded layout: pad lanes stay
exactly zero, checkpoints and parameters show the reference's shapes only, tiled widths run exactly what they ran before."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import rng, stosa_oracle as so, tape as tp  # noqa: E402
from tools.gen_golden_inputs import golden_err, sample_idx  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ["w50_h1", "w100_h2", "w48_h4", "w150_h3"]
K = 320          # samples per compacted tensor (tools/gen_golden_stosa.py:STOSA_ODD_COMPACT)
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


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def seed_tensor(seed):
    return torch.tensor([seed], device=DEV, dtype=torch.int32)


def perturb(P, seed):
    """tools/gen_golden_stosa.py:reference_model: Linear biases away from their zero init."""
    r = np.random.RandomState(seed + 1)
    for k in P:
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return P


def load_case(tag):
    g = np.load(os.path.join(GOLD, "stosa_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    return g, cfg, perturb(so.init_params(cfg, int(g["seed"])), int(g["seed"]))


def make_case(d, H, nl=1, V=40, L=12, seed=5, lens=(12, 3, 0)):
    """A seeded model and a batch with one full row, one mostly padded row and one all-padding row (left-padded, as stosa/datasets.py)."""
    cfg = so.Cfg(V, L, d, H, nl, num_users=4, pvn_weight=0.1)
    P = perturb(so.init_params(cfg, seed), seed)
    r = np.random.RandomState(seed + 7)
    B = len(lens)
    inp, dec, pos, neg = (np.zeros((B, L), np.int64) for _ in range(4))
    for b, n in enumerate(lens):
        if n == 0:
            continue
        items = r.randint(1, V, size=n + 1)
        inp[b, L - n:], pos[b, L - n:], neg[b, L - n:] = items[:-1], items[1:], r.randint(1, V, size=n)
        dec[b, 1:] = inp[b, :-1]
    return cfg, P, (inp, dec, pos, neg)


def build(cfg, P, prec, dropout=0.0, attention_dropout=0.0, metric="wasserstein"):
    from adt_amd.stosa.models import DisenDistSAModel
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, cfg.item_size, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.num_users
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = dropout, attention_dropout, cfg.pvn_weight, prec, metric
    m = DisenDistSAModel(a)
    if P is not None:
        m.load_numpy(P)
    return m


def pad_mask(m):
    """True on every float of the flat layout that no reference element maps to (pad lanes and alignment gaps)."""
    mask = torch.ones(m.n_flat, dtype=torch.bool, device=m.dev)
    mask[m.lane_idx.long()] = False
    return mask


def loss_weights(cfg, lam1, lam2):
    w = [1.0, 1.0, 0.0]
    for l in range(cfg.num_layers):
        w += [lam1[l]] * 2
    for l in range(cfg.num_layers):
        w += [lam2[l]] * 2
    return np.array(w)


def one_pass(m, cfg, batch, lam1, lam2, lo=0, hi=None, seed=None, B_global=None, nt=None):
    """Forward + loss + backward into flat_grad on rows lo:hi of the batch -> (loss, the loss slots' sums)."""
    inp, dec, pos, neg = (x[lo:hi] for x in batch)
    B, L = (len(batch[0]) if B_global is None else B_global), cfg.maxlen
    m.train()
    if seed is not None:
        m.set_seed(seed)
    m.push()
    st = m.stage(inp, dec, pos, neg, n_target_global=nt)
    norms = torch.tensor([0.0, B * L * cfg.hidden_units, B * L * cfg.num_heads], device=DEV)       # the TRUE d
    slots = torch.zeros(3 + 4 * cfg.num_layers, 64, device=DEV)
    m.flat_grad.zero_()
    m.loss_forward_backward(st, lam1, lam2, norms, slots, b_offset=lo)
    torch.cuda.synchronize()
    parts = slots.sum(1).cpu().numpy()
    return float((parts * loss_weights(cfg, lam1, lam2)).sum()), parts


def stored(g, key, got):
    got = np.asarray(got, np.float64)
    if key in g.files:
        return got.reshape(-1), np.asarray(g[key], np.float64).reshape(-1)
    return got.reshape(-1)[sample_idx(got.size, K)], np.asarray(g[key + "@sample"], np.float64)


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_finetune_predict_and_loss_parts_match_reference(tag, prec):
    """tests/test_stosa_hip.py::test_finetune_and_full_sort_match_reference and the loss parts of ::test_train_steps_match_reference_fp32."""
    from adt_amd.wide import padded_layout
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    d, H = cfg.hidden_units, cfg.num_heads
    assert m.lanes == (H,) + padded_layout(d, H)[:2] and m.hidden_units == d and m.dp == padded_layout(d, H)[2] and m.ref_flat is not None
    m.eval()
    B, L = g["input_ids"].shape
    mo, co, _, margins, enc_in, enc_rec, dec_out = m.finetune(g["input_ids"], g["dec_ids"], np.zeros(B, np.int64))
    tol = 1e-4 if prec == "f32" else 3e-2
    assert tuple(mo.shape) == (B, L, d) and tuple(margins.shape) == (B, 1)
    figs = {"mean_out": golden_err(mo.cpu().numpy(), g, "mean_out", K), "cov_out": golden_err(co.cpu().numpy(), g, "cov_out", K)}
    for i in range(cfg.num_layers):
        assert tuple(enc_in[i][1].shape) == (B, L, d) and tuple(enc_rec[i][0].shape) == (B, L, H, H)
        for nm, pair in (("enc_in", enc_in[i]), ("rec", enc_rec[i]), ("dec_out", dec_out[i])):
            for t, which in enumerate(("mean", "cov")):
                figs["%s_%s_%d" % (nm, which, i)] = golden_err(pair[t].cpu().numpy(), g, "%s_%s_%d" % (nm, which, i), K)
    figs["full_dist"] = golden_err(m.predict_full(g["input_ids"], g["dec_ids"]).cpu().numpy(), g, "full_dist", K)
    print(tag, prec, figs)
    for k, e in figs.items():
        assert e < tol, (k, e)
    sd = m.state_dict()          # state_dict names and shapes are the reference's
    assert set(sd) == set(P) and all(tuple(sd[k].shape) == P[k].shape for k in P)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    loss, parts = one_pass(m, cfg, tuple(g[k] for k in ("input_ids", "dec_ids", "pos_ids", "neg_ids")), lam1, lam2)
    print("bpr %.7f (%.7f) pvn %.7f (%.7f) auc %.7f (%.7f) loss %.7f (%.7f)" % (parts[0], g["bpr"], parts[1], g["pvn"], parts[2], g["auc"], loss, g["loss"]))
    lt = 1e-4 if prec == "f32" else 3e-2          # bf16: the loss is a mean of distances of bf16-bound activations (tests/test_stosa_long_hip.py)
    assert abs(parts[0] - float(g["bpr"])) < lt * abs(float(g["bpr"]))
    assert abs(parts[1] - float(g["pvn"])) < lt * max(abs(float(g["pvn"])), 1e-5)
    if prec == "f32":
        assert abs(parts[2] - float(g["auc"])) < 1e-5
    assert abs(loss - float(g["loss"])) < lt * abs(float(g["loss"]))


@pytest.mark.parametrize("tag", TAGS)
def test_weights_after_one_and_three_steps_fp32(tag):
    """Step 1: the bounds of tests/test_stosa_hip.py::test_train_steps_match_reference_fp32.  Step 3 (that test stops at 1): Adam moves an
    entry by at most about lr a step, so 3.03 lr bounds everything; an entry whose first gradient is well above Adam's eps keeps its
    direction and is held to 0.3 lr, the bound tests/test_oracle_wide.py holds the CPU oracle to after three steps."""
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P, "f32")
    lam1, lam2, lr = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]], float(g["lr"])
    tr = FusedStosaTrainer(m, lam1, lam2, lr=lr)
    none = set(str(x) for x in g["grad_none"])
    for step in (1, 2, 3):
        tr.step(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
        torch.cuda.synchronize()
        if step == 1:
            assert abs(float(tr.loss()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
        if step == 2:
            continue
        worst = 0.0
        for k in P:
            got, want = stored(g, "w%d." % step + k, m.R(k).cpu().numpy())
            diff = np.abs(got - want)
            if k in none:
                assert diff.max() == 0.0, k          # grad None in the reference: untouched by Adam
                continue
            big = np.abs(stored(g, "grad." + k, np.zeros(P[k].shape))[1]) > 1e-5
            worst = max(worst, diff[big].max() / lr if big.any() else 0.0)
            assert (diff[big].max() if big.any() else 0.0) < (0.05 if step == 1 else 0.3) * lr, (step, k)
            assert diff.max() < (1.01 if step == 1 else 3.03) * lr, (step, k)
        print(tag, "step", step, "worst well-conditioned entry: %.3g lr" % worst)
    assert torch.equal(m.compact(m.flat), m.ref_flat)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_gradients_match_reference(tag, prec):
    """tests/test_stosa_hip.py::test_gradients_match_reference on the stored entries; the pad lanes of the gradient are exact zeros."""
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    one_pass(m, cfg, tuple(g[k] for k in ("input_ids", "dec_ids", "pos_ids", "neg_ids")), lam1, lam2)
    none = set(str(x) for x in g["grad_none"])
    gmax = max(float(np.abs(stored(g, "grad." + k, np.zeros(P[k].shape))[1]).max()) for k in P if k not in none)
    worst = ("", 0.0)
    for k in P:
        full = m.GR(k).cpu().numpy()
        assert full.shape == P[k].shape, k
        if k in none:
            assert np.all(full == 0.0), k
            continue
        got, want = stored(g, "grad." + k, full)
        if prec == "f32":
            e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-3 * gmax)
            assert e < 5e-4, (k, e)
        else:
            e = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-3 * gmax * np.sqrt(want.size))
            assert e < 0.1, (k, e)
        worst = max(worst, (k, e), key=lambda kv: kv[1])
    print(tag, prec, "worst", worst)
    assert float(m.flat_grad[pad_mask(m)].abs().max()) == 0.0


# ---- dropout on: every site indexes the counter RNG at the TRUE width -------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(50, 1), (48, 4), (100, 2)])
def test_dropout_step_matches_oracle(d, H):
    """tests/test_stosa_hip.py::test_training_step_with_dropout_matches_oracle at padded widths, its bounds.  B = 3 at d = 50 makes a
    register quad straddle two rows: an index computed with the padded row length shows up here.  One full row, one mostly padded row and
    one all-padding row (every query dead: uniform attention over all keys, no loss term)."""
    cfg, P, batch = make_case(d, H, nl=2 if d == 50 else 1)
    cfg.dropout, cfg.attention_dropout = 0.3, 0.3
    m = build(cfg, P, "f32", 0.3, 0.3)
    assert m.lanes is not None
    lam1, lam2 = [0.25, 0.1][:cfg.num_layers], [0.15, 0.05][:cfg.num_layers]
    got, _ = one_pass(m, cfg, batch, lam1, lam2, seed=9001)
    loss, parts, G = so.loss_and_grads(P, cfg, *batch, lam1, lam2, training=True, seed=9001)
    print("loss %.7f (oracle %.7f)" % (got, loss))
    assert abs(got - loss) < 1e-4 * abs(loss)
    gmax = max(float(np.abs(v).max()) for v in G.values() if v is not None)
    errs = {k: np.abs(m.GR(k).cpu().numpy() - G[k]).max() / max(np.abs(G[k]).max(), 1e-3 * gmax) for k in P if G[k] is not None}
    print("worst", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    for k, e in errs.items():
        assert e < 5e-4, (k, e)
    assert float(m.flat_grad[pad_mask(m)].abs().max()) == 0.0


# ---- the new kernels alone ------------------------------------------------------------------------------------------------------------
def _act64(x, elu1):
    y = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    dy = np.where(x > 0, 1.0, np.exp(np.minimum(x, 0)))
    return (y + 1.0 if elu1 else y), dy


@pytest.mark.parametrize("T", [1, 3, 67])                     # 67 rows: not a multiple of anything the grid uses
@pytest.mark.parametrize("H,hd,hd_pad", [(1, 50, 64), (4, 12, 16), (2, 50, 64), (3, 50, 64), (4, 50, 64)])          # d_pad 64, 64, 128, 192, 256
def test_act_lanes_against_float64(H, hd, hd_pad, T):
    """adt_act_lanes_fwd / _bwd, ELU and ELU + 1, with and without dropout, with the bounds of
    tests/test_sasrec_oddwidth_hip.py::test_layernorm_lanes_against_float64 for the same kind of comparison (y 2e-6, dx 1e-5).  Output
    buffers start as NaN: every pad lane must come back as +0.0, bit for bit -- ELU(0) + 1 = 1 must not appear there."""
    from adt_amd import ops
    d, dp, seed, site = H * hd, H * hd_pad, 4242, 23
    lanes = (H, hd, hd_pad)
    col = np.arange(dp)
    live = (col % hd_pad) < hd
    tcol = ((col // hd_pad) * hd + col % hd_pad)[live]
    r = np.random.RandomState(H * 1000 + hd + T)
    X, dY = np.zeros((T, dp), np.float32), np.zeros((T, dp), np.float32)
    X[:, live], dY[:, live] = r.randn(T, d) * 1.5, r.randn(T, d)
    dY[:, ~live] = 3.0          # a pad lane of dY must not reach dX whatever it holds
    tX, tdY, tseed = T_(X), T_(dY), seed_tensor(seed)
    nan = float("nan")
    for act, elu1 in ((ops.ACT_ELU, False), (ops.ACT_ELU1, True)):
        for p, row_offset in ((0.0, 0), (0.5, 0), (0.5, 5)):
            if p == 0.0:
                keep, scale = np.ones((T, d), bool), 1.0
            else:
                keep = rng.keep_mask(seed, site, (np.arange(T)[:, None] + row_offset) * d + tcol[None, :], p)
                scale = 1.0 / (1.0 - rng.drop_prob(p))
                assert 0.3 < keep.mean() < 0.7 or T < 8
            what = "act %d p %g offset %d" % (act, p, row_offset)
            u = keep * scale * X[:, live].astype(np.float64)
            y, du = _act64(u, elu1)
            Y = ops.act_lanes_fwd(tX, lanes, act, p, tseed, site, row_offset).cpu().numpy()
            close(Y[:, live], y, 2e-6, what + " y")
            assert (Y[:, ~live].view(np.uint32) == 0).all(), what
            for acc in (False, True):
                dX0 = np.full((T, dp), nan, np.float32)
                if acc:
                    dX0[:, live] = 0.1 * r.randn(T, d)              # pad lanes stay NaN: they are written, not added to
                tdX = T_(dX0)
                ops.act_lanes_bwd(tdY, tX, lanes, act, tdX, acc, p, tseed, site, row_offset)
                torch.cuda.synchronize()
                dX = tdX.cpu().numpy()
                close(dX[:, live], dY[:, live].astype(np.float64) * du * keep * scale + (dX0[:, live] if acc else 0.0), 1e-5, what + " dx acc %d" % acc)
                assert not np.any(dX[:, live][~keep]) or acc, what            # dropped: exactly zero
                assert (dX[:, ~live].view(np.uint32) == 0).all(), what
    # three padded rows side by side (the q / k / v projections), contiguous and as column slices of a wider buffer
    X3 = np.concatenate([X, 0.5 * X, -X], 1)
    want = np.concatenate([_act64(c[:, live].astype(np.float64), True)[0] for c in (X, 0.5 * X, -X)], 1)
    wide = torch.zeros(T, 3 * dp + 64, device=DEV)
    wide[:, :3 * dp] = T_(X3)
    for src in (T_(X3), wide[:, :3 * dp]):
        Y3 = ops.act_lanes_fwd(src, lanes, ops.ACT_ELU1).cpu().numpy()
        live3 = np.tile(live, 3)
        close(Y3[:, live3], want, 2e-6, "three rows side by side")
        assert (Y3[:, ~live3].view(np.uint32) == 0).all()


def _dist_case(H, hd, hd_pad, V=40, T=36):
    r = np.random.RandomState(H * 100 + hd)
    d, dp = H * hd, H * hd_pad
    col = np.arange(dp)
    live = (col % hd_pad) < hd
    Em, Ec, sm, sc = (np.zeros((n, dp), np.float32) for n in (V, V, T, T))
    Em[:, live], Ec[:, live] = r.standard_normal((V, d)), r.standard_normal((V, d))
    sm[:, live], sc[:, live] = r.standard_normal((T, d)), np.exp(0.3 * r.standard_normal((T, d)))
    pos, neg = r.randint(1, V, size=T), r.randint(1, V, size=T)
    pos[:4], neg[:4] = 0, 0
    neg[7] = 0          # a negative that is the padding row: no gradient into it
    return d, dp, live, Em, Ec, sm, sc, pos, neg


@pytest.mark.parametrize("H,hd,hd_pad", [(4, 12, 16), (1, 50, 64)])
def test_lane_aware_distances_against_float64(H, hd, hd_pad):
    """adt_wdist_bpr_lanes / adt_wdist_full_lanes / adt_wdist_pack_lanes against the Wasserstein distance over the TRUE d (the oracle's
    bpr_terms and wasserstein_distance_matmul on the live columns), with the bounds of the direct tests of the unpadded kernels
    (tests/test_wide_kernels.py::test_wasserstein_bpr_and_full_sort: losses 2e-5, gradients 3e-5, distances 2e-5;
    tests/test_stosa_fullrank_hip.py: image bit-equal to the operands, norm 1e-6).  Pad lanes of every gradient and of the image: +0.0."""
    from adt_amd import ops
    V, T = 40, 36
    d, dp, live, Em, Ec, sm, sc, pos, neg = _dist_case(H, hd, hd_pad, V, T)
    lanes = (H, hd, hd_pad)
    cfg = so.Cfg(V, T, d, H, 1, pvn_weight=0.3)
    f64 = lambda a: a[:, live].astype(np.float64)
    Vv = {"item_mean_embeddings.weight": tp.leaf(f64(Em)), "item_cov_embeddings.weight": tp.leaf(f64(Ec))}
    vsm, vsc = tp.leaf(f64(sm)[None]), tp.leaf(f64(sc)[None])
    loss, auc, pvn = so.bpr_terms(Vv, cfg, vsm, vsc, pos[None], neg[None])
    tp.backward(tp.add(loss, pvn))
    inv = torch.tensor([1.0 / float((pos > 0).sum())], device=DEV, dtype=torch.float32)
    dEm, dEc = torch.zeros(V, dp, device=DEV), torch.zeros(V, dp, device=DEV)
    loss3 = torch.zeros(192, device=DEV)
    dSm, dSc = ops.wdist_bpr_lanes(T_(sm), T_(sc), T_(Em), T_(Ec), T_(pos.astype(np.int32)), T_(neg.astype(np.int32)), 0.3, inv, dEm, dEc, loss3, lanes)
    torch.cuda.synchronize()
    l3 = loss3.view(3, 64).sum(1).cpu().numpy()
    print("bpr %.7f (%.7f) pvn %.7f (%.7f) auc %.7f (%.7f)" % (l3[0], float(loss.v), l3[1], float(pvn.v), l3[2], auc))
    assert abs(l3[0] - float(loss.v)) < 2e-5 * abs(float(loss.v)) and abs(l3[1] - float(pvn.v)) < 2e-5 * abs(float(pvn.v)) and abs(l3[2] - auc) < 1e-6
    for nm, got, want in (("dSm", dSm, vsm.g[0]), ("dSc", dSc, vsc.g[0]), ("dEm", dEm, Vv["item_mean_embeddings.weight"].g),
                          ("dEc", dEc, Vv["item_cov_embeddings.weight"].g)):
        got = got.cpu().numpy()
        close(got[:, live], want, 3e-5, nm)
        assert (got[:, ~live].view(np.uint32) == 0).all(), nm
    last_m, last_c = sm[-5:], sc[-5:]
    want = so.wasserstein_distance_matmul(tp.const(f64(last_m)), tp.const(f64(last_c)), tp.const(f64(Em)), tp.elu(tp.const(f64(Ec)), True)).v
    got = ops.wdist_full_lanes(T_(last_m), T_(last_c), T_(Em), T_(Ec), V, lanes).cpu().numpy()
    close(got, want, 2e-5, "wdist_full_lanes")
    # the image of the fused ranking: [mean | sqrt(cov)] on the live lanes, +0.0 on the pad lanes of both halves; dist = na - 2 (A . W + bias)
    W, bias = ops.wdist_pack_lanes(T_(Em), T_(Ec), True, -0.5, lanes)
    A, na = ops.wdist_pack_lanes(T_(last_m), T_(last_c), False, 1.0, lanes)
    W, bias, A, na = (t.cpu().numpy() for t in (W, bias, A, na))
    ec1 = np.where(f64(Ec) > 0, f64(Ec), np.expm1(np.minimum(f64(Ec), 0))) + 1.0
    close(W[:, :dp][:, live], f64(Em), 1e-7, "image mean")
    close(W[:, dp:][:, live], np.sqrt(np.maximum(ec1, 1e-24)), 1e-6, "image sqrt cov")
    close(bias, -0.5 * ((f64(Em) ** 2).sum(1) + ec1.sum(1)), 1e-6, "image bias")
    close(na, (f64(last_m) ** 2).sum(1) + f64(last_c).sum(1), 1e-6, "state norm")
    for img in (W, A):
        assert (img[:, :dp][:, ~live].view(np.uint32) == 0).all() and (img[:, dp:][:, ~live].view(np.uint32) == 0).all()
    close(na[:, None] - 2.0 * (A.astype(np.float64) @ W.astype(np.float64).T + bias[None]), want, 2e-5, "distance from the images")


def wattn_oracle(t6, ids, B, H, L, hd, p, seed, site, b_off, dOm, dOc):
    """tests/test_wide_kernels.py:wattn_oracle over the TRUE head size."""
    d = H * hd
    vs = [tp.leaf(x) for x in t6]

    def split(x):
        return tp.transpose(tp.reshape(x, (B, L, H, hd)), (0, 2, 1, 3))
    qm, qc, km, kc, vm, vc = [split(v) for v in vs]
    s = tp.div_const(tp.neg(so.wasserstein_distance_matmul(qm, qc, km, kc)), np.sqrt(hd))
    s = tp.add_const(s, so._mask(ids))
    pr = tp.dropout(tp.softmax(s), p, seed, site, tp.idx_attn(B, H, L, b_off))
    om = tp.reshape(tp.transpose(tp.matmul(pr, vm), (0, 2, 1, 3)), (B * L, d))
    oc = tp.reshape(tp.transpose(tp.matmul(tp.square(pr), vc), (0, 2, 1, 3)), (B * L, d))
    loss = tp.add(tp.sum_(tp.mul_mask(om, dOm)), tp.sum_(tp.mul_mask(oc, dOc)))
    tp.backward(loss)
    return om.v, oc.v, [v.g for v in vs]


def _padded(x, live, dp):
    out = np.zeros((x.shape[0], dp), np.float32)
    out[:, live] = x
    return out


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("family,H,hd,hd_pad,L", [("valu", 4, 12, 16, 12), ("mfma", 4, 12, 16, 12), ("valu", 1, 50, 64, 12), ("long", 1, 50, 64, 150),
                                                  ("long", 4, 12, 16, 12)])
def test_scaled_attention_against_the_true_head_size(family, H, hd, hd_pad, L, p):
    """adt_wattn_scaled_* (vector ALU), adt_wattn_mfma_scaled_* (matrix cores, exact fp32) and adt_wattn_long_scaled_* (streamed; L 150 is
    past the 141 rows the resident kernels hold at 64 lanes) on padded heads with scale = 1 / sqrt(hd), against the oracle over the true hd:
    exact fp32 1e-4 forward, 5e-4 gradients (tests/test_stosa_long_hip.py).  Sequence 0 starts with padding: its first rows are fully masked
    (uniform attention whose backward must reproduce the forward's scores bit for bit, or exp(+-512) shows up here as inf / 0)."""
    from adt_amd import ops
    B = 2
    d, dp, T = H * hd, H * hd_pad, B * L
    live = (np.arange(dp) % hd_pad) < hd
    r = np.random.RandomState(L * 100 + hd + H)
    qm, km, vm = (r.standard_normal((T, d)).astype(np.float32) for _ in range(3))
    qc, kc, vc = (np.exp(0.5 * r.standard_normal((T, d))).astype(np.float32) for _ in range(3))
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    ids[0, : L // 3] = 0
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    seed, site, b_off = 4321, 16, 3
    om, oc, grads = wattn_oracle((qm, qc, km, kc, vm, vc), ids, B, H, L, hd, p, seed, site, b_off, dOm, dOc)
    g = [T_(_padded(x, live, dp)) for x in (qm, qc, km, kc, vm, vc)]
    kid, sd, scale = T_(ids.reshape(-1)), seed_tensor(seed), 1.0 / np.sqrt(hd)
    pdOm, pdOc = _padded(dOm, live, dp), _padded(dOc, live, dp)
    pdOm[:, ~live], pdOc[:, ~live] = 2.0, -2.0          # what a pad lane of dO holds must not matter to the live gradients
    prec = None if family == "valu" else ops.PREC_F32          # prec None: the vector-ALU kernels; given: the matrix cores where they cover the shape
    if family == "long":
        Om, Oc, LSE = ops.wattn_long_scaled_fwd(*g, kid, B, H, L, scale, hd, p, sd, site, b_off, prec=prec)
    else:
        Om, Oc, LSE = ops.wattn_scaled_fwd(*g, kid, B, H, L, scale, hd, p, sd, site, b_off, prec=prec)
    close(Om.cpu().numpy()[:, live], om, 1e-4, "Om")
    close(Oc.cpu().numpy()[:, live], oc, 1e-4, "Oc")
    assert not np.any(Om.cpu().numpy()[:, ~live]) and not np.any(Oc.cpu().numpy()[:, ~live])
    if family == "long":
        outs = ops.wattn_long_scaled_bwd(*g, kid, Om, Oc, LSE, T_(pdOm), T_(pdOc), B, H, L, scale, hd, p, sd, site, b_off, prec=prec)
    else:
        outs = ops.wattn_scaled_bwd(*g, kid, Om, Oc, LSE, T_(pdOm), T_(pdOc), B, H, L, scale, hd, p, sd, site, b_off, prec=prec)
    torch.cuda.synchronize()
    for name, got, want in zip(("dQm", "dQc", "dKm", "dKc", "dVm", "dVc"), outs, grads):
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), name
        close(got[:, live], want, 5e-4, name)
        if name in ("dQm", "dQc", "dKm", "dKc"):          # dV's pad lanes carry P^T dO of the pad lanes of dO: the model's are zero
            assert not np.any(got[:, ~live]), name


@pytest.mark.parametrize("family", ["valu", "mfma", "long"])
def test_scaled_entry_points_equal_the_plain_ones_at_an_unpadded_head(family):
    """scale = 1 / sqrt(16) = 0.25 and hd_live = hd = 16: bit-equal outputs, forward and backward, dropout on, a fully masked prefix."""
    from adt_amd import ops
    B, H, L, hd, p = 2, 4, 20, 16, 0.3
    d, T = H * hd, B * L
    r = np.random.RandomState(7)
    qm, km, vm = (T_(r.standard_normal((T, d)).astype(np.float32)) for _ in range(3))
    qc, kc, vc = (T_(np.exp(0.5 * r.standard_normal((T, d))).astype(np.float32)) for _ in range(3))
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    ids[0, :7] = 0
    kid, sd = T_(ids.reshape(-1)), seed_tensor(99)
    dOm, dOc = T_(r.standard_normal((T, d)).astype(np.float32)), T_(r.standard_normal((T, d)).astype(np.float32))
    plain, scaled, prec = {"valu": ((ops.wattn_fwd, ops.wattn_bwd), (ops.wattn_scaled_fwd, ops.wattn_scaled_bwd), None),
                           "mfma": ((ops.wattn_fwd, ops.wattn_bwd), (ops.wattn_scaled_fwd, ops.wattn_scaled_bwd), ops.PREC_BF16),
                           "long": ((ops.wattn_long_fwd, ops.wattn_long_bwd), (ops.wattn_long_scaled_fwd, ops.wattn_long_scaled_bwd), ops.PREC_BF16)}[family]
    a = plain[0](qm, qc, km, kc, vm, vc, kid, B, H, L, p, sd, 16, 1, prec=prec)
    b = scaled[0](qm, qc, km, kc, vm, vc, kid, B, H, L, 0.25, hd, p, sd, 16, 1, prec=prec)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ga = plain[1](qm, qc, km, kc, vm, vc, kid, *a, dOm, dOc, B, H, L, p, sd, 16, 1, prec=prec)
    gb = scaled[1](qm, qc, km, kc, vm, vc, kid, *b, dOm, dOc, B, H, L, 0.25, hd, p, sd, 16, 1, prec=prec)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


# ---- the padded layout through training, checkpoints and data parallelism -------------------------------------------------------------
def _trainer(d, H, seed, prec="bf16", p=0.3, use_graph=False, V=60, L=12, nl=1, wd=1e-3, clip=0.25):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    torch.manual_seed(seed)
    cfg = so.Cfg(V, L, d, H, nl, num_users=4, pvn_weight=0.1)
    m = build(cfg, None, prec, p, p)
    tr = FusedStosaTrainer(m, [0.2] * nl, [0.1] * nl, lr=1e-3, weight_decay=wd, use_graph=use_graph, seed=5)
    tr.clip = clip          # the reference never clips (FusedStosaTrainer: 1e30); the kernel's clip path must keep the pad lanes zero too
    return m, tr


def _batches(n, B=8, V=60, L=12):
    out = []
    for i in range(n):
        r = np.random.RandomState(100 + i)
        lens = [L] + [int(r.randint(2, L + 1)) for _ in range(B - 1)]
        out.append(make_case(64, 1, V=V, L=L, seed=100 + i, lens=lens)[2])
    return out


@pytest.mark.parametrize("d,H", [(50, 1), (48, 4), (150, 3)])
def test_pad_lanes_stay_zero_through_training(d, H):
    """Five graph-replayed steps with dropout, coupled weight decay and an active clip: every float of the weights, the gradient and both
    Adam moments that is not a reference element is bit-zero, and the weights moved."""
    m, tr = _trainer(d, H, 3, use_graph=True)
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
    from adt_amd.stosa.models import param_table
    d, H = 50, 1
    m1, tr1 = _trainer(d, H, 11)
    ref = dict(param_table(60, 12, d, H, 1, 4)[0])
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
    m2, tr2 = _trainer(d, H, 99)            # different init: everything must come from the file
    assert not torch.equal(m2.ref_flat, m1.ref_flat)
    ck.load(path, m2, tr2)
    torch.cuda.synchronize()
    assert torch.equal(m2.ref_flat, m1.ref_flat) and torch.equal(m2.flat, m1.flat)
    assert torch.equal(tr2.m, tr1.m) and torch.equal(tr2.v, tr1.v) and torch.equal(m2._seed, m1._seed)
    assert tr2.nstep == 2
    tr1.step(*batches[2])
    tr2.step(*batches[2])
    torch.cuda.synchronize()
    dlt = (m2.ref_flat - m1.ref_flat).abs()        # the bound of tests/test_checkpoint_hip.py::test_resume_equals_uninterrupted (float atomics)
    assert float((dlt > 1e-5).float().mean()) < 1e-3 and float(dlt.max()) <= 4e-3


def test_two_shards_and_graph_replay():
    """tests/test_stosa_hip.py::test_dp_shard_and_graph_replay at (50, 1), its bounds: a batch of 4 split 2 + 2 with global normalisers and
    global dropout indices sums to the whole batch's gradient (1e-4), pads (zeros) included; four graph-replayed steps equal four eager ones
    (loss 1e-4, weights 5e-3)."""
    from adt_amd.stosa.trainer import FusedStosaTrainer
    cfg, P, batch = make_case(50, 1, lens=(12, 7, 3, 9))
    cfg.dropout, cfg.attention_dropout = 0.2, 0.2
    lam1, lam2 = [0.3], [0.2]
    nt = int((batch[2] > 0).sum())
    m = build(cfg, P, "f32", 0.2, 0.2)
    grads = []
    for lo, hi in ((0, 4), (0, 2), (2, 4)):
        one_pass(m, cfg, batch, lam1, lam2, lo, hi, seed=31337, B_global=4, nt=nt)
        grads.append(m.flat_grad.clone())
    err = rel((grads[1] + grads[2]).cpu().numpy(), grads[0].cpu().numpy())
    print("shards against the whole batch: %.3g" % err)
    assert err < 1e-4
    assert float((grads[1] + grads[2])[pad_mask(m)].abs().max()) == 0.0
    outs = []
    for use_graph in (False, True):
        m = build(cfg, P, "bf16", 0.2, 0.2)
        tr = FusedStosaTrainer(m, lam1, lam2, use_graph=use_graph, seed=5)
        for _ in range(4):
            tr.step(*batch)
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.ref_flat.cpu().numpy().copy()))
    print("eager loss %.7f graph loss %.7f weights %.3g" % (outs[0][0], outs[1][0], rel(outs[1][1], outs[0][1])))
    assert abs(outs[0][0] - outs[1][0]) < 1e-4 * abs(outs[0][0])
    assert rel(outs[1][1], outs[0][1]) < 5e-3


def test_ranking_at_d50():
    """full_sort(fused=True), rank_full and recommend on the padded tables against the materialised two-pass distances (predict_full), the
    way tests/test_stosa_fullrank_hip.py compares them: ranks bracketed at tol = 1e-4 of the largest distance, top-k sets equal where the
    k-th gap is clear, returned distances within tol of their ids'."""
    from adt_amd.stosa.trainer import FusedStosaTrainer
    V, L, B, k = 300, 12, 4, 5
    cfg, P, batch = make_case(50, 1, V=V, L=L, lens=(12, 7, 3, 9))
    m = build(cfg, P, "f32")
    m.eval()
    inp = batch[0]
    D = m.predict_full(inp).cpu().numpy().astype(np.float64)          # (B, item_size), two-pass
    assert D.shape == (B, V)
    tol = 1e-4 * np.abs(D).max()
    tgt = np.array([3, 17, 200, 299])
    seen = np.zeros((B, V), np.int8)
    for b in range(B):
        seen[b, inp[b][inp[b] > 0]] = 1
    rank, n_elig, top_idx, top_dist = m.rank_full(inp, tgt, seen, k)
    rank, n_elig, top_idx, top_dist = (t.cpu().numpy() for t in (rank, n_elig, top_idx, top_dist))
    for b in range(B):
        other = (seen[b] == 0) & (np.arange(V) >= 1) & (np.arange(V) != tgt[b])
        lo, hi = (other & (D[b] < D[b, tgt[b]] - tol)).sum(), (other & (D[b] < D[b, tgt[b]] + tol)).sum()
        assert int(n_elig[b]) == other.sum() and lo <= int(rank[b]) <= hi, (b, lo, int(rank[b]), hi)
        elig = (seen[b] == 0) & (np.arange(V) >= 1)
        Db = np.where(elig, D[b], np.inf)
        order = np.argsort(Db, kind="stable")
        if Db[order[k]] - Db[order[k - 1]] > 2 * tol:
            assert set(top_idx[b].tolist()) == set(order[:k].tolist()), b
        assert (np.abs(top_dist[b] - D[b, top_idx[b]]) <= tol).all() and (np.diff(top_dist[b]) >= 0).all(), b
    ids, dist = m.recommend(inp, k, seen)
    assert np.array_equal(ids.cpu().numpy(), top_idx)
    tr = FusedStosaTrainer(m, [0.1], [0.1])
    ans = tgt[:, None]
    fused, _ = tr.full_sort([(inp, seen, ans)], fused=True)
    two, _ = tr.full_sort([(inp, seen, ans)], fused=False)
    assert tr.fused_fallbacks == 0 and fused.shape == two.shape == (B, 40)
    for b in range(B):
        Db = np.where(seen[b] == 0, D[b], np.inf)
        s = np.sort(Db)
        if s[40] - s[39] > 2 * tol:
            assert set(fused[b].tolist()) == set(two[b].tolist()), b
        assert (np.abs(Db[fused[b]] - s[:40]) <= 2 * tol).all(), b          # the same distances in the same order, up to ties within tol


def test_tiled_widths_are_untouched_and_unsupported_uses_raise(monkeypatch):
    from adt_amd import ops
    from adt_amd._lib import AdtError
    from adt_amd.stosa.models import param_table
    from adt_amd.stosa.supernet import DisenDistSASupernet
    from adt_amd.stosa.trainer import FusedStosaTrainer
    calls = []
    for name in ("act_lanes_fwd", "act_lanes_bwd", "wattn_scaled_fwd", "wattn_scaled_bwd", "wattn_long_scaled_fwd", "wattn_long_scaled_bwd",
                 "wdist_bpr_lanes", "wdist_full_lanes", "wdist_pack_lanes", "layernorm_lanes_fwd", "drop_lanes", "lane_map"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    cfg, _, batch = make_case(64, 4, lens=(12, 7, 3))
    m = build(cfg, None, "bf16", 0.2, 0.2)
    assert m.lanes is None and m.ref_flat is None and m.master is m.flat and m.dp == 64 and m.hd == m.hd_pad == 16
    assert m.n_flat == sum((int(np.prod(s)) + 3) // 4 * 4 for _, s in param_table(40, 12, 64, 4, 1, 4)[0])
    assert m.P("item_mean_embeddings.weight").data_ptr() == m.item_mean_embeddings.weight.data_ptr()
    tr = FusedStosaTrainer(m, [0.2], [0.1])
    tr.step(*batch)
    m.predict_full(batch[0])
    m.recommend(batch[0], 5)
    torch.cuda.synchronize()
    assert calls == []
    m50 = build(make_case(50, 1)[0], None, "f32")          # ... and a padded width does call them
    FusedStosaTrainer(m50, [0.2], [0.1]).step(*batch)
    assert {"act_lanes_fwd", "act_lanes_bwd", "wattn_scaled_fwd", "wattn_scaled_bwd", "wdist_bpr_lanes"} <= set(calls)
    with pytest.raises(AdtError, match="kl"):
        build(make_case(50, 1)[0], None, "f32", metric="kl")
    with pytest.raises(AdtError, match="head size"):
        build(make_case(128, 1)[0], None, "f32")
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, 40, 12, 50, 1, 1, 4
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = 0.0, 0.0, 0.1, "bf16", "wasserstein"
    with pytest.raises(AdtError, match="supernet"):
        DisenDistSASupernet(a, [0.0, 0.5], [0.0, 0.5])
    m50.train()
    with pytest.raises(AdtError, match="FusedStosaTrainer"):
        m50.finetune(batch[0], batch[1])


@pytest.mark.parametrize("extra", [[], ["--device_batches", "--device_scores", "--fused_eval"]], ids=["host", "device-fused"])
def test_main_at_hidden_units_50_end_to_end(tmp_path, capsys, extra):
    """stosa/main.py --synthetic tiny --hidden_units 50 --num_heads 1: one epoch, finite metrics.  The data set's template sets the width
    itself, so the width goes through --override too; the checkpoint's name and shapes show what ran."""
    from adt_amd.stosa.main import main
    out = tmp_path / "out"
    over = {"epochs": 1, "hidden_units": 50, "num_heads": 1, "maxlen": 20, "batch_size": 32, "eval_batch_size": 48}
    main(["--dataset", "Beauty", "--data_dir", str(tmp_path / "data") + "/", "--output_dir", str(out) + "/", "--synthetic", "tiny",
          "--hidden_units", "50", "--num_heads", "1", "--epochs", "1", "--eval_set", "64", "--override", json.dumps(over)] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["epoch"] for l in lines] == [0]
    for key in ("rec_cur_loss", "auc", "valid_HIT@10", "valid_NDCG@10", "valid_MRR"):
        assert np.isfinite(lines[0][key]), (key, lines[0])
    assert 0.0 <= lines[0]["valid_MRR"] <= 1.0 and lines[0]["sequences_per_sec"] > 0
    ck = [f for f in os.listdir(out) if f.endswith(".pt")]
    assert len(ck) == 1 and "-50-" in ck[0]
    sd = torch.load(os.path.join(out, ck[0]), map_location="cpu")
    assert tuple(sd["item_mean_embeddings.weight"].shape)[1] == 50
