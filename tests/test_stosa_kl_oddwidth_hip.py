"""GPU: STOSA-ADT under distance_metric='kl' at widths the kernels pad -- hidden_units 50 (one head: 64 lanes), 100 (2 x 64), 48 (4 heads
of 12: 4 x 16), 150 (3 x 64) -- with DisenDistSAModel(..., allow_kl_lanes=True).

Kernels alone against float64 at the TRUE head size (the reference side on compact rows, the kernel side on rows widened with mean 0 /
covariance 0 pad lanes): the scaled KL attention of the three families (vector ALU, matrix cores, streamed), the lane-aware row-wise
loss, full sort and row-wise images.  Model: the three stosa_kl_w* fixtures in f32 and bf16 with the bounds of tests/test_stosa_kl_hip.py,
a dropout-on step against the numpy oracle with the KL distances swapped in, pad floats through training, checkpoints, shards, graph
replay, row-wise ranking, the untouched tiled path, the constructor's refusals and stosa/main.py end to end.

Bounds (tests/test_stosa_kl_hip.py): exact arithmetic 1e-4 outputs / 5e-4 gradients; bf16 matrix-core operands 3e-2 / 6e-2 at kernel level,
3e-2 / relative Frobenius 0.1 for the model."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import stosa_oracle as so  # noqa: E402
from tests.test_stosa_kl_hip import kl_full_ref, kl_oracle, kl_rows64, klattn_ref  # noqa: E402
from tests.test_stosa_klrow_cpu import elu1_64, images64, kl_direct64  # noqa: E402
from tests.test_stosa_oddwidth_hip import (DEV, Args, T_, _batches, _padded, close, make_case, one_pass, pad_mask, perturb, rel,  # noqa: E402
                                           seed_tensor, stored)
from tools.gen_golden_inputs import golden_err  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ["w50_h1", "w100_h2", "w48_h4"]
K = 320          # samples per compacted tensor (tools/gen_golden_stosa.py:STOSA_ODD_COMPACT)
GRADS = ("dQm", "dQc", "dKm", "dKc", "dVm", "dVc")


def load_case(tag):
    g = np.load(os.path.join(GOLD, "stosa_kl_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    return g, cfg, perturb(so.init_params(cfg, int(g["seed"])), int(g["seed"]))


def kl_args(cfg, prec, dropout=0.0, attention_dropout=0.0, metric="kl"):
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, cfg.item_size, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.num_users
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = dropout, attention_dropout, cfg.pvn_weight, prec, metric
    return a


def build(cfg, P, prec, dropout=0.0, attention_dropout=0.0, **kw):
    from adt_amd.stosa.models import DisenDistSAModel
    m = DisenDistSAModel(kl_args(cfg, prec, dropout, attention_dropout), allow_kl_lanes=True, **kw)
    if P is not None:
        m.load_numpy(P)
    return m


def bits_zero(a):
    return bool((np.ascontiguousarray(a, np.float32).view(np.uint32) == 0).all())


# ---- the scaled KL attention against float64 at the true head size --------------------------------------------------------------------
def _attn_case(H, hd, hd_pad, L, B=2):
    d, dp, T = H * hd, H * hd_pad, B * L
    live = (np.arange(dp) % hd_pad) < hd
    r = np.random.RandomState(L * 100 + hd + H)
    qm, km, vm = (r.standard_normal((T, d)).astype(np.float32) for _ in range(3))
    qc, kc, vc = (np.exp(0.5 * r.standard_normal((T, d))).astype(np.float32) for _ in range(3))
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    ids[0, : L // 3] = 0          # left padding: fully masked query rows, masked key columns
    ids[1, L // 2] = 0            # one padded key inside a sequence
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    return d, dp, T, live, (qm, qc, km, kc, vm, vc), ids, dOm, dOc


def _attn_fns(family):
    from adt_amd import ops
    return (ops.klattn_long_scaled_fwd, ops.klattn_long_scaled_bwd) if family == "long" else (ops.klattn_scaled_fwd, ops.klattn_scaled_bwd)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("family,prec,H,hd,hd_pad,L", [("valu", None, 4, 12, 16, 12), ("mfma", "f32", 4, 12, 16, 12), ("mfma", "bf16", 4, 12, 16, 12),
                                                       ("mfma", "f32", 2, 20, 32, 37), ("valu", None, 1, 50, 64, 12),
                                                       ("long", "f32", 1, 50, 64, 150), ("long", "bf16", 1, 50, 64, 150),
                                                       ("long", "f32", 4, 12, 16, 300)])
def test_scaled_kl_attention_against_the_true_head_size(family, prec, H, hd, hd_pad, L, p):
    """adt_klattn_scaled_* (prec None: vector ALU), adt_klattn_mfma_scaled_* (hd_pad 16 / 32, L <= 128) and adt_klattn_long_scaled_* on heads
    widened with mean 0 / covariance 0 pad lanes, scale = 1 / sqrt(hd), b_offset 5, against klattn_ref on the compact rows.  Every gradient
    buffer starts as NaN.  Live lanes: the bounds of test_kl_attention_kernels; pad lanes of Om, Oc and all six gradients: exactly 0.0;
    nothing NaN or inf, LSE included."""
    from adt_amd import ops
    B = 2
    d, dp, T, live, t6, ids, dOm, dOc = _attn_case(H, hd, hd_pad, L, B)
    pk = None if prec is None else {"f32": ops.PREC_F32, "bf16": ops.PREC_BF16}[prec]
    tol_f, tol_g = (3e-2, 6e-2) if prec == "bf16" else (1e-4, 5e-4)
    seed, site, b_off = 2468, 16, 5
    om, oc, grads = klattn_ref(t6, ids, B, H, L, p, seed, site, b_off, dOm, dOc)
    g = [T_(_padded(x, live, dp)) for x in t6]
    kid, sd, scale = T_(ids.reshape(-1)), seed_tensor(seed), 1.0 / np.sqrt(hd)
    fwd, bwd = _attn_fns(family)
    Om, Oc, LSE = fwd(*g, kid, B, H, L, scale, hd, p, sd, site, b_off, prec=pk)
    hOm, hOc, hL = Om.cpu().numpy(), Oc.cpu().numpy(), LSE.cpu().numpy()
    assert np.isfinite(hOm).all() and np.isfinite(hOc).all() and np.isfinite(hL).all()
    close(hOm[:, live], om, tol_f, "Om")
    close(hOc[:, live], oc, tol_f, "Oc")
    assert not np.any(hOm[:, ~live]) and not np.any(hOc[:, ~live])
    outs = [torch.full((T, dp), float("nan"), device=DEV) for _ in range(6)]
    bwd(*g, kid, Om, Oc, LSE, T_(_padded(dOm, live, dp)), T_(_padded(dOc, live, dp)), B, H, L, scale, hd, p, sd, site, b_off, out=outs, prec=pk)
    torch.cuda.synchronize()
    for name, got, want in zip(GRADS, outs, grads):
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), name
        close(got[:, live], want, tol_g, name)
        assert not np.any(got[:, ~live]), name


@pytest.mark.parametrize("prec", [None, "f32"])
def test_scaled_kl_cross_attention_strided_outputs(prec):
    """tests/test_stosa_kl_hip.py::test_kl_cross_attention_strided_outputs on padded heads (4 x 12 in 4 x 16 lanes): query and key / value
    rows from different tensors, gradients into strided views of NaN-filled shared buffers, dKc / dQc accumulated across the two passes."""
    from adt_amd import ops
    pk = None if prec is None else ops.PREC_F32
    r = np.random.RandomState(5)
    B, H, L, hd, hd_pad = 2, 4, 24, 12, 16
    d, dp, T = H * hd, H * hd_pad, B * L
    live = (np.arange(dp) % hd_pad) < hd
    dec, enc = r.standard_normal((T, 3 * d)).astype(np.float32), r.standard_normal((T, 3 * d)).astype(np.float32)
    decc, encc = np.exp(0.4 * dec).astype(np.float32), np.exp(0.4 * enc).astype(np.float32)
    t6 = (dec[:, :d], decc[:, :d], enc[:, d:2 * d], encc[:, d:2 * d], enc[:, 2 * d:], encc[:, 2 * d:])
    ids = r.randint(1, 9, size=(B, L)).astype(np.int32)
    ids[1, :7] = 0
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    om, oc, grads = klattn_ref(t6, ids, B, H, L, 0.0, 1, 16, 0, dOm, dOc)
    wide = lambda x: np.concatenate([_padded(x[:, k * d:(k + 1) * d], live, dp) for k in range(3)], 1)
    Dm, Dc, Em, Ec = (T_(wide(x)) for x in (dec, decc, enc, encc))
    args = (Dm[:, :dp], Dc[:, :dp], Em[:, dp:2 * dp], Ec[:, dp:2 * dp], Em[:, 2 * dp:], Ec[:, 2 * dp:])
    kid, sd, scale = T_(ids.reshape(-1)), seed_tensor(1), 1.0 / np.sqrt(hd)
    Om, Oc, LSE = ops.klattn_scaled_fwd(*args, kid, B, H, L, scale, hd, 0.0, sd, 16, 0, prec=pk)
    close(Om.cpu().numpy()[:, live], om, 1e-4, "Om")
    close(Oc.cpu().numpy()[:, live], oc, 1e-4, "Oc")
    gm = torch.full((T, 3 * dp), float("nan"), device=DEV)
    gc = torch.full((T, 3 * dp), float("nan"), device=DEV)
    outs = (gm[:, :dp], gc[:, :dp], gm[:, dp:2 * dp], gc[:, dp:2 * dp], gm[:, 2 * dp:], gc[:, 2 * dp:])
    ops.klattn_scaled_bwd(*args, kid, Om, Oc, LSE, T_(_padded(dOm, live, dp)), T_(_padded(dOc, live, dp)), B, H, L, scale, hd, 0.0, sd, 16, 0,
                          out=outs, prec=pk)
    torch.cuda.synchronize()
    for name, got, want in zip(GRADS, outs, grads):
        got = got.cpu().numpy()
        close(got[:, live], want, 5e-4, name)
        assert bits_zero(got[:, ~live]), name


@pytest.mark.parametrize("family", ["valu", "mfma", "long"])
def test_scaled_kl_entry_points_equal_the_plain_ones_at_an_unpadded_head(family):
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
    plain, prec = {"valu": ((ops.klattn_fwd, ops.klattn_bwd), None), "mfma": ((ops.klattn_fwd, ops.klattn_bwd), ops.PREC_BF16),
                   "long": ((ops.klattn_long_fwd, ops.klattn_long_bwd), ops.PREC_BF16)}[family]
    scaled = _attn_fns(family)
    a = plain[0](qm, qc, km, kc, vm, vc, kid, B, H, L, p, sd, 16, 1, prec=prec)
    b = scaled[0](qm, qc, km, kc, vm, vc, kid, B, H, L, 0.25, hd, p, sd, 16, 1, prec=prec)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ga = plain[1](qm, qc, km, kc, vm, vc, kid, *a, dOm, dOc, B, H, L, p, sd, 16, 1, prec=prec)
    gb = scaled[1](qm, qc, km, kc, vm, vc, kid, *b, dOm, dOc, B, H, L, 0.25, hd, p, sd, 16, 1, prec=prec)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


# ---- the lane-aware distances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,V", [(7, 40), (3, 2)])          # E does not divide V; E > V
@pytest.mark.parametrize("H,hd,hd_pad", [(4, 12, 16), (1, 50, 64)])
def test_lane_aware_kl_distances_against_float64(H, hd, hd_pad, E, V):
    """adt_kldist_bpr_lanes / adt_kldist_full_lanes / adt_klrow_pack_lanes against test_kl_bpr_and_full_sort_kernels' float64 reference over
    the TRUE d (compact columns): loss and distances 1e-4, gradients 5e-4.  Pad lanes of dSm / dSc, of the table gradients and of both
    image halves are bit-zero; a target whose negative is row 0 sends nothing to row 0."""
    from adt_amd import ops
    r = np.random.RandomState(E * 1000 + V + hd)
    B, L, pvn_w = 5, 12, 0.3
    d, dp, T = H * hd, H * hd_pad, B * L
    live = (np.arange(dp) % hd_pad) < hd
    lanes = (H, hd, hd_pad)
    Em, Ec = (0.3 * r.standard_normal((V, d))).astype(np.float32), (0.3 * r.standard_normal((V, d))).astype(np.float32)
    sm = (0.3 * r.standard_normal((T, d))).astype(np.float32)
    sc = np.exp(0.2 * r.standard_normal((T, d))).astype(np.float32)
    pos, neg = r.randint(1, V, size=T), r.randint(1, V, size=T)
    pos[:4] = 0
    neg[:4] = 0
    neg[7] = 0                          # a target token whose negative is the padding row: no gradient into row 0
    tEm, tEc, tsm, tsc = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (Em, Ec, sm, sc))
    elu1 = lambda x: torch.nn.functional.elu(x) + 1
    pe, ne = torch.from_numpy(pos), torch.from_numpy(neg)
    pm, pc, nm, nc = tEm[pe], elu1(tEc[pe]), tEm[ne], elu1(tEc[ne])
    pos_l, neg_l, pvn = kl_rows64(tsm, tsc, pm, pc), kl_rows64(tsm, tsc, nm, nc), kl_rows64(pm, pc, nm, nc)
    ist = (pe > 0).double()
    n = ist.sum()
    loss = torch.sum(-torch.log(torch.sigmoid(neg_l - pos_l + 1e-24)) * ist) / n
    pvn_loss = pvn_w * torch.sum(torch.clamp(pos_l - pvn, 0) * ist) / n
    auc = float((torch.sum(((torch.sign(neg_l - pos_l) + 1) / 2) * ist) / n).detach())
    (loss + pvn_loss).backward()
    gEm, gEc = tEm.grad.clone(), tEc.grad.clone()
    gEm[0] = 0
    gEc[0] = 0                          # padding_idx = 0 (nn.Embedding): row 0 receives no gradient
    inv = torch.tensor([1.0 / float(n)], device=DEV, dtype=torch.float32)
    dEm, dEc = torch.zeros(V, dp, device=DEV), torch.zeros(V, dp, device=DEV)
    loss3 = torch.zeros(192, device=DEV)
    pEm, pEc, psm, psc = (_padded(x, live, dp) for x in (Em, Ec, sm, sc))
    dSm, dSc = ops.kldist_bpr_lanes(T_(psm), T_(psc), T_(pEm), T_(pEc), T_(pos.astype(np.int32)), T_(neg.astype(np.int32)), pvn_w, inv, dEm, dEc,
                                    loss3, lanes)
    torch.cuda.synchronize()
    l3 = loss3.view(3, 64).sum(1).cpu().numpy()
    print("bpr %.7f (%.7f) pvn %.7f (%.7f) auc %.7f (%.7f)" % (l3[0], float(loss), l3[1], float(pvn_loss), l3[2], auc))
    assert np.isfinite(l3).all()
    assert abs(l3[0] - float(loss)) < 1e-4 * abs(float(loss)) and abs(l3[1] - float(pvn_loss)) < 1e-4 * max(abs(float(pvn_loss)), 1e-6)
    assert abs(l3[2] - auc) < 1e-6
    for nm_, got, want in (("dSm", dSm, tsm.grad), ("dSc", dSc, tsc.grad), ("dEm", dEm, gEm), ("dEc", dEc, gEc)):
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), nm_
        close(got[:, live], want.numpy(), 5e-4, nm_)
        assert bits_zero(got[:, ~live]), nm_
    assert bits_zero(dEm[0].cpu().numpy()) and bits_zero(dEc[0].cpu().numpy())
    # full sort: E users (the eval batch) against all V items, the reference's chunking by E
    um, uc = sm[:E], sc[:E]
    got = ops.kldist_full_lanes(T_(psm[:E]), T_(psc[:E]), T_(pEm), T_(pEc), V, lanes).cpu().numpy()
    close(got, kl_full_ref(um, uc, Em, Ec), 1e-4, "kldist_full_lanes")
    # the row-wise images: KL[u][v] = nu[u] - (A[u] . W[v] + bias[v]) over the live lanes, zero pad columns on both sides
    W, bias = ops.klrow_pack_lanes(T_(pEm), T_(pEc), True, lanes)
    A, nu = ops.klrow_pack_lanes(T_(psm[:E]), T_(psc[:E]), False, lanes)
    W, bias, A, nu = (t.cpu().numpy() for t in (W, bias, A, nu))
    ci = elu1_64(Ec.astype(np.float64))
    A64, nu64, W64, b64 = images64(um.astype(np.float64), uc.astype(np.float64), Em.astype(np.float64), ci)
    for nm_, got2, want2 in (("A", A, A64), ("W", W, W64)):
        assert got2.shape[1] == 2 * dp and np.isfinite(got2).all()
        close(np.concatenate([got2[:, :dp][:, live], got2[:, dp:][:, live]], 1), want2, 1e-4, "image " + nm_)
        assert bits_zero(got2[:, :dp][:, ~live]) and bits_zero(got2[:, dp:][:, ~live]), nm_
    close(nu, nu64, 1e-4, "nu")
    close(bias, b64, 1e-4, "bias")
    D = kl_direct64(um.astype(np.float64), uc.astype(np.float64), Em.astype(np.float64), ci)
    close(nu[:, None] - (A.astype(np.float64) @ W.astype(np.float64).T + bias[None]), D, 1e-4, "distance from the images")


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_kl_finetune_predict_and_loss_parts_match_reference(tag, prec):
    from adt_amd.wide import padded_layout
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    d, H = cfg.hidden_units, cfg.num_heads
    assert m.lanes == (H,) + padded_layout(d, H)[:2] and m.distance_metric == "kl" and m.ref_flat is not None
    m.eval()
    B, L = g["input_ids"].shape
    mo, co, _, margins, enc_in, enc_rec, dec_out = m.finetune(g["input_ids"], g["dec_ids"], np.zeros(B, np.int64))
    tol = 1e-4 if prec == "f32" else 3e-2
    assert tuple(mo.shape) == (B, L, d)
    figs = {"mean_out": golden_err(mo.cpu().numpy(), g, "mean_out", K), "cov_out": golden_err(co.cpu().numpy(), g, "cov_out", K)}
    for i in range(cfg.num_layers):
        for nm, pair in (("enc_in", enc_in[i]), ("rec", enc_rec[i]), ("dec_out", dec_out[i])):
            for t, which in enumerate(("mean", "cov")):
                figs["%s_%s_%d" % (nm, which, i)] = golden_err(pair[t].cpu().numpy(), g, "%s_%s_%d" % (nm, which, i), K)
    figs["full_dist"] = golden_err(m.predict_full(g["input_ids"], g["dec_ids"]).cpu().numpy(), g, "full_dist", K)
    print(tag, prec, figs)
    for k, e in figs.items():
        assert e < tol, (k, e)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    loss, parts = one_pass(m, cfg, tuple(g[k] for k in ("input_ids", "dec_ids", "pos_ids", "neg_ids")), lam1, lam2)
    print("bpr %.7f (%.7f) pvn %.7f (%.7f) auc %.7f (%.7f) loss %.7f (%.7f)" % (parts[0], g["bpr"], parts[1], g["pvn"], parts[2], g["auc"], loss, g["loss"]))
    if prec == "f32":          # the loss parts in fp32 (tests/test_stosa_kl_hip.py::test_kl_train_step_matches_reference_fp32)
        assert abs(parts[0] - float(g["bpr"])) < 1e-4 * abs(float(g["bpr"]))
        assert abs(parts[1] - float(g["pvn"])) < 1e-4 * max(abs(float(g["pvn"])), 1e-5)
        assert abs(parts[2] - float(g["auc"])) < 1e-5
        assert abs(loss - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    else:
        assert np.isfinite(loss)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_kl_gradients_match_reference(tag, prec):
    """tests/test_stosa_kl_hip.py::test_kl_gradients_match_reference on the stored entries (f32: 5e-4 of max(|G|, 1e-3 gmax); bf16: relative
    Frobenius 0.1); the pad floats of the gradient are exact zeros."""
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    one_pass(m, cfg, tuple(g[k] for k in ("input_ids", "dec_ids", "pos_ids", "neg_ids")), lam1, lam2)
    none = set(str(x) for x in g["grad_none"])
    assert none == set(k for k in P if so.is_unused(k))
    gmax = max(float(np.abs(stored(g, "grad." + k, np.zeros(P[k].shape))[1]).max()) for k in P if k not in none)
    worst = ("", 0.0)
    for k in P:
        full = m.GR(k).cpu().numpy()
        assert full.shape == P[k].shape and np.isfinite(full).all(), k
        if k in none:
            assert np.all(full == 0.0), k
            continue
        got, want = stored(g, "grad." + k, full)
        if prec == "f32":
            e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-3 * gmax)
            worst = max(worst, (k, e), key=lambda kv: kv[1])
            assert e < 5e-4, (k, e)
        else:
            e = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-3 * gmax * np.sqrt(want.size))
            worst = max(worst, (k, e), key=lambda kv: kv[1])
            assert e < 0.1, (k, e)
    print(tag, prec, "worst", worst)
    assert float(m.flat_grad[pad_mask(m)].abs().max()) == 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_kl_weights_after_one_and_three_steps_fp32(tag):
    """The bounds of tests/test_stosa_oddwidth_hip.py::test_weights_after_one_and_three_steps_fp32 (step 1: those of
    tests/test_stosa_kl_hip.py::test_kl_train_step_matches_reference_fp32)."""
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
                assert diff.max() == 0.0, k
                continue
            big = np.abs(stored(g, "grad." + k, np.zeros(P[k].shape))[1]) > 1e-5
            worst = max(worst, diff[big].max() / lr if big.any() else 0.0)
            assert (diff[big].max() if big.any() else 0.0) < (0.05 if step == 1 else 0.3) * lr, (step, k)
            assert diff.max() < (1.01 if step == 1 else 3.03) * lr, (step, k)
        print(tag, "step", step, "worst well-conditioned entry: %.3g lr" % worst)
    assert torch.equal(m.compact(m.flat), m.ref_flat)


# ---- dropout on ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(50, 1), (48, 4), (150, 3)])
def test_kl_dropout_step_matches_oracle(d, H):
    """tests/test_stosa_kl_hip.py::test_kl_training_step_with_dropout_matches_oracle at padded widths, its bounds (loss 1e-4, gradients
    5e-4 * max(|G|, 1e-3 gmax)).  One full row, one mostly padded row and one all-padding row; (150, 3) is d_pad 192."""
    cfg, P, batch = make_case(d, H, nl=2 if d == 50 else 1)
    cfg.dropout, cfg.attention_dropout = 0.3, 0.3
    m = build(cfg, P, "f32", 0.3, 0.3)
    assert m.lanes is not None
    lam1, lam2 = [0.25, 0.1][:cfg.num_layers], [0.15, 0.05][:cfg.num_layers]
    got, _ = one_pass(m, cfg, batch, lam1, lam2, seed=9001)
    with kl_oracle():
        loss, parts, G = so.loss_and_grads(P, cfg, *batch, lam1, lam2, training=True, seed=9001)
    print("loss %.7f (oracle %.7f)" % (got, loss))
    assert abs(got - loss) < 1e-4 * abs(loss)
    gmax = max(float(np.abs(v).max()) for v in G.values() if v is not None)
    errs = {k: np.abs(m.GR(k).cpu().numpy() - G[k]).max() / max(np.abs(G[k]).max(), 1e-3 * gmax) for k in P if G[k] is not None}
    print("worst", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    for k, e in errs.items():
        assert e < 5e-4, (k, e)
    assert float(m.flat_grad[pad_mask(m)].abs().max()) == 0.0


# ---- the padded layout through training, checkpoints and data parallelism ---------------------------------------------------------------
def _trainer(d, H, seed, prec="bf16", p=0.3, use_graph=False, V=60, L=12, nl=1, wd=1e-3):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    torch.manual_seed(seed)
    cfg = so.Cfg(V, L, d, H, nl, num_users=4, pvn_weight=0.1)
    m = build(cfg, None, prec, p, p)
    return m, FusedStosaTrainer(m, [0.2] * nl, [0.1] * nl, lr=1e-3, weight_decay=wd, use_graph=use_graph, seed=5)


@pytest.mark.parametrize("d,H", [(50, 1), (48, 4), (150, 3)])
def test_kl_pad_floats_stay_zero_through_training(d, H):
    """Five dropout-on steps: every float of the flat buffer, the gradient and both Adam moments that no reference element maps to is
    bit-zero; the weights moved and they and the loss are finite."""
    m, tr = _trainer(d, H, 3)
    w0 = m.ref_flat.clone()
    pads = pad_mask(m)
    assert int(pads.sum()) > 0
    for b in _batches(5):
        tr.step(*b)
        assert np.isfinite(float(tr.loss()))
    torch.cuda.synchronize()
    for nm, t in (("flat", m.flat), ("flat_grad", m.flat_grad), ("exp_avg", tr.m), ("exp_avg_sq", tr.v)):
        assert (t[pads].view(torch.int32) == 0).all(), nm
        assert bool(torch.isfinite(t).all()), nm
    assert float((m.ref_flat - w0).abs().max()) > 1e-3
    assert torch.equal(m.compact(m.flat), m.ref_flat)


def test_kl_checkpoint_holds_reference_shapes_only(tmp_path):
    from adt_amd import checkpoint as ck
    from adt_amd.stosa.models import param_table
    d, H = 50, 1
    m1, tr1 = _trainer(d, H, 11)
    ref = dict(param_table(60, 12, d, H, 1, 4)[0])
    batches = _batches(2)
    for b in batches:
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
    assert torch.equal(tr2.m, tr1.m) and torch.equal(tr2.v, tr1.v) and tr2.nstep == 2


def test_kl_two_shards_and_graph_replay():
    """tests/test_stosa_kl_hip.py::test_kl_dp_shard_and_graph_replay at (50, 1), its bounds: two shards (b_offset 0 and 1 of a batch of 2,
    global normalisers and dropout indices) sum to the whole batch's gradient (1e-4), pad floats included; four graph-replayed steps equal
    four eager ones (loss 1e-4, weights 5e-3)."""
    from adt_amd.stosa.trainer import FusedStosaTrainer
    cfg, P, batch = make_case(50, 1, lens=(12, 7))
    cfg.dropout, cfg.attention_dropout = 0.2, 0.2
    lam1, lam2 = [0.3], [0.2]
    nt = int((batch[2] > 0).sum())
    m = build(cfg, P, "f32", 0.2, 0.2)
    grads = []
    for lo, hi in ((0, 2), (0, 1), (1, 2)):
        one_pass(m, cfg, batch, lam1, lam2, lo, hi, seed=31337, B_global=2, nt=nt)
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


def test_kl_rowwise_ranking_at_d50():
    """rank_full(rowwise=True) and recommend on the padded tables against the materialised row-wise divergences (kl_rows64 in float64 on the
    live lanes of the model's own last states and the reference-shaped tables), the way tests/test_stosa_oddwidth_hip.py::test_ranking_at_d50
    compares them: ranks bracketed at tol = 1e-4 of the largest distance, top-k sets equal where the k-th gap is clear, distances within tol."""
    V, L, B, k = 300, 12, 4, 5
    cfg, P, batch = make_case(50, 1, V=V, L=L, lens=(12, 7, 3, 9))
    m = build(cfg, P, "f32")
    m.eval()
    inp = batch[0]
    sm, sc = m._last_state(inp)
    live = (np.arange(m.dp) % m.hd_pad) < m.hd
    sm, sc = sm.cpu().numpy(), sc.cpu().numpy()
    assert bits_zero(sm[:, ~live]) and bits_zero(sc[:, ~live])
    tm, tc = torch.tensor(sm[:, live], dtype=torch.float64), torch.tensor(sc[:, live], dtype=torch.float64)
    Em = torch.tensor(m.R("item_mean_embeddings.weight").cpu().numpy(), dtype=torch.float64)
    Ec = torch.nn.functional.elu(torch.tensor(m.R("item_cov_embeddings.weight").cpu().numpy(), dtype=torch.float64)) + 1
    D = np.stack([kl_rows64(tm[b:b + 1].expand(V, -1), tc[b:b + 1].expand(V, -1), Em, Ec).numpy() for b in range(B)])
    assert D.shape == (B, V) and np.isfinite(D).all()
    tol = 1e-4 * np.abs(D).max()
    tgt = np.array([3, 17, 200, 299])
    seen = np.zeros((B, V), np.int8)
    for b in range(B):
        seen[b, inp[b][inp[b] > 0]] = 1
    rank, n_elig, top_idx, top_dist = (t.cpu().numpy() for t in m.rank_full(inp, tgt, seen, k, rowwise=True))
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
    ids, dist = m.recommend(inp, k, seen, rowwise=True)
    assert np.array_equal(ids.cpu().numpy(), top_idx) and np.isfinite(dist.cpu().numpy()).all()
    W, bias = m.kl_row_image()
    W = W.cpu().numpy()
    assert W.shape == (V, 2 * m.dp) and bits_zero(W[:, :m.dp][:, ~live]) and bits_zero(W[:, m.dp:][:, ~live])


NEW_OPS = ("klattn_scaled_fwd", "klattn_scaled_bwd", "klattn_long_scaled_fwd", "klattn_long_scaled_bwd", "kldist_bpr_lanes", "kldist_full_lanes",
           "klrow_pack_lanes")


def test_tiled_kl_path_is_untouched_and_refusals_stay(monkeypatch):
    from adt_amd import ops
    from adt_amd._lib import AdtError
    from adt_amd.stosa.models import DisenDistSAModel
    from adt_amd.stosa.supernet import DisenDistSASupernet
    from adt_amd.stosa.trainer import FusedStosaTrainer
    calls = []
    for name in NEW_OPS + ("act_lanes_fwd", "act_lanes_bwd", "lane_map"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    cfg, _, batch = make_case(64, 4, lens=(12, 7, 3))
    m = build(cfg, None, "bf16", 0.2, 0.2)          # the flag changes nothing at a tiled width
    assert m.lanes is None and m.ref_flat is None and m.dp == 64 and m.hd == m.hd_pad == 16
    FusedStosaTrainer(m, [0.2], [0.1]).step(*batch)
    m.predict_full(batch[0])
    m.rank_full(batch[0], None, None, 5, rowwise=True)
    torch.cuda.synchronize()
    assert calls == []
    c50 = make_case(50, 1)[0]
    m50 = build(c50, None, "f32")                   # ... and a padded width does call them
    FusedStosaTrainer(m50, [0.2], [0.1]).step(*batch)
    m50.predict_full(batch[0])
    m50.rank_full(batch[0], None, None, 5, rowwise=True)
    assert {"klattn_scaled_fwd", "klattn_scaled_bwd", "kldist_bpr_lanes", "kldist_full_lanes", "klrow_pack_lanes"} <= set(calls)
    # the constructor: opt-in, and the other refusals stay
    with pytest.raises(AdtError, match="allow_kl_lanes=True") as ei:
        DisenDistSAModel(kl_args(c50, "f32"))
    msg = str(ei.value)
    assert "kl" in msg and "d=50" in msg and "H=1" in msg and "d_pad=64" in msg
    with pytest.raises(AdtError, match="head size"):
        build(make_case(128, 1)[0], None, "f32")
    with pytest.raises(AdtError, match="supernet"):
        DisenDistSASupernet(kl_args(c50, "bf16"), [0.0, 0.5], [0.0, 0.5], allow_kl=True)
    m50.train()
    with pytest.raises(AdtError, match="FusedStosaTrainer"):
        m50.finetune(batch[0], batch[1])
    with pytest.raises(AdtError):
        m50.rank_full(batch[0], None, None, 5)          # the fused (non-row-wise) ranking under kl


@pytest.mark.parametrize("extra", [[], ["--device_batches", "--device_scores", "--rowwise_eval"]], ids=["host", "device-rowwise"])
def test_main_kl_at_hidden_units_50_end_to_end(tmp_path, capsys, extra):
    """stosa/main.py --synthetic tiny --distance_metric kl --hidden_units 50 --num_heads 1: one epoch, finite metrics."""
    from adt_amd.stosa.main import main
    out = tmp_path / "out"
    over = {"epochs": 1, "hidden_units": 50, "num_heads": 1, "maxlen": 20, "batch_size": 32, "eval_batch_size": 48, "distance_metric": "kl"}
    main(["--dataset", "Beauty", "--data_dir", str(tmp_path / "data") + "/", "--output_dir", str(out) + "/", "--synthetic", "tiny",
          "--distance_metric", "kl", "--hidden_units", "50", "--num_heads", "1", "--epochs", "1", "--eval_set", "64",
          "--override", json.dumps(over)] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["epoch"] for l in lines] == [0]
    for key in ("rec_cur_loss", "auc", "valid_HIT@10", "valid_NDCG@10", "valid_MRR"):
        assert np.isfinite(lines[0][key]), (key, lines[0])
    assert 0.0 <= lines[0]["valid_MRR"] <= 1.0 and lines[0]["sequences_per_sec"] > 0
    ck = [f for f in os.listdir(out) if f.endswith(".pt")]
    assert len(ck) == 1 and "-50-" in ck[0]
    sd = torch.load(os.path.join(out, ck[0]), map_location="cpu")
    assert tuple(sd["item_mean_embeddings.weight"].shape)[1] == 50
