"""STOSA-ADT with distance_metric='kl' on the HIP path (adt_klattn.cuh through the C ABI).

Kernel level: the KL attention (forward and all six gradients), the row-wise KL BPR loss and the chunked full-sort score against
a float64 torch restatement of the reference's arithmetic (stosa/modules.py:45-70, trainer.py:358-391, :481-511) with its
broadcast quirks.  Model level: the four stosa_kl_* fixtures recorded from the imported reference (tools/gen_golden_stosa.py
--metric kl; compacted: tensors above 2048 entries are checked on their norm and 1024 strided samples), a dropout-on step
against the numpy oracle with the KL distances swapped in, the fused trainer, and the reference's loop body under autograd.

Tolerances: exact arithmetic (vector-ALU KL kernels, exact-fp32 MFMA) 1e-4 outputs / 5e-4 gradients; bf16 operands (the dense layers
and, where it covers the shape, the matrix-core KL attention) 3e-2 / 6e-2 at kernel level and 3e-2 / relative Frobenius 0.1 for the
model, as in test_stosa_hip.py."""
import contextlib
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import stosa_oracle as so, tape as tp  # noqa: E402
from tools.gen_golden_inputs import sample_idx  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASK = np.float32(-2.0 ** 32 + 1)
TAGS = ["small", "l2h2", "h1", "cfg5_beauty"]


def dev():
    return torch.device("cuda:0")


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


# ---- float64 restatement of the reference's KL arithmetic ---------------------------------------------------------------
def kl_matmul64(m1, c1, m2, c2):
    """kl_distance_matmul (stosa/modules.py:52-70) with log(prod) as sum(log): (..., n, hd) x (..., n, hd) -> (..., n, n)."""
    hd = m1.shape[-1]
    logdet = torch.log(c2).sum(-1).unsqueeze(-2) - torch.log(c1).sum(-1).unsqueeze(-1)
    mean = torch.matmul((m1 - m2) ** 2, (1.0 / c2).transpose(-1, -2))
    trace = torch.matmul(1.0 / c2, c1.transpose(-1, -2))
    return (logdet + mean + trace - hd) / 2


def kl_rows64(m1, c1, m2, c2):
    """kl_distance (stosa/modules.py:45-50), row-wise."""
    return (torch.sum(c1 / c2, -1) + torch.sum((m2 - m1) / c2 * (m2 - m1), -1) - m1.shape[1]
            + (torch.log(c2).sum(-1) - torch.log(c1).sum(-1))) / 2


def klattn_ref(t6, ids, B, H, L, p, seed, site, b_off, dOm, dOc):
    """DistAttention's score / softmax / dropout / contexts in float64; the additive mask rounds in fp32 as in the reference
    (scores + (-2^32 + 1) of a fully masked row collapse to one value), with gradient 1 through it."""
    d = t6[0].shape[1]
    hd = d // H
    vs = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in t6]
    qm, qc, km, kc, vm, vc = [v.view(B, L, H, hd).permute(0, 2, 1, 3) for v in vs]
    s = -kl_matmul64(qm, qc, km, kc) / math.sqrt(hd)
    masked = torch.from_numpy(np.broadcast_to(so._mask(ids) != 0, (B, H, L, L)).copy())
    rounded = (s.detach().float() + torch.tensor(MASK)).double()
    s = torch.where(masked, s + (rounded - s).detach(), s)
    keep = torch.from_numpy(tp.dropout(tp.const(np.ones((B, H, L, L), np.float32)), p, seed, site, tp.idx_attn(B, H, L, b_off)).v).double()
    pr = torch.softmax(s, -1) * keep
    om = torch.matmul(pr, vm).permute(0, 2, 1, 3).reshape(B * L, d)
    oc = torch.matmul(pr * pr, vc).permute(0, 2, 1, 3).reshape(B * L, d)
    ((om * torch.from_numpy(dOm).double()).sum() + (oc * torch.from_numpy(dOc).double()).sum()).backward()
    return om.detach().numpy(), oc.detach().numpy(), [v.grad.numpy() for v in vs]


def kl_full_ref(sm, sc, Em, Ec):
    """kl_predict_full (stosa/trainer.py:481-511): pad the items to a multiple of E = len(sm), chunk by E."""
    E, V, d = sm.shape[0], Em.shape[0], Em.shape[1]
    pad = E - V % E
    sm, sc = torch.tensor(sm, dtype=torch.float64), torch.tensor(sc, dtype=torch.float64)
    cm = torch.cat((torch.tensor(Em, dtype=torch.float64), torch.zeros(pad, d, dtype=torch.float64)))
    cc = torch.cat((torch.nn.functional.elu(torch.tensor(Ec, dtype=torch.float64)) + 1, torch.ones(pad, d, dtype=torch.float64)))
    out = torch.cat([kl_matmul64(sm, sc, cm[s0:s0 + E], cc[s0:s0 + E]) for s0 in range(0, cm.shape[0], E)], 1)
    return out[:, :V].numpy()


# ---- kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [None, "f32", "bf16"])
@pytest.mark.parametrize("B,H,L,hd,p", [(3, 4, 20, 16, 0.0), (2, 4, 100, 16, 0.3), (2, 2, 37, 32, 0.3), (2, 1, 100, 64, 0.2),
                                        (2, 2, 150, 16, 0.2), (1, 2, 200, 32, 0.0), (2, 1, 9, 64, 0.0)])
def test_kl_attention_kernels(B, H, L, hd, p, prec):
    """prec None: the exact vector-ALU kernels (adt_klattn.cuh); "f32" / "bf16": the matrix-core kernels (adt_wattn_mfma.cuh with the
    KL score) where they cover the shape (hd 16 / 32, L <= 128), the vector-ALU kernels elsewhere.  Bounds: exact arithmetic 1e-4 /
    5e-4 (outputs / gradients), bf16 operands 3e-2 / 6e-2 (the Wasserstein attention's bf16 bounds)."""
    from adt_amd import ops
    pk = None if prec is None else {"f32": ops.PREC_F32, "bf16": ops.PREC_BF16}[prec]
    mfma = prec is not None and hd in (16, 32) and L <= 128
    tol_f, tol_g = (3e-2, 6e-2) if prec == "bf16" and mfma else (1e-4, 5e-4)
    r = np.random.RandomState(B * 100 + L + hd)
    d = H * hd
    T = B * L
    qm, km, vm = (r.standard_normal((T, d)).astype(np.float32) for _ in range(3))
    qc, kc, vc = (np.exp(0.5 * r.standard_normal((T, d))).astype(np.float32) for _ in range(3))
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    ids[0, : L // 3] = 0          # left padding: fully masked query rows (uniform attention, gradient kept), masked key columns
    if B > 1:
        ids[1, L // 2] = 0        # one padded key inside a sequence
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    seed, site, b_off = 2468, 16, 5
    om, oc, grads = klattn_ref((qm, qc, km, kc, vm, vc), ids, B, H, L, p, seed, site, b_off, dOm, dOc)
    sd = torch.tensor([seed], device=dev(), dtype=torch.int32)
    g = [T_(x) for x in (qm, qc, km, kc, vm, vc)]
    kid = T_(ids.reshape(-1))
    Om, Oc, LSE = ops.klattn_fwd(*g, kid, B, H, L, p, sd, site, b_off, prec=pk)
    assert rel(Om.cpu().numpy(), om) < tol_f and rel(Oc.cpu().numpy(), oc) < tol_f
    assert np.isfinite(LSE.cpu().numpy()).all()
    outs = ops.klattn_bwd(*g, kid, Om, Oc, LSE, T_(dOm), T_(dOc), B, H, L, p, sd, site, b_off, prec=pk)
    for name, got, want in zip(("dQm", "dQc", "dKm", "dKc", "dVm", "dVc"), outs, grads):
        assert rel(got.cpu().numpy(), want) < tol_g, name


@pytest.mark.parametrize("prec", [None, "f32"])
def test_kl_cross_attention_strided_outputs(prec):
    """Decoder-style call: query and key/value rows from different tensors, gradients into strided views of shared buffers (the
    model's layout), dKc / dQc accumulated across the two passes; vector-ALU (None) and exact matrix-core ("f32") kernels."""
    from adt_amd import ops
    pk = None if prec is None else ops.PREC_F32
    r = np.random.RandomState(5)
    B, H, L, hd = 2, 4, 24, 16
    d, T = H * hd, B * L
    dec = r.standard_normal((T, 3 * d)).astype(np.float32)
    enc = r.standard_normal((T, 3 * d)).astype(np.float32)
    decc, encc = np.exp(0.4 * dec), np.exp(0.4 * enc)
    qm, km, vm = dec[:, :d], enc[:, d:2 * d], enc[:, 2 * d:]
    qc, kc, vc = decc[:, :d], encc[:, d:2 * d], encc[:, 2 * d:]
    ids = r.randint(1, 9, size=(B, L)).astype(np.int32)
    ids[1, :7] = 0
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    om, oc, grads = klattn_ref((qm, qc, km, kc, vm, vc), ids, B, H, L, 0.0, 1, 16, 0, dOm, dOc)
    Dm, Ec = T_(dec), T_(enc)
    Dc, Ecc = T_(decc.astype(np.float32)), T_(encc.astype(np.float32))
    args = (Dm[:, :d], Dc[:, :d], Ec[:, d:2 * d], Ecc[:, d:2 * d], Ec[:, 2 * d:], Ecc[:, 2 * d:])
    kid = T_(ids.reshape(-1))
    sd = torch.tensor([1], device=dev(), dtype=torch.int32)
    Om, Oc, LSE = ops.klattn_fwd(*args, kid, B, H, L, 0.0, sd, 16, 0, prec=pk)
    assert rel(Om.cpu().numpy(), om) < 1e-4 and rel(Oc.cpu().numpy(), oc) < 1e-4
    gm = torch.full((T, 3 * d), float("nan"), device=dev())
    gc = torch.full((T, 3 * d), float("nan"), device=dev())
    outs = (gm[:, :d], gc[:, :d], gm[:, d:2 * d], gc[:, d:2 * d], gm[:, 2 * d:], gc[:, 2 * d:])
    ops.klattn_bwd(*args, kid, Om, Oc, LSE, T_(dOm), T_(dOc), B, H, L, 0.0, sd, 16, 0, out=outs, prec=pk)
    for name, got, want in zip(("dQm", "dQc", "dKm", "dKc", "dVm", "dVc"), outs, grads):
        assert rel(got.cpu().numpy(), want) < 5e-4, name


@pytest.mark.parametrize("E,V", [(5, 40), (4, 40), (8, 300), (3, 2)])
def test_kl_bpr_and_full_sort_kernels(E, V):
    """kldist_bpr: loss slots, dSm / dSc and the accumulated item-table gradients (ELU+1 chain included) against torch autograd
    in float64; kldist_full against kl_predict_full's padded chunking, including E not dividing V and E > V."""
    from adt_amd import ops
    r = np.random.RandomState(E * 1000 + V)
    B, L, d, pvn_w = 5, 12, 64, 0.3
    T = B * L
    # magnitudes of trained embeddings: the KL differences stay where fp32 -log(sigmoid(.)) is finite (in the reference too)
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
    inv = torch.tensor([1.0 / float(n)], device=dev(), dtype=torch.float32)
    dEm, dEc = torch.zeros(V, d, device=dev()), torch.zeros(V, d, device=dev())
    loss3 = torch.zeros(192, device=dev())
    dSm, dSc = ops.kldist_bpr(T_(sm), T_(sc), T_(Em), T_(Ec), T_(pos.astype(np.int32)), T_(neg.astype(np.int32)), pvn_w, inv, dEm, dEc, loss3)
    l3 = loss3.view(3, 64).sum(1).cpu().numpy()
    assert abs(l3[0] - float(loss)) < 1e-4 * abs(float(loss)) and abs(l3[1] - float(pvn_loss)) < 1e-4 * max(abs(float(pvn_loss)), 1e-6)
    assert abs(l3[2] - auc) < 1e-6
    assert rel(dSm.cpu().numpy(), tsm.grad.numpy()) < 5e-4 and rel(dSc.cpu().numpy(), tsc.grad.numpy()) < 5e-4
    assert rel(dEm.cpu().numpy(), gEm.numpy()) < 5e-4 and rel(dEc.cpu().numpy(), gEc.numpy()) < 5e-4
    # full sort: E users (the eval batch) against all V items
    um, uc = sm[:E], sc[:E]
    got = ops.kldist_full(T_(um), T_(uc), T_(Em), T_(Ec), V).cpu().numpy()
    assert rel(got, kl_full_ref(um, uc, Em, Ec)) < 1e-4


# ---- model against the reference fixtures ------------------------------------------------------------------------------
class Args:
    pass


def load_case(tag):
    g = np.load(os.path.join(GOLD, "stosa_kl_%s.npz" % tag))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


def build(cfg, P, prec, dropout=0.0, attention_dropout=0.0):
    from adt_amd.stosa.models import DisenDistSAModel
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = "cuda:0", cfg.item_size, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.num_users
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = dropout, attention_dropout, cfg.pvn_weight, prec, "kl"
    m = DisenDistSAModel(a)
    m.load_numpy(P)
    return m


def pick(g, key, got):
    """(got entries, fixture entries, fixture norm or None): the whole tensor, or the compacted fixture's strided samples."""
    got = np.asarray(got, np.float64).reshape(-1)
    if key in g.files:
        return got, np.asarray(g[key], np.float64).reshape(-1), None
    return got[sample_idx(got.size, 1024)], np.asarray(g[key + "@sample"], np.float64), float(g[key + "@norm"])


def close(g, key, got, tol):
    a, b, norm = pick(g, key, got)
    scale = max(np.abs(b).max(), 1e-6 if norm is None else norm / np.sqrt(np.asarray(got).size))
    ok = np.abs(a - b).max() < tol * scale
    if norm is not None:
        ok = ok and abs(np.linalg.norm(np.asarray(got, np.float64)) - norm) < tol * max(norm, 1e-9)
    return ok


def grads_match(g, P, grad_of, prec):
    none = set(str(x) for x in g["grad_none"])
    assert none == set(k for k in P if so.is_unused(k))
    gmax = max(float(np.abs(pick(g, "grad." + k, P[k])[1]).max()) for k in P if k not in none)
    for k in P:
        got = grad_of(k)
        if k in none:
            assert np.all(got == 0.0), k
            continue
        a, b, norm = pick(g, "grad." + k, got)
        if prec == "f32":
            floor = max(np.abs(b).max(), 1e-3 * gmax)
            assert np.abs(a - b).max() < 5e-4 * floor, k
            if norm is not None:
                assert abs(np.linalg.norm(got.astype(np.float64)) - norm) < 5e-4 * max(norm, 1e-3 * gmax * np.sqrt(got.size)), k
        else:
            assert np.linalg.norm(a - b) < 0.1 * max(np.linalg.norm(b), 1e-3 * gmax * np.sqrt(b.size)), k


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_kl_finetune_and_predict_full_match_reference(tag, prec):
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    m.eval()
    mo, co, _, margins, enc_in, enc_rec, dec_out = m.finetune(g["input_ids"], g["dec_ids"], np.zeros(len(g["input_ids"]), np.int64))
    tol = 1e-4 if prec == "f32" else 3e-2
    assert close(g, "mean_out", mo.cpu().numpy(), tol) and close(g, "cov_out", co.cpu().numpy(), tol)
    for i in range(cfg.num_layers):
        assert close(g, "enc_in_mean_%d" % i, enc_in[i][0].cpu().numpy(), tol) and close(g, "enc_in_cov_%d" % i, enc_in[i][1].cpu().numpy(), tol)
        assert close(g, "rec_mean_%d" % i, enc_rec[i][0].cpu().numpy(), tol) and close(g, "rec_cov_%d" % i, enc_rec[i][1].cpu().numpy(), tol)
        assert close(g, "dec_out_mean_%d" % i, dec_out[i][0].cpu().numpy(), tol) and close(g, "dec_out_cov_%d" % i, dec_out[i][1].cpu().numpy(), tol)
    assert close(g, "full_dist", m.predict_full(g["input_ids"], g["dec_ids"]).cpu().numpy(), tol)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_kl_gradients_match_reference(tag, prec):
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    m.train()
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    st = m.stage(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
    B, L = g["input_ids"].shape
    norms = torch.tensor([0.0, B * L * cfg.hidden_units, B * L * cfg.num_heads], device="cuda:0")
    slots = torch.zeros(3 + 4 * cfg.num_layers, 64, device="cuda:0")
    m.flat_grad.zero_()
    m.loss_forward_backward(st, lam1, lam2, norms, slots)
    torch.cuda.synchronize()
    grads_match(g, P, lambda k: m.G(k).cpu().numpy(), prec)


@pytest.mark.parametrize("tag", TAGS)
def test_kl_train_step_matches_reference_fp32(tag):
    """Loss parts of the fused step and the weights after its Adam step: from zero moments, torch.optim.Adam moves each weight by
    lr * g / (|g| + eps), so the reference's weights follow from the recorded gradient."""
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P, "f32")
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    lr = float(g["lr"])
    tr = FusedStosaTrainer(m, lam1, lam2, lr=lr)
    tr.step(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
    torch.cuda.synchronize()
    parts = tr.loss_parts().cpu().numpy()
    assert abs(parts[0] - float(g["bpr"])) < 1e-4 * abs(float(g["bpr"]))
    assert abs(parts[1] - float(g["pvn"])) < 1e-4 * max(abs(float(g["pvn"])), 1e-5)
    assert abs(parts[2] - float(g["auc"])) < 1e-5
    assert abs(float(tr.loss()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    none = set(str(x) for x in g["grad_none"])
    for k in P:
        w1 = m.P(k).cpu().numpy().astype(np.float64)
        if k in none:
            assert np.array_equal(w1, P[k].astype(np.float64)), k
            continue
        got, gr, _ = pick(g, "grad." + k, w1)
        w0 = pick(g, "grad." + k, P[k])[0]
        want = w0 - lr * gr / (np.abs(gr) + 1e-8)
        diff = np.abs(got - want)
        big = np.abs(gr) > 1e-5
        assert (diff[big].max() if big.any() else 0.0) < 0.05 * lr, k
        assert diff.max() < 1.01 * lr, k


# ---- the numpy oracle with the KL distances swapped in (dropout on) ------------------------------------------------------
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
def kl_oracle():
    """oracle.stosa_oracle with its two distance functions replaced for the duration of the call (the module is not edited)."""
    saved = so.wasserstein_distance, so.wasserstein_distance_matmul
    so.wasserstein_distance, so.wasserstein_distance_matmul = tape_kl_distance, tape_kl_distance_matmul
    try:
        yield so
    finally:
        so.wasserstein_distance, so.wasserstein_distance_matmul = saved


def test_kl_oracle_reproduces_reference_fixture():
    """The test-side KL oracle itself against the reference (dropout 0): loss and a few gradients of stosa_kl_small."""
    g, cfg, P = load_case("small")
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    with kl_oracle():
        loss, parts, G = so.loss_and_grads(P, cfg, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, training=False)
    assert abs(loss - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    assert abs(parts["bpr"] - float(g["bpr"])) < 1e-4 * abs(float(g["bpr"]))
    grads_match(g, P, lambda k: G[k] if G[k] is not None else np.zeros_like(P[k]), "f32")


@pytest.mark.parametrize("tag", ["small", "l2h2"])
def test_kl_training_step_with_dropout_matches_oracle(tag):
    g, cfg, P = load_case(tag)
    cfg.dropout, cfg.attention_dropout = 0.3, 0.3
    m = build(cfg, P, "f32", 0.3, 0.3)
    m.train()
    m.set_seed(9001)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    st = m.stage(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
    B, L = g["input_ids"].shape
    norms = torch.tensor([0.0, B * L * cfg.hidden_units, B * L * cfg.num_heads], device="cuda:0")
    slots = torch.zeros(3 + 4 * cfg.num_layers, 64, device="cuda:0")
    m.flat_grad.zero_()
    m.loss_forward_backward(st, lam1, lam2, norms, slots)
    torch.cuda.synchronize()
    with kl_oracle():
        loss, parts, G = so.loss_and_grads(P, cfg, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, training=True, seed=9001)
    w = [1.0, 1.0, 0.0]
    for l in range(cfg.num_layers):
        w += [lam1[l]] * 2
    for l in range(cfg.num_layers):
        w += [lam2[l]] * 2
    got = float((slots.sum(1).cpu().numpy() * np.array(w)).sum())
    assert abs(got - loss) < 1e-4 * abs(loss)
    gmax = max(float(np.abs(v).max()) for v in G.values() if v is not None)
    for k in P:
        if G[k] is not None:
            assert np.abs(m.G(k).cpu().numpy() - G[k]).max() < 5e-4 * max(np.abs(G[k]).max(), 1e-3 * gmax), k


# ---- trainer -------------------------------------------------------------------------------------------------------------
def test_kl_dp_shard_and_graph_replay():
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g, cfg, P = load_case("small")
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    B, L = g["input_ids"].shape
    nt = int((g["pos_ids"] > 0).sum())
    grads = []
    for lo, hi in ((0, B), (0, B // 2), (B // 2, B)):
        m = build(cfg, P, "f32", 0.2, 0.2)
        m.train()
        m.set_seed(31337)
        st = m.stage(g["input_ids"][lo:hi], g["dec_ids"][lo:hi], g["pos_ids"][lo:hi], g["neg_ids"][lo:hi], n_target_global=nt)
        norms = torch.tensor([0.0, B * L * cfg.hidden_units, B * L * cfg.num_heads], device="cuda:0")
        slots = torch.zeros(3 + 4 * cfg.num_layers, 64, device="cuda:0")
        m.flat_grad.zero_()
        m.loss_forward_backward(st, lam1, lam2, norms, slots, b_offset=lo)
        grads.append(m.flat_grad.cpu().numpy().copy())
    assert rel(grads[1] + grads[2], grads[0]) < 1e-4
    outs = []
    for use_graph in (False, True):
        m = build(cfg, P, "bf16", 0.2, 0.2)
        tr = FusedStosaTrainer(m, lam1, lam2, use_graph=use_graph, seed=5)
        for _ in range(4):
            tr.step(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().copy()))
    assert abs(outs[0][0] - outs[1][0]) < 1e-4 * abs(outs[0][0])
    assert rel(outs[1][1], outs[0][1]) < 5e-3


def test_kl_full_sort_ranks_like_reference():
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g, cfg, P = load_case("small")
    m = build(cfg, P, "f32")
    tr = FusedStosaTrainer(m, [0.3], [0.2])
    B = len(g["input_ids"])
    seen = np.zeros((B, cfg.item_size), bool)
    for b in range(B):
        seen[b, g["input_ids"][b]] = True
    pred, _ = tr.full_sort([(g["input_ids"], seen, g["pos_ids"][:, -1:])], topk=10)
    dist = g["full_dist"].copy()
    dist[seen] = 1e24
    want = np.argsort(dist, axis=1, kind="stable")[:, :10]
    assert np.array_equal(np.sort(pred, 1), np.sort(want, 1)) or np.array_equal(pred, want)


def test_kl_reference_loop_body_under_autograd():
    """stosa/trainer.py:534-559 with distance_metric='kl' (bpr_optimization's kl_distance branch) on finetune under autograd."""
    import torch.nn.functional as F
    g, cfg, P = load_case("small")
    m = build(cfg, P, "f32")
    m.train()
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    t = [torch.from_numpy(g[k]).cuda() for k in ("input_ids", "dec_ids", "pos_ids", "neg_ids")]
    uid = torch.zeros(len(g["input_ids"]), dtype=torch.long).cuda()
    d, H, L = cfg.hidden_units, cfg.num_heads, cfg.maxlen

    def kld(m1, c1, m2, c2):     # modules.kl_distance (stosa/modules.py:45-50)
        return (torch.sum(c1 / c2, -1) + torch.sum((m2 - m1) / c2 * (m2 - m1), -1) - m1.shape[1]
                + torch.log(torch.prod(c2, -1) / torch.prod(c1, -1))) / 2
    mo, co, att, margins, enc_in, enc_rec, dec_out = m.finetune(t[0], t[1], uid)
    act = torch.nn.ELU()
    pos_mean, neg_mean = m.item_mean_embeddings(t[2]), m.item_mean_embeddings(t[3])
    pos_cov, neg_cov = act(m.item_cov_embeddings(t[2])) + 1, act(m.item_cov_embeddings(t[3])) + 1
    pos_mean, pos_cov, neg_mean, neg_cov = (x.view(-1, d) for x in (pos_mean, pos_cov, neg_mean, neg_cov))
    sm, sc = mo.view(-1, d), co.view(-1, d)
    pos_logits, neg_logits, pos_vs_neg = kld(sm, sc, pos_mean, pos_cov), kld(sm, sc, neg_mean, neg_cov), kld(pos_mean, pos_cov, neg_mean, neg_cov)
    istarget = (t[2] > 0).view(-1).float()
    loss = torch.sum(-torch.log(torch.sigmoid(neg_logits - pos_logits + 1e-24)) * istarget) / torch.sum(istarget)
    pvn_loss = cfg.pvn_weight * torch.sum(torch.clamp(pos_logits - pos_vs_neg, 0) * istarget) / torch.sum(istarget)
    dec_out.reverse()
    for l in range(cfg.num_layers):
        loss = loss + lam1[l] * F.mse_loss(enc_in[l][0], dec_out[l][0])
        loss = loss + lam1[l] * F.mse_loss(enc_in[l][1], dec_out[l][1])
    bs = enc_rec[0][0].shape[0]
    label = torch.tile(torch.arange(H), [bs * L, 1]).cuda()
    for l in range(cfg.num_layers):
        loss = loss + lam2[l] * F.nll_loss(enc_rec[l][0].view(bs * L, H, H), label)
        loss = loss + lam2[l] * F.nll_loss(enc_rec[l][1].view(bs * L, H, H), label)
    loss = loss + pvn_loss
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    grads = dict(m.named_parameters())
    grads_match(g, P, lambda k: (grads[k].grad.cpu().numpy() if grads[k].grad is not None else np.zeros_like(P[k])), "f32")


# ---- trained metric -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_kl_deterministic_training_matches_reference(precision):
    """10 epochs with distance_metric='kl', dropout 0, from the same initial weights as the reference run recorded in
    ref_ndcg_stosa_small_kl_det.json (tools/ref_train_wide.py stosa_det_kl; evaluation in the reference's 256-user batches, on which
    the KL scores depend): NDCG@10 / HIT@10 / MRR within +-0.01, the epoch-mean loss within 1 %.  Ten epochs, not twenty: the reference's
own loss turns NaN at epoch 14 of this run (it takes log(prod(cov)) over 64 covariances; this implementation sums the logs)."""
    import json
    from tools.gpu_wide_ndcg_run import run_stosa
    ref = json.load(open(os.path.join(GOLD, "ref_ndcg_stosa_small_kl_det.json")))
    assert ref["distance_metric"] == "kl" and np.isfinite(ref["loss"]).all()
    ours = run_stosa(seed=42, precision=precision, deterministic=True, metric="kl", epochs=ref["cfg"]["epochs"])
    assert len(ours["evals"]) == len(ref["evals"]) > 0
    for lo, lr in zip(ours["loss"], ref["loss"]):
        assert abs(lo - lr) <= 0.01 * abs(lr), (ours["loss"], ref["loss"])
    for eo, er in zip(ours["evals"], ref["evals"]):
        for mode in ("val", "test"):
            for k in ("ndcg10", "hit10", "mrr"):
                assert abs(eo[mode][k] - er[mode][k]) <= 0.01, (precision, eo["epoch"], mode, k, eo[mode], er[mode])
