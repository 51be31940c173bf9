"""The streamed STOSA-ADT distance-attention kernels (adt_wattn_long.cuh through ops.wattn_long_* / klattn_long_*) against a float64 torch
restatement of DistAttention (stosa/modules.py:222-275) for both metrics and both precisions: past the whole-(b, h) kernels' length bound
(257 .. 1024 rows), below it on the same tensors as the existing exact kernels (same dropped elements), with strided operands and outputs,
and the refusals.

Inputs as in test_stosa_kl_hip.py::test_kl_attention_kernels: normal means, exp(0.5 N) covariances, seed, site, b_off = 2468, 16, 5.
Bounds, relative to the reference's largest magnitude: exact arithmetic 1e-4 outputs / 5e-4 gradients, bf16 operands 3e-2 / 6e-2 (the
project's own for these kernels).  Every figure is printed before it is asserted (pytest -s)."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import stosa_oracle as so, tape as tp  # noqa: E402

MASK = np.float32(-2.0 ** 32 + 1)
SEED, SITE, B_OFF = 2468, 16, 5
NAMES = ("dQm", "dQc", "dKm", "dKc", "dVm", "dVc")
TOL = {"f32": (1e-4, 5e-4), "bf16": (3e-2, 6e-2)}


def dev():
    return torch.device("cuda:0")


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


# ---- float64 restatement of the reference's arithmetic ------------------------------------------------------------------
def kl_matmul64(m1, c1, m2, c2):
    """kl_distance_matmul (stosa/modules.py:52-70) with log(prod) as sum(log): (..., n, hd) x (..., n, hd) -> (..., n, n)."""
    hd = m1.shape[-1]
    logdet = torch.log(c2).sum(-1).unsqueeze(-2) - torch.log(c1).sum(-1).unsqueeze(-1)
    mean = torch.matmul((m1 - m2) ** 2, (1.0 / c2).transpose(-1, -2))
    trace = torch.matmul(1.0 / c2, c1.transpose(-1, -2))
    return (logdet + mean + trace - hd) / 2


def w_matmul64(m1, c1, m2, c2):
    """wasserstein_distance_matmul (stosa/modules.py:30-43)."""
    mean = (m1 ** 2).sum(-1, keepdim=True) + (m2 ** 2).sum(-1).unsqueeze(-2) - 2 * torch.matmul(m1, m2.transpose(-1, -2))
    s1, s2 = torch.sqrt(torch.clamp(c1, min=1e-24)), torch.sqrt(torch.clamp(c2, min=1e-24))
    cov = (s1 ** 2).sum(-1, keepdim=True) + (s2 ** 2).sum(-1).unsqueeze(-2) - 2 * torch.matmul(s1, s2.transpose(-1, -2))
    return mean + cov


def attn_ref(metric, t6, ids, B, H, L, p, seed, site, b_off, dOm, dOc):
    """klattn_ref of test_stosa_kl_hip.py and its Wasserstein twin: DistAttention's score / softmax / dropout / contexts in float64; the
    additive mask rounds in fp32 as in the reference (scores + (-2^32 + 1) of a fully masked row collapse to one value), with gradient 1
    through it."""
    d = t6[0].shape[1]
    hd = d // H
    vs = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in t6]
    qm, qc, km, kc, vm, vc = [v.view(B, L, H, hd).permute(0, 2, 1, 3) for v in vs]
    s = -(kl_matmul64 if metric == "kl" else w_matmul64)(qm, qc, km, kc) / math.sqrt(hd)
    masked = torch.from_numpy(np.broadcast_to(so._mask(ids) != 0, (B, H, L, L)).copy())
    rounded = (s.detach().float() + torch.tensor(MASK)).double()
    s = torch.where(masked, s + (rounded - s).detach(), s)
    keep = torch.from_numpy(tp.dropout(tp.const(np.ones((B, H, L, L), np.float32)), p, seed, site, tp.idx_attn(B, H, L, b_off)).v).double()
    pr = torch.softmax(s, -1) * keep
    om = torch.matmul(pr, vm).permute(0, 2, 1, 3).reshape(B * L, d)
    oc = torch.matmul(pr * pr, vc).permute(0, 2, 1, 3).reshape(B * L, d)
    ((om * torch.from_numpy(dOm).double()).sum() + (oc * torch.from_numpy(dOc).double()).sum()).backward()
    return om.detach().numpy(), oc.detach().numpy(), [v.grad.numpy() for v in vs]


# ---- cases: (B, H, L, hd, p, padding) ---------------------------------------------------------------------------------------
def pad_default(ids, L):
    ids[0, : L // 3] = 0          # left padding: dead query rows (uniform attention over all keys, gradient kept), masked key columns
    if len(ids) > 1:
        ids[1, L // 2] = 0        # one padded key inside a sequence


def pad_b(ids, L):
    ids[0, :90] = 0               # dead rows over several query tiles and key chunks
    ids[1, L // 2] = 0


def pad_c(ids, L):
    ids[0, :] = 0                 # a sequence of padding only: every row dead
    ids[1, L // 2] = 0


def pad_d(ids, L):
    ids[0, :100] = 0


CASES = {
    "a_l257": (2, 2, 257, 16, 0.0, pad_default),       # the first length the whole-(b, h) kernels refuse; ragged last tile, partly filled last group
    "b_l272": (2, 1, 272, 64, 0.3, pad_b),
    "c_l300": (2, 2, 300, 32, 0.0, pad_c),
    "d_l1024_hd64": (1, 1, 1024, 64, 0.2, pad_d),
    "d_l1024_hd16": (1, 4, 1024, 16, 0.2, pad_d),
    "e_l100_hd64": (2, 1, 100, 64, 0.3, pad_default),
    "e_l37_hd32": (2, 2, 37, 32, 0.3, pad_default),
    "e_l9_hd64": (2, 1, 9, 64, 0.3, pad_default),
    "e_l128_hd16": (1, 4, 128, 16, 0.3, pad_default),
}
LONG = [k for k in CASES if not k.startswith("e_")]
SHORT = [k for k in CASES if k.startswith("e_")]


@functools.lru_cache(maxsize=None)
def case(tag, metric):
    """Inputs and the float64 reference of one case, computed once and shared by the precisions (read-only)."""
    B, H, L, hd, p, pad = CASES[tag]
    r = np.random.RandomState(B * 100 + L + hd)
    d, T = H * hd, B * L
    qm, km, vm = (r.standard_normal((T, d)).astype(np.float32) for _ in range(3))
    qc, kc, vc = (np.exp(0.5 * r.standard_normal((T, d))).astype(np.float32) for _ in range(3))
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    pad(ids, L)
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    t6 = (qm, qc, km, kc, vm, vc)
    om, oc, grads = attn_ref(metric, t6, ids, B, H, L, p, SEED, SITE, B_OFF, dOm, dOc)
    return dict(B=B, H=H, L=L, hd=hd, p=p, t6=t6, ids=ids, dOm=dOm, dOc=dOc, om=om, oc=oc, grads=grads)


def fns(metric, long):
    from adt_amd import ops
    if long:
        return (ops.klattn_long_fwd, ops.klattn_long_bwd) if metric == "kl" else (ops.wattn_long_fwd, ops.wattn_long_bwd)
    return (ops.klattn_fwd, ops.klattn_bwd) if metric == "kl" else (ops.wattn_fwd, ops.wattn_bwd)


def prec_of(prec):
    from adt_amd import ops
    return {"f32": ops.PREC_F32, "bf16": ops.PREC_BF16}[prec]


def run(c, metric, long, pk):
    fwd, bwd = fns(metric, long)
    B, H, L, p = c["B"], c["H"], c["L"], c["p"]
    sd = torch.tensor([SEED], device=dev(), dtype=torch.int32)
    g = [T_(x) for x in c["t6"]]
    kid = T_(c["ids"].reshape(-1))
    Om, Oc, LSE = fwd(*g, kid, B, H, L, p, sd, SITE, B_OFF, prec=pk)
    outs = bwd(*g, kid, Om, Oc, LSE, T_(c["dOm"]), T_(c["dOc"]), B, H, L, p, sd, SITE, B_OFF, prec=pk)
    torch.cuda.synchronize()
    return Om.cpu().numpy(), Oc.cpu().numpy(), LSE.cpu().numpy(), [o.cpu().numpy() for o in outs]


def check(tag, what, c, Om, Oc, outs, tol_f, tol_g):
    figs = [("Om", rel(Om, c["om"]), tol_f), ("Oc", rel(Oc, c["oc"]), tol_f)]
    figs += [(n, rel(got, want), tol_g) for n, got, want in zip(NAMES, outs, c["grads"])]
    print("%s %s: %s" % (tag, what, "  ".join("%s %.3g" % (n, e) for n, e, _ in figs)))
    for n, e, tol in figs:
        assert e < tol, (tag, what, n, e, tol)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", LONG)
def test_long_kernels_against_float64(tag, metric, prec):
    """(a) L 257; (b) L 272, hd 64, dropout, a dead prefix of 90 rows and a padded key inside; (c) L 300 with a sequence of padding only;
    (d) L 1024 at hd 64 and hd 16 with dropout and a dead prefix of 100 rows."""
    c = case(tag, metric)
    Om, Oc, LSE, outs = run(c, metric, True, prec_of(prec))
    assert np.isfinite(LSE).all()
    check(tag, "%s %s" % (metric, prec), c, Om, Oc, outs, *TOL[prec])


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", SHORT)
def test_below_the_old_bound_both_families_on_the_same_tensors(tag, metric):
    """(e) The long entry points take every 1 <= L <= 1024: against float64, and against the existing exact kernels (prec=None) on the same
    tensors with p = 0.3 -- one dropped element that differed would move an output by far more than the exact bound."""
    c = case(tag, metric)
    Om0, Oc0, LSE0, outs0 = run(c, metric, False, None)
    check(tag, "%s existing exact" % metric, c, Om0, Oc0, outs0, *TOL["f32"])
    for prec in ("f32", "bf16"):
        Om, Oc, LSE, outs = run(c, metric, True, prec_of(prec))
        check(tag, "%s long %s" % (metric, prec), c, Om, Oc, outs, *TOL[prec])
        if prec == "f32":
            figs = [rel(Om, Om0), rel(Oc, Oc0)] + [rel(a, b) for a, b in zip(outs, outs0)]
            print("%s %s long f32 vs existing exact: %s  LSE %.3g" % (tag, metric, "  ".join("%.3g" % e for e in figs), np.abs(LSE - LSE0).max()))
            assert max(figs[:2]) < 1e-4 and max(figs[2:]) < 5e-4
            assert np.abs(LSE - LSE0).max() < 1e-4 * max(np.abs(LSE0).max(), 1.0)
            # the same elements dropped: exactly the same context entries are exact zeros (a query all of whose kept keys are dropped)
            assert np.array_equal(Om == 0.0, Om0 == 0.0)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
def test_strided_cross_attention_at_l272(metric, prec):
    """(f) Decoder-style call: queries from a (T, 3d) tensor, keys / values from columns of a (T, 2d) tensor, gradients into strided views of
    two (T, 3d) buffers (the model's layout; under KL dKc / dQc are accumulated across the two passes in place)."""
    B, H, L, hd = 2, 2, 272, 32
    d, T = H * hd, B * L
    r = np.random.RandomState(5)
    dec = r.standard_normal((T, 3 * d)).astype(np.float32)
    enc = r.standard_normal((T, 2 * d)).astype(np.float32)
    decc, encc = np.exp(0.4 * dec).astype(np.float32), np.exp(0.4 * enc).astype(np.float32)
    ids = r.randint(1, 9, size=(B, L)).astype(np.int32)
    ids[1, :70] = 0
    ids[0, 130] = 0
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    t6 = (dec[:, :d], decc[:, :d], enc[:, :d], encc[:, :d], enc[:, d:], encc[:, d:])
    om, oc, grads = attn_ref(metric, t6, ids, B, H, L, 0.0, 1, 16, 0, dOm, dOc)
    fwd, bwd = fns(metric, True)
    Dm, Dc, Em, Ec = T_(dec), T_(decc), T_(enc), T_(encc)
    args = (Dm[:, :d], Dc[:, :d], Em[:, :d], Ec[:, :d], Em[:, d:], Ec[:, d:])
    kid = T_(ids.reshape(-1))
    sd = torch.tensor([1], device=dev(), dtype=torch.int32)
    pk = prec_of(prec)
    Om, Oc, LSE = fwd(*args, kid, B, H, L, 0.0, sd, 16, 0, prec=pk)
    gm = torch.full((T, 3 * d), float("nan"), device=dev())
    gc = torch.full((T, 3 * d), float("nan"), device=dev())
    outs = (gm[:, :d], gc[:, :d], gm[:, d:2 * d], gc[:, d:2 * d], gm[:, 2 * d:], gc[:, 2 * d:])
    bwd(*args, kid, Om, Oc, LSE, T_(dOm), T_(dOc), B, H, L, 0.0, sd, 16, 0, out=outs, prec=pk)
    torch.cuda.synchronize()
    c = dict(om=om, oc=oc, grads=grads)
    check("f_l272", "%s %s strided" % (metric, prec), c, Om.cpu().numpy(), Oc.cpu().numpy(), [o.cpu().numpy() for o in outs], *TOL[prec])


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("B,H,L,hd,p,b_off,why", [(1, 1, 1025, 64, 0.0, 0, "outside 1..1024"), (1, 1, 64, 128, 0.0, 0, "head_dim=128"),
                                                  (1, 1, 1024, 64, 0.2, 4096, "dropout index space")])
def test_refusals_return_an_error_and_launch_nothing(metric, B, H, L, hd, p, b_off, why):
    """(g) L 1025, head size 128, and p > 0 with an index space (b_offset + B) H L L of 2^32 or more: the C ABI returns non-zero, names
    the reason, and the output buffers keep their sentinel."""
    from adt_amd import _lib, ops
    lib = _lib.load()
    d, T = H * hd, B * L
    x = torch.ones(T, d, device=dev())
    kid = torch.ones(T, device=dev(), dtype=torch.int32)
    sd = torch.tensor([SEED], device=dev(), dtype=torch.int32)
    Om, Oc, LSE = torch.full((T, d), -7.0, device=dev()), torch.full((T, d), -7.0, device=dev()), torch.full((B * H * L,), -7.0, device=dev())
    outs = [torch.full((T, d), -7.0, device=dev()) for _ in range(6)]
    P, st = ops._p, ops._stream()
    six = [P(x), d] * 6
    name = "klattn_long" if metric == "kl" else "wattn_long"
    for prec in (ops.PREC_F32, ops.PREC_BF16):
        rc = getattr(lib, "adt_%s_fwd" % name)(prec, *six, P(kid), B, H, L, hd, p, P(sd), SITE, b_off, P(Om), d, P(Oc), d, P(LSE), st)
        assert rc != 0 and why in lib.adt_last_error().decode(), lib.adt_last_error()
        rc = getattr(lib, "adt_%s_bwd" % name)(prec, *six, P(kid), P(x), d, P(x), d, P(x.view(-1)), P(x), d, P(x), d, B, H, L, hd, p, P(sd), SITE, b_off,
                                                *[P(o) for o in outs], d, st)
        assert rc != 0 and why in lib.adt_last_error().decode(), lib.adt_last_error()
    torch.cuda.synchronize()
    for t in [Om, Oc, LSE] + outs:
        assert bool((t == -7.0).all())
    with pytest.raises(_lib.AdtError):
        fns(metric, True)[0](x, x, x, x, x, x, kid, B, H, L, p, sd, SITE, b_off, prec=ops.PREC_F32)
