"""GPU: the distance attention at head size 128 (adt_wattn_hd128.hip through ops.wattn_hd128_* / klattn_hd128_*)
against the float64 reference of tests/test_wattn_long_hip.py (attn_ref), both metrics, both precisions: ragged and multi-tile lengths,
a head offset, dead rows over several tiles and chunks, a sequence of padding only, L 1024; heads padded from 100 to 128 lanes against the
true 100-wide head; the model's strided operands; the refusals.

Bounds, relative to the reference's largest magnitude (the project's own for these kernels): exact arithmetic 1e-4 outputs / 5e-4
gradients, bf16 operands 3e-2 / 6e-2.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_wattn_long_hip import (B_OFF, NAMES, SEED, SITE, T_, TOL, attn_ref, check, dev, pad_c, pad_d, pad_default, prec_of,  # noqa: E402
                                       rel)

HD = 128


def pad_dead40(ids, L):
    ids[0, :40] = 0               # dead rows over three query tiles and two key chunks
    ids[1, L // 2] = 0            # one padded key inside a sequence


# (B, H, L, hd, p, padding)
CASES = {
    "l9": (2, 1, 9, HD, 0.3, pad_default),            # one ragged tile
    "l37_h2": (2, 2, 37, HD, 0.0, pad_default),       # head offset at d 256, three tiles in a group of four
    "l100": (2, 1, 100, HD, 0.3, pad_dead40),         # several forward and backward chunks, dead rows over several tiles
    "l150": (2, 1, 150, HD, 0.0, pad_c),              # a sequence of padding only, three workgroups per (b, h)
    "l1024": (1, 1, 1024, HD, 0.2, pad_d),            # the last LSE / delta / validity slots
}


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


def fns(metric):
    from adt_amd import ops
    return (ops.klattn_hd128_fwd, ops.klattn_hd128_bwd) if metric == "kl" else (ops.wattn_hd128_fwd, ops.wattn_hd128_bwd)


def seed_tensor(seed=SEED):
    return torch.tensor([seed], device=dev(), dtype=torch.int32)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", list(CASES))
def test_kernels_against_float64(tag, metric, prec):
    """scale = 1 / sqrt(128), hd_live = 128 (under KL: the unpadded kernel).  bf16 gradients at head size 64 measured 3.2e-2 of the 6e-2
    bound at L 1024; the figures of this head size are in section 29."""
    c = case(tag, metric)
    fwd, bwd = fns(metric)
    B, H, L, p = c["B"], c["H"], c["L"], c["p"]
    pk, sd, scale = prec_of(prec), seed_tensor(), 1.0 / np.sqrt(HD)
    g = [T_(x) for x in c["t6"]]
    kid = T_(c["ids"].reshape(-1))
    Om, Oc, LSE = fwd(*g, kid, B, H, L, scale, HD, p, sd, SITE, B_OFF, prec=pk)
    outs = bwd(*g, kid, Om, Oc, LSE, T_(c["dOm"]), T_(c["dOc"]), B, H, L, scale, HD, p, sd, SITE, B_OFF, prec=pk)
    torch.cuda.synchronize()
    assert np.isfinite(LSE.cpu().numpy()).all()
    check(tag, "%s %s" % (metric, prec), c, Om.cpu().numpy(), Oc.cpu().numpy(), [o.cpu().numpy() for o in outs], *TOL[prec])


# ---- heads padded from 100 to 128 lanes -------------------------------------------------------------------------------------------------
def bits_zero(a):
    return bool((np.ascontiguousarray(a, np.float32).view(np.uint32) == 0).all())


def widen(x, live, dp):
    out = np.zeros((x.shape[0], dp), np.float32)
    out[:, live] = x
    return out


@functools.lru_cache(maxsize=None)
def padded_case(metric, L, p):
    B, H, hd = 2, 1, 100
    d, T = H * hd, B * L
    r = np.random.RandomState(L * 100 + hd)
    qm, km, vm = (r.standard_normal((T, d)).astype(np.float32) for _ in range(3))
    qc, kc, vc = (np.exp(0.5 * r.standard_normal((T, d))).astype(np.float32) for _ in range(3))
    ids = r.randint(1, 50, size=(B, L)).astype(np.int32)
    pad_default(ids, L)
    dOm, dOc = r.standard_normal((T, d)).astype(np.float32), r.standard_normal((T, d)).astype(np.float32)
    t6 = (qm, qc, km, kc, vm, vc)
    om, oc, grads = attn_ref(metric, t6, ids, B, H, L, p, SEED, SITE, B_OFF, dOm, dOc)
    return dict(B=B, H=H, L=L, hd=hd, p=p, t6=t6, ids=ids, dOm=dOm, dOc=dOc, om=om, oc=oc, grads=grads)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("L", [12, 150])
@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
def test_padded_lanes_against_the_true_head_size(metric, L, p, prec):
    """hd_live 100 of 128, scale = 1 / sqrt(100): operands widened with zero pad lanes (means, covariances and dO alike: what the model
    holds there), the reference on the compact 100-wide rows.  Gradient buffers start as NaN; every pad lane of the contexts and of all six
    gradients comes back as +0.0, bit for bit; nothing is NaN or inf."""
    c = padded_case(metric, L, p)
    fwd, bwd = fns(metric)
    B, H, hd = c["B"], c["H"], c["hd"]
    dp, T = H * HD, B * L
    live = (np.arange(dp) % HD) < hd
    pk, sd, scale = prec_of(prec), seed_tensor(), 1.0 / np.sqrt(hd)
    g = [T_(widen(x, live, dp)) for x in c["t6"]]
    kid = T_(c["ids"].reshape(-1))
    Om, Oc, LSE = fwd(*g, kid, B, H, L, scale, hd, p, sd, SITE, B_OFF, prec=pk)
    outs = [torch.full((T, dp), float("nan"), device=dev()) for _ in range(6)]
    bwd(*g, kid, Om, Oc, LSE, T_(widen(c["dOm"], live, dp)), T_(widen(c["dOc"], live, dp)), B, H, L, scale, hd, p, sd, SITE, B_OFF, out=outs, prec=pk)
    torch.cuda.synchronize()
    hOm, hOc, houts = Om.cpu().numpy(), Oc.cpu().numpy(), [o.cpu().numpy() for o in outs]
    assert np.isfinite(LSE.cpu().numpy()).all() and all(np.isfinite(x).all() for x in [hOm, hOc] + houts)
    check("w100 L%d p%g" % (L, p), "%s %s" % (metric, prec), c, hOm[:, live], hOc[:, live], [x[:, live] for x in houts], *TOL[prec])
    for name, x in zip(("Om", "Oc") + NAMES, [hOm, hOc] + houts):
        assert bits_zero(x[:, ~live]), name


# ---- the model's packed rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("layout", ["self", "cross"])
def test_strided_operands_equal_the_contiguous_call(layout, metric, prec):
    """L 40, B 2, one head.  self: Q / K / V are column blocks of one (T, 3d) tensor per kind, as the model's fused projection leaves them.
    cross: Q from a (T, d) tensor, K / V from a (T, 2d) one.  Gradients into column blocks of two (T, 3d) buffers.  Every result equals the
    contiguous call's bit for bit."""
    B, H, L, d, p = 2, 1, 40, HD, 0.3
    T = B * L
    r = np.random.RandomState(11)
    fwd, bwd = fns(metric)
    pk, sd, scale = prec_of(prec), seed_tensor(), 1.0 / np.sqrt(HD)
    Pm = T_(r.standard_normal((T, 3 * d)).astype(np.float32))
    Pc = T_(np.exp(0.4 * r.standard_normal((T, 3 * d))).astype(np.float32))
    ids = r.randint(1, 9, size=(B, L)).astype(np.int32)
    ids[1, :17] = 0
    ids[0, 20] = 0
    kid = T_(ids.reshape(-1))
    dOm, dOc = T_(r.standard_normal((T, d)).astype(np.float32)), T_(r.standard_normal((T, d)).astype(np.float32))
    if layout == "self":
        views = (Pm[:, :d], Pc[:, :d], Pm[:, d:2 * d], Pc[:, d:2 * d], Pm[:, 2 * d:], Pc[:, 2 * d:])
    else:
        qm, qc = Pm[:, :d].contiguous(), Pc[:, :d].contiguous()
        kvm, kvc = Pm[:, d:].contiguous(), Pc[:, d:].contiguous()
        views = (qm, qc, kvm[:, :d], kvc[:, :d], kvm[:, d:], kvc[:, d:])
        assert qm.stride(0) == d and kvm.stride(0) == 2 * d
    flat = tuple(v.contiguous() for v in views)
    a = fwd(*flat, kid, B, H, L, scale, HD, p, sd, SITE, B_OFF, prec=pk)
    b = fwd(*views, kid, B, H, L, scale, HD, p, sd, SITE, B_OFF, prec=pk)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ga = bwd(*flat, kid, *a, dOm, dOc, B, H, L, scale, HD, p, sd, SITE, B_OFF, prec=pk)
    gm = torch.full((T, 3 * d), float("nan"), device=dev())
    gc = torch.full((T, 3 * d), float("nan"), device=dev())
    outs = (gm[:, :d], gc[:, :d], gm[:, d:2 * d], gc[:, d:2 * d], gm[:, 2 * d:], gc[:, 2 * d:])
    bwd(*views, kid, *b, dOm, dOc, B, H, L, scale, HD, p, sd, SITE, B_OFF, out=outs, prec=pk)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, ga, outs):
        assert torch.equal(x, y), name
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gc).all())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
GOOD = dict(B=1, H=1, L=16, hd=HD, ld=HD, scale=1.0 / np.sqrt(HD), hd_live=HD, p=0.0, b_off=0, kid=True)
REFUSALS = [(dict(hd=64, ld=64), "head_dim=64"), (dict(hd=256, ld=256), "head_dim=256"), (dict(L=1025), "outside 1..1024"),
            (dict(hd_live=0), "hd_live=0"), (dict(hd_live=129), "hd_live=129"), (dict(scale=0.0), "scale 0"), (dict(ld=130), "ld % 4"),
            (dict(kid=False), "key_ids is null"), (dict(L=1024, p=0.2, b_off=4095), "dropout index space")]


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("change,why", REFUSALS, ids=[w.replace(" ", "_") for _, w in REFUSALS])
def test_refusals_return_an_error_and_launch_nothing(metric, change, why):
    """Each refusal returns non-zero from both directions in both precisions, names the entry point and the reason, and leaves the output
    buffers at their sentinel; a good call afterwards still succeeds."""
    from adt_amd import _lib, ops
    lib = _lib.load()
    c = dict(GOOD, **change)
    B, H, L, hd, ld = c["B"], c["H"], c["L"], c["hd"], c["ld"]
    T = B * L
    x = torch.ones(T, max(ld, H * hd), device=dev())
    kid = torch.ones(T, device=dev(), dtype=torch.int32)
    sd = seed_tensor()
    sent = lambda *shape: torch.full(shape, -7.0, device=dev())
    Om, Oc, LSE = sent(T, x.shape[1]), sent(T, x.shape[1]), sent(B * H * L)
    outs = [sent(T, x.shape[1]) for _ in range(6)]
    P, st = ops._p, ops._stream()
    six = [P(x), ld] * 6
    name = "klattn_hd128" if metric == "kl" else "wattn_hd128"
    pk_id = P(kid) if c["kid"] else None
    for prec in (ops.PREC_F32, ops.PREC_BF16):
        rc = getattr(lib, "adt_%s_fwd" % name)(prec, *six, pk_id, B, H, L, hd, c["scale"], c["hd_live"], c["p"], P(sd), SITE, c["b_off"], P(Om), ld, P(Oc), ld,
                                               P(LSE), st)
        msg = lib.adt_last_error().decode()
        assert rc != 0 and why in msg and msg.startswith(name + "_fwd"), msg
        rc = getattr(lib, "adt_%s_bwd" % name)(prec, *six, pk_id, P(x), ld, P(x), ld, P(x.view(-1)), P(x), ld, P(x), ld, B, H, L, hd, c["scale"], c["hd_live"],
                                               c["p"], P(sd), SITE, c["b_off"], *[P(o) for o in outs], ld, st)
        msg = lib.adt_last_error().decode()
        assert rc != 0 and why in msg and msg.startswith(name + "_bwd"), msg
    torch.cuda.synchronize()
    for t in [Om, Oc, LSE] + outs:
        assert bool((t == -7.0).all())
    # a good call still succeeds, through the same raw entry points
    g = GOOD
    T = g["B"] * g["L"]
    y = torch.ones(T, HD, device=dev())
    kid = torch.ones(T, device=dev(), dtype=torch.int32)
    Om, Oc, LSE = fns(metric)[0](y, y, y, y, y, y, kid, g["B"], g["H"], g["L"], g["scale"], HD, 0.0, sd, SITE, 0, prec=ops.PREC_F32)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Om).all()) and bool(torch.isfinite(LSE).all())
    assert rel(Om.cpu().numpy(), np.ones((T, HD))) < 1e-6          # identical value rows: every context is that row
    with pytest.raises(_lib.AdtError):
        fns(metric)[0](y[:, :64], y[:, :64], y[:, :64], y[:, :64], y[:, :64], y[:, :64], kid, 1, 1, 16, 0.125, 64, 0.0, sd, SITE, 0, prec=ops.PREC_F32)
