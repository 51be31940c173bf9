"""The four one-layer-per-call entry points of the bf16 SASRec supernet (adt_seq_enc_layer_fwd / _bwd, adt_seq_dec_layer_fwd / _bwd) called directly
through the C ABI and compared with the float64 bf16-operand reference of tests/seq_layer_cases.py: every output and every parameter gradient on
its own, bound min(2 D_k, cap) with D_k measured from the reference (see that module's docstring), plus the exact contracts of the interface
(padding rows, y_scale / y_acc, gx_acc, gradients are added, nothing reads what it did not write, shards).

With ADT_SEQ_LAYER_PARITY_OUT=<file> the module writes the worst err / D_k per tensor class and case group there (profiles/seq_layer_parity.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import seq_layer_cases as sc  # noqa: E402
from oracle import sasrec_oracle as so  # noqa: E402

RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("ADT_SEQ_LAYER_PARITY_OUT")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "worst err / D_k per tensor class and case group: err = kernel against the bf16x64 float64 oracle, D_k = fp32-operand against "
                               "bf16-operand oracle (tests/seq_layer_cases.py); the tests allow min(2 D_k, cap)",
                       "ratios": {k: RATIOS[k] for k in sorted(RATIOS)}}, f, indent=1, sort_keys=True)
            f.write("\n")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


def host(t):
    return t.detach().cpu().numpy()


def compare(c, got, ref, keys=None):
    """Every tensor of `got` against the reference within its bound; prints the figure first, records err / D_k."""
    inp, want, Dk, bound = ref[:4]
    gmax = sc.grad_scale(want)
    bad = []
    for k in (keys or sorted(got)):
        assert np.isfinite(got[k]).all(), "%s: %s is not finite" % (sc.case_id(c), k)
        err = sc.dist(k, got[k], want[k], gmax)
        print("%s %-40s err %.3e  D_k %.3e  bound %.3e" % (sc.case_id(c), k, err, Dk[k], bound[k]))
        if Dk[k] > 0.0:
            slot = "%s/%s/%s" % (c.group, c.kind, sc.tensor_class(k))
            if err / Dk[k] >= RATIOS.get(slot, {"ratio": -1.0})["ratio"]:
                RATIOS[slot] = {"ratio": round(err / Dk[k], 4), "err": float("%.4g" % err), "D_k": float("%.4g" % Dk[k]), "case": sc.case_id(c), "tensor": k}
        if not err <= bound[k]:
            bad.append((k, err, bound[k]))
    assert not bad, "%s: %r" % (sc.case_id(c), bad)


def grads_of(lay, prefix="g."):
    return {prefix + k: host(lay.g(k)).copy() for k in sc.names(lay.c.kind)}


def check_saved_u(c, lay, u_ref):
    """The u rows the forward saved against the reference's u, within the activation bound (1e-2 of the tensor's max: bf16 storage is 2^-9 of
    it); -> the kernel's gates u > 0.  A gate that differs from the reference's therefore sits on a u within that bound of zero."""
    u = host(lay.saved_u()).reshape(u_ref.shape)
    assert np.isfinite(u).all()
    tol = sc.CAP_ACT * np.abs(u_ref).max()
    err = np.abs(u - u_ref).max()
    flips = int(((u > 0) != (u_ref > 0)).sum())
    print("%s saved u: max err %.3e (allowed %.3e), %d of %d gates differ from the reference's" % (sc.case_id(c), err, tol, flips, u.size))
    assert err <= tol
    return u > 0


def run_layer(c, inp, u_ref, b_offset=None):
    """Forward, backward (encoder: with drec, then without), the encoder's eval forward: -> ({key: array} in the reference's keys, the kernel's
    ReLU gates), and the exact checks every run can make (padding rows, untouched classifier gradients, ignored rec, the saved u)."""
    lay = sc.Layer(c, inp)
    ids = inp["ids"]
    pad = torch.from_numpy((ids == 0).reshape(-1)).to("cuda:0")
    gy = dev(inp["gy"].reshape(-1, sc.D))
    got = {}
    y, rec = lay.fwd(b_offset=b_offset)
    got["y"] = host(y)
    assert float(y[pad].abs().max()) == 0.0 if bool(pad.any()) else True, "rows of id 0 must be exactly zero"
    gate = check_saved_u(c, lay, u_ref)
    if c.kind == "dec":
        gx, gf = lay.bwd(gy, b_offset=b_offset)
        got["gx"] = host(gx)
        got["gfeats"] = host(gf)
        got.update(grads_of(lay))
        return got, gate
    drec = dev(inp["drec"].reshape(-1, c.H * c.H))
    cls = [lay.g(k) for k in sc.CLS]
    if c.H > 1:
        got["rec"] = host(rec)
        gx, _ = lay.bwd(gy, rec=rec, drec=drec, b_offset=b_offset)
        got["gx"] = host(gx)
        got.update(grads_of(lay))
        lay.grad.zero_()
    else:
        assert bool(torch.isnan(rec).all()), "H = 1: rec is ignored, the buffer is not written"
    # drec == NULL (H = 1: rec and drec given, and ignored): no head-classifier term, its gradients stay exactly as prefilled
    fill = [torch.randn_like(t) for t in cls]
    for t, f in zip(cls, fill):
        t.copy_(f)
    gx, _ = lay.bwd(gy, rec=rec, drec=drec if c.H == 1 else None, b_offset=b_offset)
    pre = "n." if c.H > 1 else ""
    got[pre + "gx"] = host(gx)
    for t, f in zip(cls, fill):
        assert torch.equal(t, f), "the head-classifier gradients must stay as prefilled without drec"
    got.update({k: v for k, v in grads_of(lay, pre + "g.").items() if "sparse" not in k})
    # the eval call of SuperSASRecModel._candidate_feature_rows: training 0, p 0, no rec, y_scale 0 (plain store)
    ye, _ = lay.fwd(y_scale=0.0, training=0, p=0.0, want_rec=False, b_offset=b_offset)
    got["y_eval"] = host(ye)
    return got, gate


def at_gates(c, ref, gate, rec, b_offset=None, rows=None):
    """The reference with its backward taken at the kernel's gates and at the rec the kernel's backward was given (seq_layer_cases.py: the ReLU
    gate; run_oracle); D_k and the bounds stay the reference's own."""
    want = sc.run_oracle(c, ref[0], "bf16x64", b_offset, rows, gate=gate, rec_given=rec)
    want.pop("_u")
    for k in ("y", "rec", "y_eval"):
        assert k not in want or np.array_equal(want[k], ref[1][k])
    return (ref[0], want) + tuple(ref[2:])


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_layer_matches_float64_reference(c):
    assert sc.Layer.supported(c), "the per-sequence kernels do not cover this case"
    ref = sc.reference(c)
    got, gate = run_layer(c, ref[0], ref[4])
    assert set(got) == set(ref[1])
    compare(c, got, at_gates(c, ref, gate, got.get("rec")))


def _shard_inputs(c, inp, lo, hi):
    part = dict(inp, ids=inp["ids"][lo:hi], x=inp["x"][lo:hi], gy=inp["gy"][lo:hi])
    if c.kind == "enc":
        part["drec"] = so.rec_reference_order(so.rec_token_order(inp["drec"])[lo:hi])
    else:
        part["feats"] = inp["feats"][lo:hi]
    return part


@pytest.mark.parametrize("c", sc.SHARD, ids=sc.case_id)
def test_shard_matches_slice_of_full_batch(c):
    """Sequences [2:5) of a B = 6 batch, called with b_offset = 2, against the reference's slice of the full batch: the dropout indices are global."""
    ref = sc.reference(c, 0, (2, 5))
    got, gate = run_layer(c._replace(B=3), _shard_inputs(c, ref[0], 2, 5), ref[4], b_offset=2)
    compare(c, got, at_gates(c, ref, gate, got.get("rec"), 0, (2, 5)), keys=[k for k in sorted(got) if ".g." not in k and not k.startswith("g.")])


def ulps(a, b):
    """2 ulp (fp32) of the larger of the two terms, elementwise."""
    return 2.0 * np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("c", sc.CONTRACT, ids=sc.case_id)
def test_scale_accumulate_and_prefill_contracts(c):
    """No kernel tolerance here.  y = (y_acc ? y : 0) + y_scale * layer(x) against the y_scale = 1 result of the same kernel: the product and the
    sum round once each, within 2 ulp of the larger term; y_scale = 0 is the plain store (include/adt_hip.h); rows of id 0 are left alone under
    y_acc.  gx_acc and gfeats add to what is there in the same sense.  Parameter gradients are added with float atomics, workgroup by workgroup in
    any order: against the zero-prefill run the difference is within 64 (more than the workgroups of this case) half-ulps of the tensor's
    summed scales max |prefill| + max |gradient|."""
    inp = sc.reference(c)[0]
    lay = sc.Layer(c, inp)
    ids = inp["ids"].reshape(-1)
    w = np.float32(0.37)
    y1, rec1 = lay.fwd()
    y0, _ = lay.fwd(y_scale=0.0)
    assert torch.equal(y0, y1), "y_scale = 0 is the plain store"
    pre = torch.randn_like(y1)
    y2, _ = lay.fwd(y=pre.clone(), y_scale=float(w), y_acc=1)
    a, b = host(pre).astype(np.float64), float(w) * host(y1).astype(np.float64)
    assert (np.abs(host(y2) - (a + b)) <= ulps(a, b)).all()
    assert np.array_equal(host(y2)[ids == 0], host(pre)[ids == 0]), "y_acc = 1: rows of id 0 stay unchanged"
    assert (host(y1)[ids == 0] == 0.0).all()

    gy = dev(inp["gy"].reshape(-1, sc.D))
    kw = dict(rec=rec1, drec=dev(inp["drec"].reshape(-1, c.H * c.H))) if c.kind == "enc" else {}
    gx0, gf0 = lay.bwd(gy, **kw)
    G0 = host(lay.grad).astype(np.float64)
    gxp, gfp, Rp = torch.randn_like(gx0), torch.randn_like(gx0), torch.randn_like(lay.grad)
    lay.grad.copy_(Rp)
    gx1, gf1 = lay.bwd(gy, gx=gxp.clone(), gx_acc=1, gfeats=gfp.clone() if c.kind == "dec" else None, **kw)
    a, b = host(gxp).astype(np.float64), host(gx0).astype(np.float64)
    assert np.isfinite(b).all() and (np.abs(host(gx1) - (a + b)) <= ulps(a, b)).all(), "gx_acc = 1 adds to the prefill"
    if c.kind == "dec":
        a, b = host(gfp).astype(np.float64), host(gf0).astype(np.float64)
        assert np.isfinite(b).all() and (np.abs(host(gf1) - (a + b)) <= ulps(a, b)).all(), "gfeats is added to"
    G1, R = host(lay.grad).astype(np.float64), host(Rp).astype(np.float64)
    for k, (o, shp) in lay.lay.items():
        n = int(np.prod(shp))
        g0, g1, r = G0[o:o + n], G1[o:o + n], R[o:o + n]
        assert np.abs(g0).max() > 0.0, k
        assert np.abs((g1 - r) - g0).max() <= 64 * 2.0 ** -24 * (np.abs(r).max() + np.abs(g0).max()), k
    used = np.zeros(lay.grad.numel(), bool)
    for o, shp in lay.lay.values():
        used[o:o + int(np.prod(shp))] = True
    assert np.array_equal(G1[~used], R[~used]), "the alignment gaps between the tensors are not written"


def test_unsupported_shapes_are_rejected():
    """H 3, H 0, L 10 (L % 4), L 228 (> 224) and H 4 at L 224 (head size 16 stops at 192) return non-zero from each of the four entries, with adt_last_error naming the entry; nothing is
    launched (the buffers are those of a valid H 2, L 12 case)."""
    c = sc.Case("enc", 2, 12, 3, 0.0, 0, "reject")
    le, ld = sc.Layer(c, sc.make_inputs(c)), sc.Layer(c._replace(kind="dec"), sc.make_inputs(c._replace(kind="dec")))
    from adt_amd import ops
    p, st = ops._p, ops._stream()
    buf = torch.zeros(64 * 1024, device="cuda:0")
    lib = le.lib
    assert lib.adt_seq_layer_supported(1, 224, 64, 16) == 0 and lib.adt_seq_layer_supported(1, 192, 64, 16) == 1
    for H, L in ((3, 12), (0, 12), (2, 10), (2, 228), (4, 224)):
        calls = {
            "seq_enc_layer_fwd": lambda: lib.adt_seq_enc_layer_fwd(3, L, H, p(le.ids), p(le.x), ctypes.byref(le.P), p(le.flat), p(le.wimg), 0.0, p(le.seed), 1, 2, 3, 0, 1,
                                                                   p(buf), p(buf), 1.0, 0, None, st),
            "seq_enc_layer_bwd": lambda: lib.adt_seq_enc_layer_bwd(3, L, H, p(le.ids), p(le.x), ctypes.byref(le.P), ctypes.byref(le.G), p(le.flat), p(le.wimg), 0.0,
                                                                   p(le.seed), 1, 2, 3, 0, p(buf), p(buf), 1.0, None, None, p(buf), 0, p(buf), st),
            "seq_dec_layer_fwd": lambda: lib.adt_seq_dec_layer_fwd(3, L, H, p(ld.ids), p(ld.x), p(ld.feats), ctypes.byref(ld.P), p(ld.flat), p(ld.wimg), 0.0, p(ld.seed),
                                                                   1, 2, 3, 4, 0, p(buf), p(buf), 1.0, 0, st),
            "seq_dec_layer_bwd": lambda: lib.adt_seq_dec_layer_bwd(3, L, H, p(ld.ids), p(ld.x), p(ld.feats), ctypes.byref(ld.P), ctypes.byref(ld.G), p(ld.flat), p(ld.wimg),
                                                                   0.0, p(ld.seed), 1, 2, 3, 4, 0, p(buf), p(buf), 1.0, p(buf), 0, p(buf), p(buf), st),
        }
        for name, call in calls.items():
            assert call() != 0, (name, H, L)
            assert name in lib.adt_last_error().decode(), (name, H, L, lib.adt_last_error())
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
