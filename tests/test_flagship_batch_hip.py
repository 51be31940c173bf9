"""The step bench.py times, checked at the batch sizes it runs: SASRec-ADT ml-1m shape (L 200, d 64, H 2, 2 blocks), bf16 operands, dropout 0.5,
the bench's own init and its synthetic Zipf batches (bench.CFG, bench.synth_batches), against the oracle run with the SAME operand rounding
(`so.operands("bf16")`, as test_hip_model.test_lean_step_vs_bf16_operand_oracle_cfga_shape does at B 8).

The batch size selects the code: seq_split (adt_sasrec.hip) maps 8 / 4 / 2 / 1 workgroups to a sequence at B <= 32 / 64 / 128 / above, and
sizes the partial-sum areas the gradient fold reads; the item-table scatter runs under Zipf contention; k_step_begin's second copy loop starts
above 8 x 32 x 256 16-byte words of ids (B >= 328 at L 200).  The pinned id ring is driven with the producer ahead of the GPU, so the staged
prefetch of the next batch (ring_prefetch_body) is taken, and counted; one arm starts its 32-bit ring counters just below the wrap."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bench import CFG, synth_batches
from oracle import sasrec_oracle as so

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, D, H, NL, V = CFG["maxlen"], CFG["hidden_units"], CFG["num_heads"], CFG["num_layers"], CFG["item_num"]
OCFG = so.Cfg(V, L, D, H, NL, dropout=CFG["dropout"])
LAM1, LAM2, WD = CFG["lambdas1"], CFG["lambdas2"], CFG["weight_decay"]
B1, B2, EPS = 0.9, 0.98, 1e-8      # FusedTrainer's Adam defaults

# Bounds against the bf16-operand oracle, about twice the worst value measured on an MI355X over every case below (the per-case values are
# in the docstrings) and never looser than the B 8 test's: relative Frobenius error of one parameter gradient 0.05 (worst measured 0.029), of
# the whole gradient 0.025 (0.012), max-norm error of the forward outputs relative to the tensor's largest entry 1e-2 (8.3e-3), relative
# error of the loss 6e-6 (2.7e-6) and of the gradient norm 6e-4 (3.0e-4).
TOL_TENSOR, TOL_WHOLE, TOL_OUT, TOL_LOSS, TOL_GN = 0.05, 0.025, 1e-2, 6e-6, 6e-4


def _model():
    import bench
    m = bench.build_model("cuda:0", "bf16")
    assert m.lib.adt_seq_layer_supported(1, L, D, D // H) == 1, "the per-sequence fused kernels do not cover the flagship shape"
    return m


def _trainer(m, **kw):
    from adt_amd.sasrec.trainer import FusedTrainer
    args = dict(lr=CFG["lr"], weight_decay=WD, clip=CFG["clip"], seed=23)
    args.update(kw)
    return FusedTrainer(m, LAM1, LAM2, **args)


def _params(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _flat_params(m, flat):
    out = {}
    for k, _ in so.param_shapes(OCFG):
        off, n, shape = m._views[k]
        out[k] = flat[off:off + n].view(shape).cpu().numpy().copy()
    return out


def _seed(m):
    return int(m._seed.cpu().numpy().view(np.uint32)[0])


def _global_norms(b):
    GB = b[0].shape[0]
    return (float(np.count_nonzero(b[2])), float(GB * L * D), float(GB * L * H))


def _oracle(P, batch, seed, norms=None, b_offset=0):
    with so.operands("bf16"):
        out = so.forward(P, OCFG, *batch, training=True, seed=seed, b_offset=b_offset)
        loss, _, seeds = so.loss_and_seeds(P, OCFG, out, batch[2], LAM1, LAM2, WD, norms)
        G = so.backward(P, OCFG, out[5], seeds, WD)
    return out, loss, G


def _relmax(got, want):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-6)


def _check_step(m, tr, B, out, loss, G, tag, tol_tensor=TOL_TENSOR, tol_whole=TOL_WHOLE):
    """One step's outputs and gradients against the oracle's.  Every error is measured (and printed) before any is asserted, so one run
    reports the whole picture."""
    from adt_amd.sasrec import model as mm
    T = B * L
    errs = {"pos_logits": _relmax(m.ws_view(B, mm.WS_POS_LOGITS, 0, T).view(B, L), out[0]),
            "neg_logits": _relmax(m.ws_view(B, mm.WS_NEG_LOGITS, 0, T).view(B, L), out[1])}
    for i in range(NL):
        errs["enc_in.%d" % i] = _relmax(m.ws_view(B, mm.WS_ENC_X, i, T * D).view(B, L, D), out[2][i])
        errs["dec_out.%d" % i] = _relmax(m.ws_view(B, mm.WS_DEC_X, NL - i, T * D).view(B, L, D), out[3][i])
        errs["rec_ind.%d" % i] = _relmax(m.ws_view(B, mm.WS_REC, i, T * H * H).view(B, L, H, H), so.rec_reference_order(out[4][i]))
    gl, gn, tn = float(tr.loss()), float(tr.grad_norm()), so.grad_norm(G)
    errs["loss"] = abs(gl - loss) / abs(loss)
    errs["grad_norm"] = abs(gn - tn) / tn
    gerr, num, den = {}, 0.0, 0.0
    for k, _ in so.param_shapes(OCFG):
        got = m.grad_view(k).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), k
        if G[k] is None:
            assert float(np.abs(got).max()) == 0.0, "%s: no gradient in the reference, %g here" % (k, float(np.abs(got).max()))
            continue
        want = np.asarray(G[k], np.float64).reshape(got.shape)
        e2, w2 = float(((got - want) ** 2).sum()), float((want ** 2).sum())
        assert w2 > 0.0, k
        gerr[k] = (e2 / w2) ** 0.5
        num, den = num + e2, den + w2
    whole = (num / den) ** 0.5
    worst = max(gerr, key=gerr.get)
    print("%s B %d: worst output %s %.2e, loss %.2e, grad norm %.2e (%.4f), worst tensor %s %.2e, whole gradient %.2e"
          % (tag, B, max((k for k in errs if k not in ("loss", "grad_norm")), key=errs.get),
             max(v for k, v in errs.items() if k not in ("loss", "grad_norm")), errs["loss"], errs["grad_norm"], tn, worst, gerr[worst], whole))
    for k, e in errs.items():
        tol = TOL_LOSS if k == "loss" else TOL_GN if k == "grad_norm" else TOL_OUT
        assert e <= tol, "%s B %d: %s rel err %.3e > %.1e" % (tag, B, k, e, tol)
    for k, e in gerr.items():
        assert e <= tol_tensor, "%s B %d: grad %s relative Frobenius err %.3e > %.2g" % (tag, B, k, e, tol_tensor)
    assert whole <= tol_whole, "%s B %d: whole gradient relative Frobenius err %.3e > %.2g (worst %s %.3e)" % (tag, B, whole, tol_whole, worst, gerr[worst])
    return G


# ---- 1a: one step across the workgroup-per-sequence mappings ---------------------------------------------------------------------------
SPLITS = [(32, 224), (64, 0), (128, 0), (129, 0), (256, 0), (400, 0)]      # (B, b_offset); seq_split 8, 4, 2, 1, 1, 1


@pytest.mark.parametrize("B,b_offset", SPLITS, ids=["B%d" % b for b, _ in SPLITS])
def test_flagship_step_vs_bf16_operand_oracle(B, b_offset):
    """One FusedTrainer step (dropout 0.5, eager) at each seq_split mapping; B 32 is one rank of the 8-GPU strong-scaling run: rows [224, 256)
    of a global batch of 256 with b_offset 224 and the global batch's normalisers.  Logits, every encoder input / decoder output, the
    head-classifier log-probabilities, loss, gradient norm and EVERY parameter gradient against the bf16-operand oracle.  Measured (worst
    output / worst tensor / whole gradient; seq_split workgroups per sequence):
        B  32 (split 8, b_offset 224): 6.8e-3 dec_out.1 / 0.029 encoder.encoder_layers.1.forward_layer.conv1.weight / 0.012
        B  64 (split 4):               6.6e-3 dec_out.1 / 0.025 pos_emb.weight / 9.1e-3
        B 128 (split 2):               6.0e-3 dec_out.0 / 0.019 pos_emb.weight / 6.4e-3
        B 129 (split 1):               6.5e-3 dec_out.0 / 0.023 pos_emb.weight / 7.4e-3
        B 256 (split 1):               6.0e-3 dec_out.0 / 0.019 pos_emb.weight / 5.6e-3
        B 400 (split 1, second id copy loop of k_step_begin): 6.3e-3 dec_out.0 / 0.015 pos_emb.weight / 4.3e-3
    loss within 2.7e-6, gradient norm within 3.0e-4 everywhere."""
    GB = B + b_offset
    gb = synth_batches(1, GB, L, V, seed=100 + B)[0]
    batch = tuple(np.ascontiguousarray(a[b_offset:]) for a in gb)
    norms = _global_norms(gb)
    m = _model()
    P = _params(m)
    tr = _trainer(m)
    tr.step(*batch, norms=norms, b_offset=b_offset)
    torch.cuda.synchronize()
    out, loss, G = _oracle(P, batch, _seed(m), norms=norms, b_offset=b_offset)
    _check_step(m, tr, B, out, loss, G, "split")


# ---- 1b: the benchmarked step exactly: HBM ring of staged batches, graph replay ------------------------------------------------------------
def _bench_step_case():
    """bench.py's run(): stage_ring of the global batches, step_staged with use_graph (step 1: eager warm-up + capture, step 2: the replay).
    Each step is compared against an oracle step started from the GPU's own weights, moments and seed just before it, so the replayed step is
    checked without drift between the two sides; the optimizer's update is checked against the formula on the GPU's own gradient.  Measured
    (sorted and default table gradients alike): step 1 pos_logits 6.7e-3 / pos_emb.weight 0.017 / whole 5.0e-3; step 2 (replay) pos_logits
    8.3e-3 / encoder.encoder_layers.1.forward_layer.conv1.weight 0.024 / whole 6.7e-3."""
    B = CFG["batch"]
    batches = synth_batches(2, B, L, V, seed=100)
    norms = [_global_norms(b) for b in batches]
    m = _model()
    tr = _trainer(m, use_graph=True)
    ring = tr.stage_ring(batches, norms)
    for step in range(2):
        P0 = _flat_params(m, m.flat)
        M0, V0 = tr.m.clone(), tr.v.clone()
        W0 = m.flat.clone()
        tr.step_staged(ring)
        torch.cuda.synchronize()
        out, loss, G = _oracle(P0, batches[step], _seed(m), norms=norms[step])
        _check_step(m, tr, B, out, loss, G, "bench step %d (%s)" % (step + 1, "replay" if step else "eager"))
        _check_adam(m, tr, W0, M0, V0, t=step + 1, clip=CFG["clip"], lr=CFG["lr"])
    return True


def _check_adam(m, tr, W0, M0, V0, t, clip, lr):
    """The optimizer's update of this step from the GPU's OWN gradient: m = b1 m0 + (1 - b1) c g, v = b2 v0 + (1 - b2) (c g)^2 with
    c = min(1, clip / (||g|| + 1e-6)), w = w0 - lr / bc1 * m / (sqrt(v / bc2) + eps) -- fp32 rounding only.  Returns c."""
    g = m.flat_grad.double()
    tn = float(tr.grad_norm())
    c = min(1.0, clip / (tn + 1e-6))
    n = sum(m._views[k][1] for k, _ in so.param_shapes(OCFG))      # the trainable prefix of the flat buffer
    g, M0, V0, W0 = g[:n], M0[:n].double(), V0[:n].double(), W0[:n].double()
    m_want = B1 * M0 + (1 - B1) * c * g
    v_want = B2 * V0 + (1 - B2) * (c * g) ** 2
    mg, vg = tr.m[:n].double(), tr.v[:n].double()
    assert float((mg - m_want).abs().max()) <= 1e-5 * float(m_want.abs().max()), float((mg - m_want).abs().max())
    assert float((vg - v_want).abs().max()) <= 1e-5 * float(v_want.abs().max()), float((vg - v_want).abs().max())
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    dw_want = -lr / bc1 * mg / ((vg / bc2).sqrt() + EPS)
    dw = m.flat[:n].double() - W0
    assert float((dw - dw_want).abs().max()) <= 1e-2 * lr, float((dw - dw_want).abs().max())
    return c


def test_bench_step_sorted_tables_graph_replay():
    """The exact benchmarked step: ADT_ITEM_SORT=1 (bench.py's default, the sorted segmented-sum table gradients; the switch is read once per
    process, so this runs in a child process), B 256, use_graph, ids from the staged HBM ring."""
    code = "import sys; sys.path.insert(0, %r); from tests.test_flagship_batch_hip import _bench_step_case; assert _bench_step_case(); print('bench-step-ok')" % REPO
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ADT_ITEM_SORT="1"), capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "bench-step-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_bench_step_default_tables_graph_replay():
    """The same step with the library default table gradients (float-atomic scatters into the replicas), in this process."""
    assert _bench_step_case()


# ---- 1c: clipping engaged ---------------------------------------------------------------------------------------------------------------
def test_flagship_step_clips_and_adam_moments():
    """clip 0.05 against a gradient norm of about 0.23 on the bench's init and first batch: coefficient about 0.22.  grad_norm() is the norm BEFORE clipping;
    the first-step moments are m = (1 - b1) c g and v = (1 - b2) (c g)^2 -- against the GPU's own gradient to fp32 rounding and against the
    oracle's gradient (weight-decay term of the item table included) to the gradient bound; Adam's first step moves a weight by
    -lr m^ / (sqrt(v^) + eps), which is -lr sign(g) whatever c is, so only the moments catch a wrong or missing clip factor.  Measured: gradient
    norm 0.231, c 0.2163 on both sides; 47 % of the gradient entries are clearly non-zero (the sign check's mask)."""
    B, clip, lr = CFG["batch"], 0.05, CFG["lr"]
    b = synth_batches(1, B, L, V, seed=100)[0]
    m = _model()
    P = _params(m)
    tr = _trainer(m, clip=clip)
    W0, M0, V0 = m.flat.clone(), tr.m.clone(), tr.v.clone()
    tr.step(*b)
    torch.cuda.synchronize()
    out, loss, G = _oracle(P, b, _seed(m))
    _check_step(m, tr, B, out, loss, G, "clip")
    tn = so.grad_norm(G)
    c_ref = clip / (tn + 1e-6)
    assert c_ref < 0.5, "clipping does not engage: oracle grad norm %.4f, clip %.3f" % (tn, clip)
    c = _check_adam(m, tr, W0, M0, V0, t=1, clip=clip, lr=lr)
    assert abs(c - c_ref) <= TOL_GN * c_ref, (c, c_ref)
    n_clear = n_all = 0
    for k, _ in so.param_shapes(OCFG):
        off, n, shape = m._views[k]
        mk, vk = tr.m[off:off + n].double().cpu().numpy(), tr.v[off:off + n].double().cpu().numpy()
        dw = (m.flat[off:off + n].double() - W0[off:off + n].double()).cpu().numpy()
        assert np.abs(dw).max() <= 2 * lr, k
        if G[k] is None:
            assert np.abs(mk).max() == 0.0 and np.abs(vk).max() == 0.0 and np.abs(dw).max() == 0.0, k
            continue
        g = np.asarray(G[k], np.float64).reshape(-1)
        m_ref, v_ref = (1 - B1) * c_ref * g, (1 - B2) * (c_ref * g) ** 2
        em = np.linalg.norm(mk - m_ref) / np.linalg.norm(m_ref)
        ev = np.linalg.norm(vk - v_ref) / np.linalg.norm(v_ref)
        assert em <= TOL_TENSOR, "%s: first moment relative Frobenius err %.3e" % (k, em)
        assert ev <= 2 * TOL_TENSOR + TOL_TENSOR ** 2, "%s: second moment relative Frobenius err %.3e" % (k, ev)
        # where the oracle's gradient is clearly non-zero (well above this element's own GPU-oracle difference), the weight moved by -lr sign(g)
        gg = m.grad_view(k).double().cpu().numpy().reshape(-1)
        clear = np.abs(g) > np.maximum(10 * np.abs(gg - g), 1e3 * EPS / c_ref)
        n_clear, n_all = n_clear + int(clear.sum()), n_all + clear.size
        if clear.any():
            assert np.abs(dw[clear] + lr * np.sign(g[clear])).max() <= 1e-2 * lr, k
    print("clip: coefficient %.4f (oracle %.4f), %.3f of the gradient entries clearly non-zero" % (c, c_ref, n_clear / n_all))
    assert n_clear > 0.3 * n_all, (n_clear, n_all)


# ---- 2: the pinned id ring with the producer ahead of the GPU ----------------------------------------------------------------------------
NSTEP = 6


def _ring_batches(B):
    """Six batches whose padding differs clearly from one to the next (every other batch keeps only its last 60 positions), so a step that
    ran with another batch's normalisers (n_bce differs by a factor of ~3) fails the loss comparison."""
    out = []
    for i, b in enumerate(synth_batches(NSTEP, B, L, V, seed=200)):
        b = tuple(a.copy() for a in b)
        if i % 2:
            for a in b[:3]:
                a[:, :L - 60] = 0
            b[1][:, :L - 59] = 0
            b[3][b[2] == 0] = 0
        out.append(b)
    return out


def _ring_arm(mode, B=256):
    """mode "sort" (ADT_ITEM_SORT=1: bit-equal results), "embed3" / "single" (ADT_ITEM_SORT=0 with the split / single-launch prefetch, lr 0).
    Reference: the six batches through step() with a synchronize after each (the producer never ahead: no prefetch).  Staged: the producer
    writes and publish()es batches k and k + 1 before commit() of step k, no synchronize; with `wrap` the ring counters start at 2^32 - 3."""
    sort = mode == "sort"
    assert (os.environ.get("ADT_ITEM_SORT", "0") != "0") == sort
    lr = CFG["lr"] if sort else 0.0
    batches = _ring_batches(B)
    norms = [_global_norms(b) for b in batches]
    assert len(set(n[0] for n in norms)) == NSTEP
    runs = {}
    for arm in (("ref", "staged", "wrap") if sort else ("ref", "staged")):
        m = _model()
        tr = _trainer(m, lr=lr)
        st = tr._alloc(B)
        base = 0
        if arm == "wrap":
            base = (1 << 32) - 3
            st["nsub"] = base
            st["consumed_np"][0] = base
            st["produced_np"][0] = base
            # state[0]: batches fetched; state[2] == state[0] + 1 would mean "that batch is staged": base (batch base - 1 staged) is not
            st["state"].copy_(torch.tensor(np.array([base, 0, base, 0, base, 0, 0, 0], np.uint32).view(np.int32)))
            torch.cuda.synchronize()
        losses, gns, grads = [], [], []
        if arm == "ref":
            for k in range(NSTEP):
                tr.step(*batches[k], norms=norms[k])
                torch.cuda.synchronize()
                losses.append(tr.loss().clone())
                gns.append(tr.grad_norm().clone())
                grads.append(m.flat_grad.clone())
        else:
            def produce(i):
                views, _ = tr.slot(B, base + i)
                for v, a in zip(views, batches[i]):
                    v[...] = a
                tr.publish(B, base + i, norms[i])
            produce(0)
            for k in range(NSTEP):
                if k + 1 < NSTEP:
                    produce(k + 1)      # the successor is published before this step is committed: the step prefetches it
                tr.commit(B)
                losses.append(tr.loss().clone())      # device-side reads on the step's stream: nothing waits for the GPU
                gns.append(tr.grad_norm().clone())
                grads.append(m.flat_grad.clone())
            torch.cuda.synchronize()
        state = st["state"].cpu().numpy().view(np.uint32).copy()
        expect_staged = 0 if arm == "ref" else NSTEP - 1
        assert int(state[5]) == expect_staged, "%s: %d batches taken from staging, %d steps had their successor published before commit (state %s)" % (
            arm, int(state[5]), expect_staged, state.tolist())
        assert int(state[0]) == (base + NSTEP) & 0xFFFFFFFF, (arm, state.tolist())
        runs[arm] = (torch.stack(losses).cpu().numpy(), torch.stack(gns).cpu().numpy(), grads, m.flat.clone(), tr.m.clone(), tr.v.clone(), m)
    ref = runs["ref"]
    n_tab = ref[6].offsets[2]      # item table + positional table
    for arm in runs:
        if arm == "ref":
            continue
        got = runs[arm]
        assert np.abs(got[0] - ref[0]).max() <= 1e-5 * np.abs(ref[0]).max(), (arm, got[0], ref[0])
        for k in range(NSTEP):
            a, b = got[2][k], ref[2][k]
            assert torch.isfinite(a).all()
            if sort:
                assert torch.equal(a, b), "%s step %d: gradient differs by %g" % (arm, k, float((a - b).abs().max()))
            else:
                assert torch.equal(a[n_tab:], b[n_tab:]), "%s step %d: non-table gradient differs by %g" % (arm, k, float((a[n_tab:] - b[n_tab:]).abs().max()))
                assert float((a[:n_tab] - b[:n_tab]).abs().max()) <= 4e-6 * float(b[:n_tab].abs().max()), (arm, k)
        if sort:
            assert np.array_equal(got[1], ref[1]), (arm, got[1], ref[1])
            for i, what in ((3, "weights"), (4, "first moments"), (5, "second moments")):
                assert torch.equal(got[i], ref[i]), "%s: %s differ by %g" % (arm, what, float((got[i] - ref[i]).abs().max()))
        else:
            assert np.abs(got[1] - ref[1]).max() <= 1e-5 * np.abs(ref[1]).max(), (arm, got[1], ref[1])
            assert torch.equal(got[3], ref[3])      # lr 0: the weights never move
    print("ring %s: %s" % (mode, ", ".join("%s loss %s" % (a, np.round(runs[a][0], 5).tolist()) for a in runs)))
    return True


@pytest.mark.parametrize("arm", ["ADT_ITEM_SORT=1", "ADT_ITEM_SORT=0 ADT_EMBED3=1", "ADT_ITEM_SORT=0 ADT_EMBED3=0"])
def test_pinned_ring_prefetch_is_taken_and_exact(arm):
    """The producer (this process's main thread) runs ahead of the GPU, so every step whose successor was published before it was committed
    prefetches that batch (the loss launch; with ADT_ITEM_SORT=0 ADT_EMBED3=1 half of it rides on the embedding scatter) and the next step
    takes it from staging: the device's count of batches taken from staging must EQUAL the number of such steps.  ADT_ITEM_SORT=1 also runs
    the ring with its 32-bit counters starting at 2^32 - 3, across the wrap: the same count, bit-equal results (with the prefetch's old plain
    unsigned compare the step whose producer count had wrapped skipped it: 4 batches from staging instead of 5).  Own process per arm: the
    switches are read once per process."""
    env = dict(os.environ)
    env.update(kv.split("=") for kv in arm.split())
    mode = "sort" if env["ADT_ITEM_SORT"] == "1" else ("embed3" if env["ADT_EMBED3"] == "1" else "single")
    code = "import sys; sys.path.insert(0, %r); from tests.test_flagship_batch_hip import _ring_arm; assert _ring_arm(%r); print('ring-ok')" % (REPO, mode)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "ring-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def _forward_without_backward_arm():
    """The smallest lean shape (bf16, d 64, H 2, one block, L 16, B 4, V 40).  Batches k and k + 1 are published, step k runs its first kernel and
    its forward + loss launch with the ring arguments (which copies the FIRST half of batch k + 1 into the staging buffer) -- and then no backward.
    Everything the forward saw (model, trainer, ring, staging) stays alive to the end."""
    from adt_amd import ops
    from adt_amd.sasrec.model import SASRecADT
    from adt_amd.sasrec.trainer import FusedTrainer
    from tests.test_hip_kernels import check, embed_bwd3_case, run_embed_bwd3

    class Args:
        device, maxlen, num_heads, num_layers, precision, hidden_units, dropout = "cuda:0", 16, 2, 1, "bf16", 64, 0.2
    B, Ls, Vs = 4, 16, 40
    torch.manual_seed(23)
    m = SASRecADT(1, Vs, Args())
    assert m.bce_deferred()
    tr = FusedTrainer(m, [0.1], [0.05], weight_decay=1e-3, seed=3)
    st = tr._bind(B)
    r = np.random.RandomState(7)
    for k in range(2):
        seq = r.randint(1, Vs + 1, size=(B, Ls))
        seq[:, :3] = 0
        dec = np.roll(seq, 1, 1)
        dec[:, 0] = 0
        pos, neg = (r.randint(1, Vs + 1, size=(B, Ls)) * (seq > 0) for _ in range(2))
        views, _ = tr.slot(B, k)
        for v, a in zip(views, (seq, dec, pos, neg)):
            v[...] = a
        tr.publish(B, k, (float(np.count_nonzero(pos)), float(B * Ls * 64), float(B * Ls * 2)))
    prefetch = (st["ring"], st["n_int"], tr.NSLOTS, st["state"], st["consumed"], st["staging"])
    m.run_step_begin_ring_staged(B, st["ring"], st["n_int"], tr.NSLOTS, tr._devbuf, st["state"], st["consumed"], st["staging"], st["produced"], tr.scal)
    bce = m.run_forward_loss(*tr._ids, B, tr.lambdas1, tr.lambdas2, prefetch=prefetch, bce_side=True)
    assert bce == "fwd"
    torch.cuda.synchronize()
    before = st["state"].cpu().numpy().view(np.uint32).copy()
    assert int(before[0]) == 1 and int(before[4]) == 2 and int(before[2]) == 0, before.tolist()      # batch 0 fetched, batch 1 seen published, nothing staged
    # an unrelated caller of the public entry point on this thread
    case, dE, dP = embed_bwd3_case("sampler", 0.25)
    dE_t, dP_t = run_embed_bwd3(ops, case, 0.25)
    torch.cuda.synchronize()
    after = st["state"].cpu().numpy().view(np.uint32).copy()
    assert int(after[2]) == int(before[2]), "a half-copied staging buffer was marked staged by an unrelated adt_embed_bwd3: state %s -> %s" % (
        before.tolist(), after.tolist())
    assert np.array_equal(after, before), (before.tolist(), after.tolist())
    check(dE_t, dE, 2e-5, "embed_bwd3 dE")
    check(dP_t, dP, 2e-5, "embed_bwd3 dP")
    del tr, m
    return True


def test_forward_without_backward_hands_nothing_to_embed_bwd3():
    """A forward + loss launch that was given the id ring and is not followed by its backward (an error, another trainer, a test) must leave
    nothing behind for the next adt_embed_bwd3 of the host thread: the second half of the split ring prefetch is an argument of
    adt_sasrec_backward_prefetch, not thread state.  (With the hand-over in thread-local variables the public adt_embed_bwd3 launched the
    prefetch variant of its kernel with the earlier step's ring pointers and marked the half-copied staging buffer staged: state[2] 0 -> 2.)
    The result of that adt_embed_bwd3 is the one tests/test_hip_kernels.py expects.  Own process: the switches are read once per process."""
    env = dict(os.environ, ADT_ITEM_SORT="0", ADT_EMBED3="1")
    code = ("import sys; sys.path.insert(0, %r); from tests.test_flagship_batch_hip import _forward_without_backward_arm; "
            "assert _forward_without_backward_arm(); print('handoff-ok')" % REPO)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "handoff-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
