"""GPU parity of the SASRec-ADT supernet (adt_amd/sasrec/supersasrec.py, through the C ABI) against the golden tensors
recorded from the imported reference (SuperSASRecModel + the _train_warmup loop body, dropout 0) and against the numpy
oracle with dropout ON.  Tolerances: exact-fp32 MFMA mode 1e-4 (activations) / 5e-4 (gradients) of the tensor magnitude;
bf16-operand mode 3e-2 on activations."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import super_oracle as su  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Args:
    pass


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


def load_case(tag, dropout=0.0):
    g = np.load(os.path.join(GOLD, "super_%s.npz" % tag))
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    cfg = su.Cfg(V, L, d, H, nl, g["rec_choice"], g["ind_choice"], dropout)
    return g, cfg, su.init_params(cfg, int(g["seed"]))


def build(cfg, P, prec):
    from adt_amd.sasrec.supersasrec import SuperSASRecModel
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = "cuda:0", cfg.num_heads, cfg.maxlen, cfg.num_layers, cfg.hidden_units, cfg.dropout, prec
    m = SuperSASRecModel(1, cfg.item_num, cfg.rec_choice, cfg.ind_choice, a)
    m.load_numpy(P)
    return m


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["c3", "l2"])
def test_forward_and_predict_match_reference(tag, prec):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    tr = SuperTrainer(m)
    tr.set_choice([float(x) for x in g["cand"]])
    assert [list(s[0]) for s in m.shared] == g["shared_idx"].tolist()
    m.eval()
    pl, nl, ei, do, rc = m(None, g["seq"], g["dec"], g["pos"], g["neg"])
    tol = 1e-4 if prec == "f32" else 3e-2
    assert rel(pl.cpu().numpy(), g["pos_logits"]) < tol and rel(nl.cpu().numpy(), g["neg_logits"]) < tol
    H2 = cfg.num_heads ** 2
    for i in range(cfg.num_layers):
        assert rel(ei[i].cpu().numpy(), g["enc_in_%d" % i]) < tol and rel(do[i].cpu().numpy(), g["dec_out_%d" % i]) < tol
        a, b = rc[i].cpu().numpy().reshape(-1, H2), g["rec_%d" % i].reshape(-1, H2)     # reference rows are permuted (modules.py:518)
        if prec == "f32":
            assert rel(a[np.lexsort(a.T)], b[np.lexsort(b.T)]) < tol
        else:
            assert abs(a.mean() - b.mean()) < tol
    assert rel(m.predict(None, g["seq"], g["items"]).cpu().numpy(), g["predict"]) < tol
    sd = m.state_dict()
    assert set(sd) == set(P) and all(tuple(sd[k].shape) == P[k].shape for k in P)


@pytest.mark.parametrize("tag", ["c3", "l2"])
def test_warmup_step_matches_reference_fp32(tag):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P, "f32")
    tr = SuperTrainer(m, lr=float(g["lr"]), weight_decay=float(g["wd"]), clip=float(g["clip"]))
    tr.set_choice([float(x) for x in g["cand"]])
    tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
    torch.cuda.synchronize()
    assert abs(float(tr.loss()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    assert abs(float(tr.grad_norm()) - float(g["grad_norm"])) < 3e-4 * float(g["grad_norm"])
    none = set(str(x) for x in g["grad_none"])
    gmax = max(float(np.abs(g["grad." + k]).max()) for k in P if k not in none)
    lr = float(g["lr"])
    for k in P:
        got_g = m.G(k).cpu().numpy()
        if k in none:
            assert np.all(got_g == 0.0), k
            assert np.array_equal(m.P(k).cpu().numpy(), P[k]), k      # untouched: no decay, no step
            continue
        want = g["grad." + k]
        assert np.abs(got_g - want).max() < 5e-4 * max(np.abs(want).max(), 1e-3 * gmax), k
        if ("w1." + k) in g.files:
            diff = np.abs(m.P(k).cpu().numpy().astype(np.float64) - g["w1." + k])
            big = np.abs(want) > 1e-5
            assert (diff[big].max() if big.any() else 0.0) < 0.05 * lr, k
            assert diff.max() < 1.01 * lr, k


def test_warmup_step_with_dropout_matches_oracle():
    g, cfg, P = load_case("l2", dropout=0.3)
    from adt_amd.sasrec.supersasrec import SuperTrainer
    m = build(cfg, P, "f32")
    tr = SuperTrainer(m, lr=1e-3, weight_decay=1e-4)
    cand = [float(x) for x in g["cand"]]
    tr.set_choice(cand)
    tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
    torch.cuda.synchronize()
    seed = int(m._seed.cpu().numpy().view(np.uint32)[0])
    loss, G = su.loss_and_grads(P, cfg, cand, g["seq"], g["dec"], g["pos"], g["neg"], training=True, seed=seed)
    assert abs(float(tr.loss()) - loss) < 1e-4 * abs(loss)
    gmax = max(float(np.abs(v).max()) for v in G.values() if v is not None)
    for k in P:
        if G[k] is not None:
            assert np.abs(m.G(k).cpu().numpy() - G[k]).max() < 5e-4 * max(np.abs(G[k]).max(), 1e-3 * gmax), k


@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("tag", ["c3", "l2"])
def test_grouped_candidate_layers_match_stage_kernels(tag, dropout, monkeypatch):
    """bf16 mode runs the four selected candidate layers of a depth on the per-sequence fused layer kernels (mixing weight as output
    epilogue / gradient prologue, adt_seq_{enc,dec}_layer_{fwd,bwd}); ADT_SUPER_FUSED=0 keeps one stage-kernel sequence per candidate.
    Same weights, batch and dropout seed: loss within 1e-2 relative, whole gradient within 6 % relative Frobenius (two bf16 roundings of
    the same arithmetic), every tensor the reference leaves at grad None exactly zero in both."""
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = load_case(tag, dropout)
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("ADT_SUPER_FUSED", fused)
        m = build(cfg, P, "bf16")
        assert m.fused_layers() == (fused == "1" and cfg.maxlen % 4 == 0)
        tr = SuperTrainer(m, lr=float(g["lr"]), weight_decay=float(g["wd"]), clip=float(g["clip"]), seed=7)
        tr.set_choice([float(x) for x in g["cand"]])
        m.train()
        ids = tuple(m.ids(g[k]) for k in ("seq", "dec", "pos", "neg"))
        B, L = ids[0].shape
        norms = torch.tensor([float(np.count_nonzero(g["pos"])), float(B * L * cfg.hidden_units), float(B * L * cfg.num_heads)], device=m.dev)
        tr.loss_slots.zero_()
        m.flat_grad.zero_()
        m.loss_forward_backward(ids, tr.rec_weights, tr.ind_weights, norms, tr.loss_slots)
        torch.cuda.synchronize()
        res.append((float(tr.loss()), m.flat_grad.clone(), m))
    (l1, g1, m1), (l0, g0, m0) = res
    if not m1.fused_layers():
        pytest.skip("maxlen %d: the fused layer kernels need L %% 4 == 0" % cfg.maxlen)
    assert abs(l1 - l0) < 1e-2 * abs(l0)
    assert float((g1 - g0).norm()) < 0.06 * float(g0.norm())
    for name in [str(x) for x in g["grad_none"]]:
        assert float(m1.G(name).abs().max()) == 0.0, name


# ---- zero mixing weights, and the fused layer kernels at a second depth -----------------------------------------------------------------
def run_path(cfg, P, cand, batch, fused, monkeypatch, seed=7):
    """One loss_forward_backward of the bf16 supernet on the fused layer kernels (fused "1") or the stage kernels ("0"):
    -> (loss, {name: gradient}, the dropout seed it ran with, the model)."""
    from adt_amd.sasrec.supersasrec import SuperTrainer
    monkeypatch.setenv("ADT_SUPER_FUSED", fused)
    m = build(cfg, P, "bf16")
    assert m.fused_layers() == (fused == "1")
    tr = SuperTrainer(m, lr=1e-3, weight_decay=1e-4, clip=5.0, seed=seed)
    tr.set_choice([float(x) for x in cand])
    m.train()
    ids = tuple(m.ids(a) for a in batch)
    B, L = ids[0].shape
    norms = torch.tensor([float(np.count_nonzero(batch[2])), float(B * L * cfg.hidden_units), float(B * L * cfg.num_heads)], device=m.dev)
    tr.loss_slots.zero_()
    m.flat_grad.zero_()
    m.loss_forward_backward(ids, tr.rec_weights, tr.ind_weights, norms, tr.loss_slots)
    torch.cuda.synchronize()
    return float(tr.loss()), {k: m.G(k).cpu().numpy().astype(np.float64) for k in P}, int(m._seed.cpu().numpy().view(np.uint32)[0]), m


def frob(got, want, floor=0.0):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), floor, 1e-30))


def flat_of(G, names):
    return np.concatenate([np.asarray(G[k], np.float64).ravel() for k in names])


@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("cand", [[0.0, 0.3], [0.0, 0.0]], ids=["w0.4-0-0.6-0", "w1-0-0-0"])
def test_zero_weight_candidates_contribute_nothing(cand, dropout, monkeypatch):
    """Candidate probabilities that land on a choice-table entry give mixing weights of exactly 0 (here (0.4, 0, 0.6, 0) and (1, 0, 0, 0)).  The
    layer kernels read a scale of 0 as "scale 1, plain store" (include/adt_hip.h), so the fused path must not run such a candidate: before it
    skipped them, the last zero-weight candidate's unscaled output replaced the mix and its backward ran at weight 1.  Fused against the stage
    kernels with the bounds of test_grouped_candidate_layers_match_stage_kernels (loss 1e-2, whole gradient 6 %); both against the fp32 oracle:
    loss within this file's bf16 bound of 3e-2, whole gradient within 6 %, the figure test_hip_model holds a bf16 step to against the fp32
    oracle; every tensor of a candidate that enters with weight 0 only has a gradient of exactly zero."""
    g, cfg, P = load_case("c3", dropout)
    shared = su.get_shared(cfg, su.cand_to_block(cfg, cand)[0])
    assert sorted(w for _, ws in shared for w in ws)[:2] == [0.0, 0.0]
    batch = tuple(g[k] for k in ("seq", "dec", "pos", "neg"))
    l1, g1, seed1, m1 = run_path(cfg, P, cand, batch, "1", monkeypatch)
    l0, g0, seed0, m0 = run_path(cfg, P, cand, batch, "0", monkeypatch)
    assert seed1 == seed0
    loss, G = su.loss_and_grads(P, cfg, cand, *batch, training=True, seed=seed1)
    live = [k for k in P if G[k] is not None]
    a1, a0, want = flat_of(g1, live), flat_of(g0, live), flat_of(G, live)
    print("loss fused %.6f stage %.6f oracle %.6f ; gradient fused-stage %.4f fused-oracle %.4f stage-oracle %.4f"
          % (l1, l0, loss, frob(a1, a0), frob(a1, want), frob(a0, want)))
    zero = set()
    for depth, (idxs, ws) in enumerate(shared):
        on = {i for i, w in zip(idxs, ws) if w != 0.0}
        zero |= {k for i, w in zip(idxs, ws) if w == 0.0 and i not in on for k in P
                 if k.startswith("encoder.encoder_layers.%d.%d." % (depth, i)) or k.startswith("decoder.decoder_layers.%d.%d." % (depth, i))}
    assert len(zero) >= 30
    for k in sorted(zero):
        assert float(np.abs(g1[k]).max()) == 0.0 and float(np.abs(g0[k]).max()) == 0.0, k
        assert G[k] is None or float(np.abs(G[k]).max()) == 0.0, k
    assert abs(l1 - l0) < 1e-2 * abs(l0)
    assert frob(a1, a0) < 0.06
    for name, l, a in (("fused", l1, a1), ("stage", l0, a0)):
        assert abs(l - loss) < 3e-2 * abs(loss), name
        assert frob(a, want) < 0.06, name
    for k in P:
        if G[k] is None:
            assert float(np.abs(g1[k]).max()) == 0.0, k


def test_fresh_model_without_a_choice_runs_no_candidate(monkeypatch):
    """A freshly constructed model has all four weights of every depth at 0: the mix is zero on both paths, and the fused path launches nothing
    instead of storing candidate 0 unscaled."""
    g, cfg, P = load_case("c3")
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("ADT_SUPER_FUSED", fused)
        m = build(cfg, P, "bf16")
        assert m.fused_layers() == (fused == "1") and all(w == 0.0 for _, ws in m.shared for w in ws)
        m.eval()
        outs.append(m(None, g["seq"], g["dec"], g["pos"], g["neg"]))
    for a, b in zip(outs[0][3], outs[1][3]):
        assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0      # decoder outputs: an empty mix
    assert rel(outs[0][0].cpu().numpy(), outs[1][0].cpu().numpy()) < 3e-2


PARITY_2L = {}


@pytest.mark.parametrize("H", [2, 4])
def test_two_layer_supernet_fused_per_tensor_vs_oracle(H, monkeypatch):
    """The first shape at which depth 1 runs on the fused layer kernels: x.g is accumulated (gx_acc = 1) and feats.g receives two depths.  An
    oracle-initialised two-layer supernet, L 12, B 256, p 0.3, four non-zero weights per depth.  The super oracle has no bf16-operand mode, so
    the bound is measured the way tests/seq_layer_cases.py measures it, from a second bf16 evaluation of the same arithmetic: the stage-kernel
    path and the fused path are each compared with the fp32 oracle, per tensor (relative Frobenius; a tensor under 1e-3 of the largest is
    measured against that scale), and the fused path may be no further than 1.5 x the stage path and never further than 0.15, what
    test_hip_model._lean_bounds allows a bf16 gradient against the fp32 oracle.  B is 256 because both errors are dominated by the ReLU gates
    that operand rounding moves across zero, a few per hundred rows and not the same ones on the two paths: at B 16 (118 live
    rows) the ratio of ONE candidate's tensors was measured between 0.2 and 7 from one dropout seed to the next, in both directions; at about
    1,600 live rows there are enough of them for the ratio to mean something.  ADT_SEQ_LAYER_PARITY_OUT=<file>: the figures are appended
    to that report under "two_layer"."""
    import json
    g = np.load(os.path.join(GOLD, "super_c3.npz"))
    V, L, B = 40, 12, 256
    cfg = su.Cfg(V, L, 64, H, 2, g["rec_choice"], g["ind_choice"], 0.3)
    P = su.init_params(cfg, 5)
    cand = [0.15, 0.62, 0.81, 0.33]
    assert all(w > 0.0 for _, ws in su.get_shared(cfg, su.cand_to_block(cfg, cand)[0]) for w in ws)
    from tools.gen_golden_inputs import make_batch
    batch = make_batch(np.random.RandomState(9), B, L, V)
    l1, g1, seed1, m1 = run_path(cfg, P, cand, batch, "1", monkeypatch)
    l0, g0, seed0, m0 = run_path(cfg, P, cand, batch, "0", monkeypatch)
    assert seed1 == seed0
    loss, G = su.loss_and_grads(P, cfg, cand, *batch, training=True, seed=seed1)
    live = [k for k in P if G[k] is not None]
    assert sum(k.startswith("encoder.encoder_layers.1.") for k in live) == 4 * 14 and sum(k.startswith("decoder.decoder_layers.1.") for k in live) == 4 * 14
    gmax = max(float(np.linalg.norm(G[k])) for k in live)
    # Both paths add B * L = 3072 fp32 terms into every gradient element, the fused one with atomics in any order: T * 2^-24 = 1.8e-4 of the
    # measuring scale is what the number format leaves undetermined, and a ratio of two errors below it compares summation orders, not bf16
    # roundings (measured there: the decoder's self-attention bias gradients, 9.5e-5 against 5.7e-5 of the floor scale, i.e. 1e-7 of the
    # largest gradient).  Above it the ratio holds as stated.
    fp32_floor = B * L * 2.0 ** -24
    bad, worst = [], {"ratio": 0.0}
    for k in live:
        e1, e0 = frob(g1[k], G[k], 1e-3 * gmax), frob(g0[k], G[k], 1e-3 * gmax)
        print("H%d %-60s fused %.4f stage %.4f" % (H, k, e1, e0))
        if e0 > fp32_floor and e1 / e0 > worst["ratio"]:
            worst = {"ratio": round(e1 / e0, 4), "fused": round(e1, 5), "stage": round(e0, 5), "tensor": k}
        if not (e1 <= max(1.5 * e0, fp32_floor) and e1 <= 0.15):
            bad.append((k, e1, e0))
    worst["worst_fused"] = round(max(frob(g1[k], G[k], 1e-3 * gmax) for k in live), 5)
    print("H%d worst %r ; loss fused %.6f stage %.6f oracle %.6f" % (H, worst, l1, l0, loss))
    path = os.environ.get("ADT_SEQ_LAYER_PARITY_OUT")
    if path:
        PARITY_2L["H%d" % H] = worst
        rep = json.load(open(path)) if os.path.exists(path) else {}
        rep["two_layer"] = dict(PARITY_2L, what="supernet L 12, B 256, p 0.3, two depths: per-tensor relative Frobenius error of the fused and the stage-kernel bf16 "
                                                "paths against the fp32 oracle; worst fused / stage ratio (allowed 1.5) and worst fused error (allowed 0.15)")
        with open(path, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)
            f.write("\n")
    assert abs(l1 - loss) < 3e-2 * abs(loss) and abs(l0 - loss) < 3e-2 * abs(loss)
    assert not bad, bad
    for k in P:
        if G[k] is None:
            assert float(np.abs(g1[k]).max()) == 0.0, k
