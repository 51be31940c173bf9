"""GPU: the three supernets at the widths the kernels pad, at heads of 128 lanes and (SASRec-ADT) past the resident attention's length
(DESIGN.md section 30): SuperSASRecModel, SuperBertModel and DisenDistSASupernet constructed with allow_lanes=True, against fixtures
recorded from the imported reference supernets (tools/gen_golden_super.py lanes, tools/gen_golden_super_wide.py lanes; dropout 0).

Bounds are those of tests/test_super_d256_hip.py, tests/test_superwide_hip.py and tests/test_superstosa_kl_hip.py, unchanged: activations
2e-4 (fp32) / 4e-2 (bf16 operands), full-sort distances 5e-4 / 6e-2, loss 2e-4, gradient norm 5e-4 (SASRec, BERT) / 1e-3 (STOSA),
gradients 1e-3 / 2e-3, weights after a step 2e-4 or within 1.01 n lr with a median under 0.05 lr.  SASRec-ADT also runs a dropout-on step
against oracle/super_oracle.py; the BERT / STOSA numpy oracles restate the plain models, not the supernets, so those two keep the
dropout-off fixtures.  Every supernet: pad lanes of flat, flat_grad and both Adam moments bitwise +0.0 after 5 clipped, decayed steps
with dropout 0.3; batched candidate evaluation equals one candidate at a time; the tiled twins call no *_lanes op."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import super_oracle as su  # noqa: E402
from tools.gen_golden_inputs import golden_err, sample_idx, seeded_params  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 96
SAS_TAGS = ["w50h1", "w100h2", "l272"]
BERT_TAGS = ["w50h1", "w100h2"]
STOSA_TAGS = ["w50h1", "w100h2", "w100h1"]


class Args:
    pass


def err(got, g, key):
    return golden_err(got.detach().cpu().numpy() if hasattr(got, "detach") else got, g, key, K)


def weights_ok(got, g, key, lr, nsteps=1):
    """2e-4 of the tensor's magnitude, or tests/test_super_d256_hip.py's rule in units of lr (entries whose gradient is rounding noise move
    by a rounding-dependent fraction of lr per step; most must agree far closer)."""
    if err(got, g, key) < 2e-4:
        return True
    t = got.detach().cpu().numpy().astype(np.float64).reshape(-1)
    if key in g.files:
        want, s = np.asarray(g[key], np.float64).reshape(-1), t
    else:
        want, s = np.asarray(g[key + "@sample"], np.float64), t[sample_idx(t.size, K)]
        norm = float(g[key + "@norm"])
        if not abs(np.sqrt((t ** 2).sum()) - norm) < 2e-4 * norm:
            return False
    diff = np.abs(s - want)
    return diff.max() < 1.01 * nsteps * lr and np.median(diff) < 0.05 * lr


def pad_mask(m):
    live = torch.zeros(m.flat.numel(), dtype=torch.bool, device=m.dev)
    live[m.lane_idx.long()] = True
    return ~live


def assert_pads_zero(m, tr):
    """Every element of the padded buffers that is no image of a reference element: +0.0 bit for bit."""
    pad = pad_mask(m)
    assert int(pad.sum()) > 0
    for name, buf in (("flat", m.flat), ("flat_grad", m.flat_grad), ("m", tr.m), ("v", tr.v)):
        bits = buf[pad].view(torch.int32)
        assert int((bits != 0).sum()) == 0, name


def cands_for(g, n, seed):
    nl = int(g["cfg"][4])
    r = np.random.RandomState(seed)
    extra = [[float(x) for x in r.rand(2 * nl)] for _ in range(n)]
    return [[float(x) for x in g["cand"]], [float(x) for x in g["cand2"]]] + extra


def shared_of(g, cands):
    from adt_amd.supersearch import cand_to_block, get_shared
    rc, ic = g["rec_choice"], g["ind_choice"]
    return [get_shared(rc, ic, cand_to_block(rc, ic, c)[0]) for c in cands]


class LaneSpy:
    """Counts the calls of every ops.*_lanes function (and the padded layout's other entry points)."""

    def __init__(self, monkeypatch):
        from adt_amd import ops
        self.calls = {}
        for name in dir(ops):
            if name.endswith("_lanes") or name in ("lane_map", "drop_lanes"):
                monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def spy(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return spy


# ---- SASRec-ADT -------------------------------------------------------------------------------------------------------------------
def sas_case(tag, dropout=0.0):
    g = np.load(os.path.join(GOLD, "super_%s.npz" % tag))
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    cfg = su.Cfg(V, L, d, H, nl, g["rec_choice"], g["ind_choice"], dropout)
    return g, cfg, su.init_params(cfg, int(g["seed"]))


def sas_build(cfg, P, prec, allow=True):
    from adt_amd.sasrec.supersasrec import SuperSASRecModel
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = \
        "cuda:0", cfg.num_heads, cfg.maxlen, cfg.num_layers, cfg.hidden_units, cfg.dropout, prec
    m = SuperSASRecModel(1, cfg.item_num, cfg.rec_choice, cfg.ind_choice, a, **({"allow_lanes": True} if allow else {}))
    if P:
        m.load_numpy(P)
    return m


def rec_err(a, b, H):
    a, b = np.asarray(a, np.float64).reshape(-1, H * H), np.asarray(b, np.float64).reshape(-1, H * H)
    a, b = a[np.lexsort(a.T)], b[np.lexsort(b.T)]      # reference rows are permuted (sasrec/modules.py:518)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


@pytest.mark.parametrize("tag", SAS_TAGS)
def test_sasrec_keyword_and_state_dict(tag):
    from adt_amd import _lib
    g, cfg, P = sas_case(tag)
    with pytest.raises(_lib.AdtError, match="hidden_units in"):
        sas_build(cfg, {}, "f32", allow=False)
    m = sas_build(cfg, P, "f32")
    assert m.hidden_units == cfg.hidden_units and not m.fused_layers()
    sd = m.state_dict()
    assert list(sd) == list(P) or set(sd) == set(P)
    for k, v in P.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].cpu().numpy(), v), k
    assert (m.lanes is None) == (tag == "l272")
    assert m._long_attn == (tag == "l272")
    if m.lanes is not None:
        with pytest.raises(_lib.AdtError, match="padded widths"):
            m.train()
            m(None, g["seq"], g["dec"], g["pos"], g["neg"])


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", SAS_TAGS)
def test_sasrec_forward_and_predict(tag, prec):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = sas_case(tag)
    m = sas_build(cfg, P, prec)
    tr = SuperTrainer(m)
    tol = 2e-4 if prec == "f32" else 4e-2
    errs = {}
    for c, sfx in ((g["cand"], ""), (g["cand2"], "2")):
        tr.set_choice([float(x) for x in c])
        m.eval()
        with torch.no_grad():
            pl, nl, ei, do, rc = m(None, g["seq"], g["dec"], g["pos"], g["neg"])
        errs["pos_logits" + sfx], errs["neg_logits" + sfx] = err(pl, g, "pos_logits" + sfx), err(nl, g, "neg_logits" + sfx)
        if not sfx:
            assert [list(s[0]) for s in m.shared] == g["shared_idx"].tolist()
            for i in range(cfg.num_layers):
                assert tuple(ei[i].shape) == (g["seq"].shape[0], cfg.maxlen, cfg.hidden_units)
                errs["enc_in_%d" % i], errs["dec_out_%d" % i] = err(ei[i], g, "enc_in_%d" % i), err(do[i], g, "dec_out_%d" % i)
                if prec == "f32":
                    errs["rec_%d" % i] = rec_err(rc[i].cpu().numpy(), g["rec_%d" % i], cfg.num_heads)
                else:
                    assert abs(float(rc[i].mean()) - float(g["rec_%d" % i].mean())) < tol
        errs["predict" + sfx] = err(m.predict(None, g["seq"], g["items"]), g, "predict" + sfx)
    print("super sasrec %s %s: worst %.3g (%s)" % (tag, prec, max(errs.values()), max(errs, key=errs.get)))
    for name, e in errs.items():
        assert e < tol, (name, e)


@pytest.mark.parametrize("tag", SAS_TAGS)
def test_sasrec_warmup_steps_fp32(tag):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = sas_case(tag)
    m = sas_build(cfg, P, "f32")
    lr = float(g["lr"])
    tr = SuperTrainer(m, lr=lr, weight_decay=float(g["wd"]), clip=float(g["clip"]))
    tr.set_choice([float(x) for x in g["cand"]])
    tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
    torch.cuda.synchronize()
    e_loss = abs(float(tr.loss()) - float(g["loss"])) / abs(float(g["loss"]))
    e_gn = abs(float(tr.grad_norm()) - float(g["grad_norm"])) / float(g["grad_norm"])
    none = set(str(x) for x in g["grad_none"])
    e_grad = {}
    for k in P:
        if k in none:
            assert float(m.GR(k).abs().max()) == 0.0, k
            assert np.array_equal(m.R(k).cpu().numpy(), P[k]), k      # untouched: no decay, no step
            continue
        e_grad[k] = err(m.GR(k), g, "grad." + k)
    print("super sasrec %s warm-up: loss %.3g grad-norm %.3g gradients %.3g (%s)" % (tag, e_loss, e_gn, max(e_grad.values()), max(e_grad, key=e_grad.get)))
    assert e_loss < 2e-4 and e_gn < 5e-4 and len(e_grad) > 20
    for k, e in e_grad.items():
        assert e < 1e-3, (k, e)
    for step in (1, 2):
        if step == 2:
            tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
            torch.cuda.synchronize()
        keys = sorted({f.split("@")[0][3:] for f in g.files if f.startswith("w%d." % step)})
        assert len(keys) > 10
        for k in keys:
            assert weights_ok(m.R(k), g, "w%d.%s" % (step, k), lr, step), (step, k)


@pytest.mark.parametrize("tag", ["w50h1", "w100h2"])
def test_sasrec_dropout_step_matches_oracle(tag):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = sas_case(tag, dropout=0.3)
    m = sas_build(cfg, P, "f32")
    tr = SuperTrainer(m, lr=1e-3, weight_decay=1e-4)
    cand = [float(x) for x in g["cand"]]
    tr.set_choice(cand)
    tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
    torch.cuda.synchronize()
    seed = int(m._seed.cpu().numpy().view(np.uint32)[0])
    loss, G = su.loss_and_grads(P, cfg, cand, g["seq"], g["dec"], g["pos"], g["neg"], training=True, seed=seed)
    assert abs(float(tr.loss()) - loss) < 2e-4 * abs(loss)
    gmax = max(float(np.abs(v).max()) for v in G.values() if v is not None)
    for k in P:
        if G[k] is not None:
            assert np.abs(m.GR(k).cpu().numpy() - G[k]).max() < 1e-3 * max(np.abs(G[k]).max(), 1e-3 * gmax), k


@pytest.mark.parametrize("tag", ["w50h1", "w100h2"])
def test_sasrec_pad_lanes_stay_zero(tag):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = sas_case(tag, dropout=0.3)
    m = sas_build(cfg, P, "bf16")
    tr = SuperTrainer(m, lr=1e-3, weight_decay=1e-2, clip=0.05)
    r = np.random.RandomState(3)
    for _ in range(5):
        tr.set_choice([float(x) for x in r.rand(2 * cfg.num_layers)])
        tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
    torch.cuda.synchronize()
    assert np.isfinite(float(tr.loss()))
    assert_pads_zero(m, tr)
    # the reference-shaped parameters are the truth between steps: they equal the live lanes
    assert torch.equal(m.compact(m.flat), m.ref_flat)
    # torch's bookkeeping: ranges never trained keep zero moments and no step count
    trained = sorted(tr.steps)
    assert all(1 <= tr.steps[k] <= 5 for k in trained) and tr.steps[trained[0]] == 5


@pytest.mark.parametrize("tag", SAS_TAGS)
def test_sasrec_batched_candidates(tag):
    from adt_amd.supersearch import cand_to_block
    g, cfg, P = sas_case(tag)
    m = sas_build(cfg, P, "f32")
    cands = cands_for(g, 4, 5)
    shared = shared_of(g, cands)
    stats = {}
    ranks = m.predict_rank_candidates(g["seq"], g["items"], shared, stats=stats).cpu().numpy()
    hist = torch.zeros(len(cands), g["items"].shape[1], device=m.dev, dtype=torch.int64)
    m.rank_hist_candidates(g["seq"], m.ids(g["items"]), shared, hist)
    hist = hist.cpu().numpy()
    for p, c in enumerate(cands):
        m.set_choice(cand_to_block(g["rec_choice"], g["ind_choice"], c)[0])
        _, r1 = m.predict_rank(g["seq"], g["items"])
        r1 = r1.cpu().numpy()
        assert (ranks[p] == r1).all(), p
        assert (hist[p] == np.bincount(r1, minlength=hist.shape[1])).all(), p
    assert stats["layer_calls"] < 4 * cfg.num_layers * len(cands)


def test_sasrec_tiled_shapes_take_no_lane_op(monkeypatch):
    """A shape the constructor has always taken: the same flat size and no lane op, with or without the keyword."""
    g = np.load(os.path.join(GOLD, "super_c3.npz"))
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    cfg = su.Cfg(V, L, d, H, nl, g["rec_choice"], g["ind_choice"], 0.0)
    P = su.init_params(cfg, int(g["seed"]))
    from adt_amd.sasrec.supersasrec import SuperTrainer
    spy = LaneSpy(monkeypatch)
    sizes = []
    for allow in (False, True):
        m = sas_build(cfg, P, "f32", allow=allow)
        assert m.lanes is None and m.ref_flat is None and not m._long_attn and not m._general_attn
        sizes.append(m.flat.numel())
        tr = SuperTrainer(m)
        tr.set_choice([float(x) for x in g["cand"]])
        tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
        m.predict_rank_candidates(g["seq"], g["items"], shared_of(g, [[float(x) for x in g["cand"]]]))
        assert abs(float(tr.loss()) - float(g["loss"])) < 2e-4 * abs(float(g["loss"]))
    assert sizes[0] == sizes[1] and not spy.calls, spy.calls


# ---- BERT4Rec-ADT -----------------------------------------------------------------------------------------------------------------
def bert_build(g, prec, allow=True, dropout=0.0):
    from adt_amd.bert4rec.superbert import SuperBertModel
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", L, H, nl, d, 4 * d
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = dropout, dropout, 2, prec
    m = SuperBertModel(1, V, g["rec_choice"], g["ind_choice"], a, **({"allow_lanes": True} if allow else {}))
    m.load_numpy(seeded_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    return m


@pytest.mark.parametrize("tag", BERT_TAGS)
def test_bert_keyword_and_state_dict(tag):
    from adt_amd import _lib
    g = np.load(os.path.join(GOLD, "superbert_%s.npz" % tag))
    with pytest.raises(_lib.AdtError, match="the supernet is built for"):
        bert_build(g, "f32", allow=False)
    torch.manual_seed(5)
    from adt_amd.bert4rec.superbert import SuperBertModel
    V, L, d, H, nl = [int(x) for x in g["cfg"]]
    a = Args()
    a.device, a.maxlen, a.num_heads, a.num_layers, a.hidden_units, a.inner_units = "cuda:0", L, H, nl, d, 4 * d
    a.dropout, a.attention_dropout, a.type_vocab_size, a.precision = 0.0, 0.0, 2, "f32"
    m = SuperBertModel(1, V, g["rec_choice"], g["ind_choice"], a, allow_lanes=True)
    sd = m.state_dict()
    assert m.hidden_units == d and m.lanes is not None and m.vocab == V + 2
    assert tuple(sd["encoder.encoder_layers.0.1.ffn.fc1.weight"].shape) == (4 * d, d)
    assert tuple(sd["encoder.encoder_layers.0.1.head_classifier.weight"].shape) == (H, d // H)
    # the supernet's own initialisation at the reference's shapes and fans: trunc_normal_(std 0.02) within +-2 (absolute), biases U(+-1/sqrt(fan_in))
    w = sd["encoder.encoder_layers.0.1.ffn.fc2.weight"]
    assert 0.015 < float(w.std()) < 0.025 and float(w.abs().max()) <= 2.0
    b = sd["encoder.encoder_layers.0.1.ffn.fc2.bias"]
    assert float(b.abs().max()) <= 1.0 / np.sqrt(4 * d) and float(b.abs().max()) > 0.3 / np.sqrt(4 * d)
    b1 = sd["encoder.encoder_layers.0.1.ffn.fc1.bias"]
    assert 0.9 / np.sqrt(d) < float(b1.abs().max()) <= 1.0 / np.sqrt(d)      # 4 d draws; the padded fan (d_pad) would stay under 0.9 / sqrt(d)
    pad = pad_mask(m)
    assert int((m.flat[pad].view(torch.int32) != 0).sum()) == 0            # live lanes only
    assert torch.equal(m.compact(m.flat), m.ref_flat)
    with pytest.raises(_lib.AdtError, match="padded widths"):
        m.train()
        m(g["src"], g["dec"])


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", BERT_TAGS)
def test_bert_forward_and_predict(tag, prec):
    from adt_amd.bert4rec.superbert import SuperBertTrainer
    g = np.load(os.path.join(GOLD, "superbert_%s.npz" % tag))
    m = bert_build(g, prec)
    tr = SuperBertTrainer(m)
    tr.set_choice([float(x) for x in g["cand"]])
    assert [list(s[0]) for s in m.shared] == g["shared_idx"].tolist()
    assert np.allclose([list(s[1]) for s in m.shared], g["shared_weights"], atol=1e-12)
    m.eval()
    with torch.no_grad():
        logits, ei, do, rc = m(g["src"], g["dec"])
    tol = 2e-4 if prec == "f32" else 4e-2
    errs = {"logits": err(logits, g, "logits")}
    for i in range(int(g["cfg"][4])):
        errs["enc_in_%d" % i], errs["dec_out_%d" % i], errs["rec_%d" % i] = err(ei[i], g, "enc_in_%d" % i), err(do[i], g, "dec_out_%d" % i), err(rc[i], g, "rec_%d" % i)
    errs["predict"] = err(m.predict(None, g["src"], None, None, g["items"]), g, "predict")
    tr.set_choice([float(x) for x in g["cand2"]])
    errs["predict2"] = err(m.predict(None, g["src"], None, None, g["items"]), g, "predict2")
    print("super bert %s %s: worst %.3g (%s)" % (tag, prec, max(errs.values()), max(errs, key=errs.get)))
    for name, e in errs.items():
        assert e < tol, (name, e)


@pytest.mark.parametrize("tag", BERT_TAGS)
def test_bert_warmup_step_fp32(tag):
    from adt_amd.bert4rec.superbert import SuperBertTrainer
    g = np.load(os.path.join(GOLD, "superbert_%s.npz" % tag))
    m = bert_build(g, "f32")
    lr = float(g["lr"])
    tr = SuperBertTrainer(m, lr=lr, weight_decay=float(g["wd"]), clip=float(g["clip"]))
    tr.set_choice([float(x) for x in g["cand"]])
    tr.step(g["src"], g["dec"], g["labels"])
    torch.cuda.synchronize()
    e_loss = abs(float(tr.loss()) - float(g["loss"])) / abs(float(g["loss"]))
    e_gn = abs(float(tr.grad_norm()) - float(g["grad_norm"])) / float(g["grad_norm"])
    none = set(str(x) for x in g["grad_none"])
    e_grad = {}
    for name, _ in m.table:
        key = "grad." + name
        if key in g.files or key + "@norm" in g.files:
            e_grad[name] = err(m.GR(name), g, key)
        elif name in none:
            assert float(m.G(name).abs().max()) == 0.0, name        # the reference leaves these at grad None
    print("super bert %s warm-up: loss %.3g grad-norm %.3g gradients %.3g (%s)" % (tag, e_loss, e_gn, max(e_grad.values()), max(e_grad, key=e_grad.get)))
    assert e_loss < 2e-4 and e_gn < 5e-4 and len(e_grad) > 20
    for name, e in e_grad.items():
        assert e < 1e-3, (name, e)
    for key in [k for k in g.files if k.startswith("w1.")]:
        name = key[3:].replace("@norm", "").replace("@sample", "")
        if name.endswith("key_transfer.bias"):
            continue      # softmax is invariant to a key bias: its gradient is rounding noise, which Adam normalises to +-lr steps
        assert weights_ok(m.R(name), g, "w1." + name, lr), name


@pytest.mark.parametrize("tag", BERT_TAGS)
def test_bert_pad_lanes_stay_zero(tag):
    from adt_amd.bert4rec.superbert import SuperBertTrainer
    g = np.load(os.path.join(GOLD, "superbert_%s.npz" % tag))
    m = bert_build(g, "bf16", dropout=0.3)
    tr = SuperBertTrainer(m, lr=1e-3, weight_decay=1e-2, clip=0.05)
    r = np.random.RandomState(4)
    for _ in range(5):
        tr.set_choice([float(x) for x in r.rand(2 * int(g["cfg"][4]))])
        tr.step(g["src"], g["dec"], g["labels"])
    torch.cuda.synchronize()
    assert np.isfinite(float(tr.loss()))
    assert_pads_zero(m, tr)
    assert torch.equal(m.compact(m.flat), m.ref_flat)


@pytest.mark.parametrize("tag", BERT_TAGS)
def test_bert_batched_candidates(tag):
    from adt_amd.supersearch import cand_to_block
    g = np.load(os.path.join(GOLD, "superbert_%s.npz" % tag))
    m = bert_build(g, "f32")
    nl = int(g["cfg"][4])
    cands = cands_for(g, 5, 3)
    shared = shared_of(g, cands)
    stats = {}
    ranks = m.predict_rank_candidates(g["src"], g["items"], shared, stats=stats).cpu().numpy()
    hist = torch.zeros(len(cands), g["items"].shape[1], device=m.dev, dtype=torch.int64)
    m.rank_hist_candidates(g["src"], g["items"], shared, hist)
    hist = hist.cpu().numpy()
    above = lambda s: (s[:, 1:] > s[:, :1]).sum(1)
    assert (ranks[0] == above(g["predict"])).all() and (ranks[1] == above(g["predict2"])).all()
    for p, c in enumerate(cands):
        m.set_choice(cand_to_block(g["rec_choice"], g["ind_choice"], c)[0])
        _, r1 = m.predict(None, g["src"], None, None, g["items"], want_rank=True)
        r1 = r1.cpu().numpy()
        assert (ranks[p] == r1).all(), p
        assert (hist[p] == np.bincount(r1, minlength=hist.shape[1])).all(), p
    assert stats["layer_calls"] < 4 * nl * len(cands)


def test_bert_tiled_shapes_take_no_lane_op(monkeypatch):
    from adt_amd.bert4rec.superbert import SuperBertTrainer
    g = np.load(os.path.join(GOLD, "superbert_c3.npz"))
    spy = LaneSpy(monkeypatch)
    sizes = []
    for allow in (False, True):
        m = bert_build(g, "f32", allow=allow)
        assert m.lanes is None and m.ref_flat is None
        sizes.append(m.flat.numel())
        tr = SuperBertTrainer(m, lr=float(g["lr"]), weight_decay=float(g["wd"]), clip=float(g["clip"]))
        tr.set_choice([float(x) for x in g["cand"]])
        tr.step(g["src"], g["dec"], g["labels"])
        m.predict_rank_candidates(g["src"], g["items"], shared_of(g, [[float(x) for x in g["cand"]]]))
        assert abs(float(tr.loss()) - float(g["loss"])) < 2e-4 * abs(float(g["loss"]))
    assert sizes[0] == sizes[1] and not spy.calls, spy.calls


# ---- STOSA-ADT, both metrics --------------------------------------------------------------------------------------------------------
def stosa_gold(tag, metric):
    return np.load(os.path.join(GOLD, ("superstosa_kl_%s.npz" if metric == "kl" else "superstosa_%s.npz") % tag))


def stosa_build(g, prec, metric, allow=True, dropout=0.0):
    from adt_amd.stosa.supernet import DisenDistSASupernet
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = "cuda:0", V, L, d, H, nl, nu
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = dropout, dropout, float(g["pvn_weight"]), prec, metric
    m = DisenDistSASupernet(a, g["rec_choice"], g["ind_choice"], allow_kl=True, **({"allow_lanes": True} if allow else {}))
    m.load_numpy(seeded_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"])))
    return m


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", STOSA_TAGS)
def test_stosa_keyword_and_state_dict(tag, metric):
    from adt_amd import _lib
    g = stosa_gold(tag, metric)
    with pytest.raises(_lib.AdtError):
        stosa_build(g, "f32", metric, allow=False)
    m = stosa_build(g, "f32", metric)
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    sd = m.state_dict()
    assert m.hidden_units == d and m.lanes == (H, d // H, 64 if tag != "w100h1" else 128)
    assert tuple(sd["item_encoder.layer.0.1.attention.mean_query.weight"].shape) == (d, d)
    assert tuple(sd["item_encoder.layer.0.1.mean_intermediate.dense_1.weight"].shape) == (4 * d, d)
    assert "decLayerNorm.weight" not in sd
    with pytest.raises(_lib.AdtError, match="padded"):
        m.train()
        m.finetune(g["input_ids"], g["dec_ids"], None)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", STOSA_TAGS)
def test_stosa_forward_and_full_sort(tag, metric, prec):
    from adt_amd.stosa.supernet import SuperStosaTrainer
    g = stosa_gold(tag, metric)
    m = stosa_build(g, prec, metric)
    tr = SuperStosaTrainer(m)
    tr.set_choice([float(x) for x in g["cand"]])
    assert [list(s[0]) for s in m.shared] == g["shared_idx"].tolist()
    m.eval()
    with torch.no_grad():
        mo, co, _, _, ei, er, do = m.finetune(g["input_ids"], g["dec_ids"], None)
    tol = 2e-4 if prec == "f32" else 4e-2
    errs = {"mean_out": err(mo, g, "mean_out"), "cov_out": err(co, g, "cov_out")}
    for i in range(int(g["cfg"][4])):
        for name, t in (("enc_in_mean_%d", ei[i][0]), ("enc_in_cov_%d", ei[i][1]), ("rec_mean_%d", er[i][0]), ("rec_cov_%d", er[i][1]),
                        ("dec_out_mean_%d", do[i][0]), ("dec_out_cov_%d", do[i][1])):
            errs[name % i] = err(t, g, name % i)
    e_one = err(m.predict_full(g["input_ids"]), g, "full_dist")
    dist = m.predict_full_candidates(g["input_ids"], shared_of(g, cands_for(g, 0, 0))).cpu().numpy()
    B = g["input_ids"].shape[0]
    assert np.isfinite(dist).all()
    e_grp = max(golden_err(dist[:B], g, "full_dist", K), golden_err(dist[B:], g, "full_dist2", K))
    print("super stosa %s %s %s: activations %.3g (%s), full_dist %.3g (one) %.3g (candidates)"
          % (tag, metric, prec, max(errs.values()), max(errs, key=errs.get), e_one, e_grp))
    for name, e in errs.items():
        assert e < tol, (name, e)
    assert e_one < (5e-4 if prec == "f32" else 6e-2)
    assert e_grp < (5e-4 if prec == "f32" else 6e-2)


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", STOSA_TAGS)
def test_stosa_warmup_step_fp32(tag, metric):
    from adt_amd.stosa.supernet import SuperStosaTrainer
    g = stosa_gold(tag, metric)
    m = stosa_build(g, "f32", metric)
    lr = float(g["lr"])
    tr = SuperStosaTrainer(m, lr=lr)
    tr.set_choice([float(x) for x in g["cand"]])
    tr.step(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
    torch.cuda.synchronize()
    e_loss = abs(float(tr.loss()) - float(g["loss"])) / abs(float(g["loss"]))
    e_gn = abs(float(tr.grad_norm()) - float(g["grad_norm"])) / float(g["grad_norm"])
    none = set(str(x) for x in g["grad_none"])
    e_grad = {}
    for name, _ in m.table:
        key = "grad." + name
        if key in g.files or key + "@norm" in g.files:
            e_grad[name] = err(m.GR(name), g, key)
        elif name in none:
            assert float(m.G(name).abs().max()) == 0.0, name
    print("super stosa %s %s warm-up: loss %.3g grad-norm %.3g gradients %.3g (%s)"
          % (tag, metric, e_loss, e_gn, max(e_grad.values()), max(e_grad, key=e_grad.get)))
    assert e_loss < 2e-4 and e_gn < 1e-3 and len(e_grad) > 20
    for name, e in e_grad.items():
        assert e < 2e-3, (name, e)
    for key in [k for k in g.files if k.startswith("w1.")]:
        name = key[3:].replace("@norm", "").replace("@sample", "")
        assert weights_ok(m.R(name), g, "w1." + name, lr), name


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", ["w50h1", "w100h1"])
def test_stosa_pad_lanes_stay_zero(tag, metric):
    from adt_amd.stosa.supernet import SuperStosaTrainer
    g = stosa_gold(tag, metric)
    m = stosa_build(g, "bf16", metric, dropout=0.3)
    tr = SuperStosaTrainer(m, lr=1e-3, weight_decay=1e-2)
    tr.clip = 0.05
    r = np.random.RandomState(6)
    for _ in range(5):
        tr.set_choice([float(x) for x in r.rand(2 * int(g["cfg"][4]))])
        tr.step(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
    torch.cuda.synchronize()
    assert np.isfinite(float(tr.loss()))
    assert_pads_zero(m, tr)
    assert torch.equal(m.compact(m.flat), m.ref_flat)


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
@pytest.mark.parametrize("tag", STOSA_TAGS)
def test_stosa_batched_candidates(tag, metric, monkeypatch):
    """predict_full_candidates (under 'kl' through adt_kldist_full_groups_lanes on the packed lane image) and rank_full_candidates, fused
    and row-wise, equal one candidate at a time."""
    from adt_amd import ops
    from adt_amd.supersearch import cand_to_block
    g = stosa_gold(tag, metric)
    m = stosa_build(g, "f32", metric)
    kl = metric == "kl"
    nl, B = int(g["cfg"][4]), g["input_ids"].shape[0]
    cands = cands_for(g, 4, 5)
    shared = shared_of(g, cands)
    spy = LaneSpy(monkeypatch)
    stats = {}
    dist = m.predict_full_candidates(g["input_ids"], shared, stats=stats).cpu().numpy()
    assert dist.shape == (len(cands) * B, m.item_size) and np.isfinite(dist).all()
    if kl:
        assert spy.calls.get("kldist_full_groups_lanes") == 1 and spy.calls.get("kldist_pack_lanes") == 1
        assert "kldist_full_lanes" not in spy.calls
        image = m.kl_item_image()
        assert image[0].shape == (m.item_size, 2 * m.dp)
        split = np.concatenate([m.predict_full_candidates(g["input_ids"], shared[g0:g0 + 4], image=image).cpu().numpy() for g0 in (0, 4)])
    else:
        assert spy.calls.get("wdist_full_lanes") == 1
        split = dist
    assert golden_err(dist[:B], g, "full_dist", K) < 5e-4 and golden_err(dist[B:2 * B], g, "full_dist2", K) < 5e-4
    targets = np.asarray(g["pos_ids"])[:, -1]
    rowwise = kl                       # the fused ranking: Wasserstein, or the row-wise KL divergence under 'kl'
    rank, n_elig, top_idx, top_val = m.rank_full_candidates(g["input_ids"], shared, targets, None, 5, stats=None, rowwise=rowwise)
    assert spy.calls.get("klrow_pack_lanes" if kl else "wdist_pack_lanes", 0) >= 2      # the item image and the user rows
    rank, top_idx = rank.cpu().numpy(), top_idx.cpu().numpy()
    for p, c in enumerate(cands):
        m.set_choice(cand_to_block(g["rec_choice"], g["ind_choice"], c)[0])
        one = m.predict_full(g["input_ids"]).cpu().numpy()
        assert np.abs(dist[p * B:(p + 1) * B] - one).max() <= 1e-5 * np.abs(one).max(), p
        assert np.abs(split[p * B:(p + 1) * B] - one).max() <= 1e-5 * np.abs(one).max(), p
        r1, _, t1, _ = m.rank_full(g["input_ids"], targets, None, 5, rowwise=rowwise)
        assert (rank[p * B:(p + 1) * B] == r1.cpu().numpy()).all(), p
        assert (top_idx[p * B:(p + 1) * B] == t1.cpu().numpy()).all(), p
    assert stats["layer_calls"] < 4 * nl * len(cands)


@pytest.mark.parametrize("metric", ["wasserstein", "kl"])
def test_stosa_tiled_shapes_take_no_lane_op(metric, monkeypatch):
    from adt_amd.stosa.supernet import SuperStosaTrainer
    g = stosa_gold("c3", metric)
    spy = LaneSpy(monkeypatch)
    sizes = []
    for allow in (False, True):
        m = stosa_build(g, "f32", metric, allow=allow)
        assert m.lanes is None and m.ref_flat is None
        sizes.append(m.flat.numel())
        tr = SuperStosaTrainer(m, lr=float(g["lr"]))
        tr.set_choice([float(x) for x in g["cand"]])
        tr.step(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
        m.predict_full_candidates(g["input_ids"], shared_of(g, cands_for(g, 0, 0)))
        assert abs(float(tr.loss()) - float(g["loss"])) < 2e-4 * abs(float(g["loss"]))
    assert sizes[0] == sizes[1] and not spy.calls, spy.calls


def test_stosa_256_lane_heads_stay_refused():
    from adt_amd import _lib
    g = dict(stosa_gold("w50h1", "wasserstein"))
    g["cfg"] = np.array([42, 12, 200, 1, 1, 3])
    with pytest.raises(_lib.AdtError, match="up to 128"):
        stosa_build(g, "f32", "wasserstein")
