"""GPU: STOSA-ADT at heads of 128 lanes -- hidden_units 128 / 1 and 256 / 2 as they are, 100 / 1 padded to 128 -- with
DisenDistSAModel(..., allow_wide_heads=True), under both metrics.

The five fixtures of tools/gen_golden_stosa.py:main_hd128 in f32 and bf16 with the bounds tests/test_stosa_oddwidth_hip.py and
tests/test_stosa_kl_oddwidth_hip.py use for theirs (outputs and full sort 1e-4 / 3e-2, gradients 5e-4 of max(|G|, 1e-3 gmax) / relative
Frobenius 0.1, weights after one and three fp32 steps), a dropout-on step against the numpy oracle, pad lanes through training, a checkpoint
round trip, shards and graph replay, ranking, maxlen 272, stosa/main.py end to end, and the constructor's refusals."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import stosa_oracle as so  # noqa: E402
from tests.test_stosa_kl_hip import kl_oracle, kl_rows64  # noqa: E402
from tests.test_stosa_oddwidth_hip import DEV, Args, _batches, make_case, one_pass, pad_mask, rel, stored  # noqa: E402
from tests.test_wattn_hd128_plan_cpu import FIXTURES, K, load_case  # noqa: E402
from tools.gen_golden_inputs import golden_err  # noqa: E402

METRICS = ["wasserstein", "kl"]
ADAM_EPS = 1e-8


def args_of(cfg, prec, metric, dropout=0.0, attention_dropout=0.0):
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = DEV, cfg.item_size, cfg.maxlen, cfg.hidden_units, cfg.num_heads, cfg.num_layers, cfg.num_users
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = dropout, attention_dropout, cfg.pvn_weight, prec, metric
    return a


def build(cfg, P, prec, metric="wasserstein", dropout=0.0, attention_dropout=0.0, **kw):
    from adt_amd.stosa.models import DisenDistSAModel
    kw.setdefault("allow_wide_heads", True)
    m = DisenDistSAModel(args_of(cfg, prec, metric, dropout, attention_dropout), allow_kl_lanes=True, **kw)
    if P is not None:
        m.load_numpy(P)
    return m


def pads_are_zero(m, t):
    """Every float of a flat buffer that no reference element maps to is bit-zero (nothing to check at an unpadded width)."""
    return m.lanes is None or bool((t[pad_mask(m)].view(torch.int32) == 0).all())


def batch_of(g):
    return tuple(g[k] for k in ("input_ids", "dec_ids", "pos_ids", "neg_ids"))


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", list(FIXTURES))
def test_finetune_full_sort_and_loss_parts_match_reference(tag, prec):
    metric = FIXTURES[tag][1]
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec, metric)
    d, H = cfg.hidden_units, cfg.num_heads
    assert m.hd_pad == 128 and m.dp == 128 * H and m.hd == d // H and (m.lanes is None) == (d % 128 == 0) and m.distance_metric == metric
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
    loss, parts = one_pass(m, cfg, batch_of(g), lam1, lam2)
    print("bpr %.7f (%.7f) pvn %.7f (%.7f) auc %.7f (%.7f) loss %.7f (%.7f)" % (parts[0], g["bpr"], parts[1], g["pvn"], parts[2], g["auc"], loss, g["loss"]))
    if prec == "f32":
        assert abs(parts[0] - float(g["bpr"])) < 1e-4 * abs(float(g["bpr"]))
        assert abs(parts[1] - float(g["pvn"])) < 1e-4 * max(abs(float(g["pvn"])), 1e-5)
        assert abs(parts[2] - float(g["auc"])) < 1e-5
        assert abs(loss - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    elif metric == "wasserstein":          # bf16: the loss is a mean of distances of bf16-bound activations (tests/test_stosa_oddwidth_hip.py)
        assert abs(parts[0] - float(g["bpr"])) < 3e-2 * abs(float(g["bpr"])) and abs(loss - float(g["loss"])) < 3e-2 * abs(float(g["loss"]))
    else:                                  # bf16 under KL: finite (tests/test_stosa_kl_oddwidth_hip.py)
        assert np.isfinite(loss)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", list(FIXTURES))
def test_gradients_match_reference(tag, prec):
    metric = FIXTURES[tag][1]
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec, metric)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    one_pass(m, cfg, batch_of(g), lam1, lam2)
    none = set(str(x) for x in g["grad_none"])
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
            assert e < 5e-4, (k, e)
        else:
            e = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-3 * gmax * np.sqrt(want.size))
            assert e < 0.1, (k, e)
        worst = max(worst, (k, e), key=lambda kv: kv[1])
    print(tag, prec, "worst", worst)
    assert pads_are_zero(m, m.flat_grad)


@pytest.mark.parametrize("tag", list(FIXTURES))
def test_weights_after_one_and_three_steps_fp32(tag):
    """The bounds of tests/test_stosa_oddwidth_hip.py::test_weights_after_one_and_three_steps_fp32.  The fixtures keep no weights after step
    1: from zero moments Adam's first step is w0 - lr g / (|g| + eps), formed here from the fixture's own gradient.  stosa_hd128_h2 keeps
    none after step 3 either (it would not fit 300 KB): step 1 only."""
    from adt_amd.stosa.trainer import FusedStosaTrainer
    metric = FIXTURES[tag][1]
    g, cfg, P = load_case(tag)
    m = build(cfg, P, "f32", metric)
    lam1, lam2, lr = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]], float(g["lr"])
    tr = FusedStosaTrainer(m, lam1, lam2, lr=lr)
    none = set(str(x) for x in g["grad_none"])
    has_w3 = any(k.startswith("w3.") for k in g.files)
    assert has_w3 == (tag != "hd128_h2")
    for step in (1, 2, 3) if has_w3 else (1,):
        tr.step(*batch_of(g))
        torch.cuda.synchronize()
        if step == 1:
            assert abs(float(tr.loss()) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
        if step == 2:
            continue
        worst = 0.0
        for k in P:
            now = m.R(k).cpu().numpy()
            if k in none:
                assert np.array_equal(now, P[k]), k          # grad None in the reference: untouched by Adam
                continue
            got, grad = stored(g, "grad." + k, now)          # the entries the fixture keeps of this tensor
            if step == 1:
                w0 = stored(g, "grad." + k, P[k])[0]
                want = w0 - lr * grad / (np.abs(grad) + ADAM_EPS)
            else:
                got, want = stored(g, "w3." + k, now)
            diff = np.abs(got - want)
            big = np.abs(grad) > 1e-5
            worst = max(worst, diff[big].max() / lr if big.any() else 0.0)
            assert (diff[big].max() if big.any() else 0.0) < (0.05 if step == 1 else 0.3) * lr, (step, k)
            assert diff.max() < (1.01 if step == 1 else 3.03) * lr, (step, k)
        print(tag, "step", step, "worst well-conditioned entry: %.3g lr" % worst)
    if m.lanes is not None:
        assert torch.equal(m.compact(m.flat), m.ref_flat)


# ---- dropout on -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [128, 100])
def test_dropout_step_matches_oracle(d, metric):
    """tests/test_stosa_oddwidth_hip.py::test_dropout_step_matches_oracle and its KL twin at 128 / 1 and 100 / 1, their bounds (loss 1e-4,
    gradients 5e-4 of max(|G|, 1e-3 gmax)).  One full row, one mostly padded row and one all-padding row."""
    import contextlib
    cfg, P, batch = make_case(d, 1)
    if metric == "kl" and d == 128:
        for k in P:          # the reference's product of 128 covariances stays finite (tools/gen_golden_stosa.py:main_hd128); the oracle sums logs
            if k.endswith(("cov_query.bias", "cov_key.bias")):
                P[k] = P[k] - np.float32(0.7)
    cfg.dropout, cfg.attention_dropout = 0.3, 0.3
    m = build(cfg, P, "f32", metric, 0.3, 0.3)
    assert (m.lanes is not None) == (d == 100)
    lam1, lam2 = [0.25], [0.15]
    got, _ = one_pass(m, cfg, batch, lam1, lam2, seed=9001)
    with (kl_oracle() if metric == "kl" else contextlib.nullcontext()):
        loss, parts, G = so.loss_and_grads(P, cfg, *batch, lam1, lam2, training=True, seed=9001)
    print("loss %.7f (oracle %.7f)" % (got, loss))
    assert abs(got - loss) < 1e-4 * abs(loss)
    gmax = max(float(np.abs(v).max()) for v in G.values() if v is not None)
    errs = {k: np.abs(m.GR(k).cpu().numpy() - G[k]).max() / max(np.abs(G[k]).max(), 1e-3 * gmax) for k in P if G[k] is not None}
    print("worst", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    for k, e in errs.items():
        assert e < 5e-4, (k, e)
    assert pads_are_zero(m, m.flat_grad)


# ---- the padded layout through training and checkpoints ---------------------------------------------------------------------------------
def _trainer(d, H, seed, metric, prec="bf16", p=0.3, use_graph=False, V=60, L=12):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    torch.manual_seed(seed)
    cfg = so.Cfg(V, L, d, H, 1, num_users=4, pvn_weight=0.1)
    m = build(cfg, None, prec, metric, p, p)
    return m, FusedStosaTrainer(m, [0.2], [0.1], lr=1e-3, weight_decay=1e-3, use_graph=use_graph, seed=5)


@pytest.mark.parametrize("metric", METRICS)
def test_pad_lanes_of_100_stay_zero_through_three_steps(metric):
    m, tr = _trainer(100, 1, 3, metric)
    w0 = m.ref_flat.clone()
    pads = pad_mask(m)
    assert int(pads.sum()) > 0 and m.lanes == (1, 100, 128)
    for b in _batches(3):
        tr.step(*b)
        assert np.isfinite(float(tr.loss()))
    torch.cuda.synchronize()
    for nm, t in (("flat", m.flat), ("flat_grad", m.flat_grad), ("exp_avg", tr.m), ("exp_avg_sq", tr.v)):
        assert (t[pads].view(torch.int32) == 0).all(), nm
        assert bool(torch.isfinite(t).all()), nm
    assert float((m.ref_flat - w0).abs().max()) > 1e-3
    assert torch.equal(m.compact(m.flat), m.ref_flat)


def test_checkpoint_round_trip_at_100(tmp_path):
    from adt_amd import checkpoint as ck
    from adt_amd.stosa.models import param_table
    m1, tr1 = _trainer(100, 1, 11, "wasserstein")
    ref = dict(param_table(60, 12, 100, 1, 1, 4)[0])
    for b in _batches(2):
        tr1.step(*b)
    path = os.path.join(tmp_path, "ck.pt")
    ck.save(path, m1, tr1)
    saved = torch.load(path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == {k: tuple(s) for k, s in ref.items()}
    m2, tr2 = _trainer(100, 1, 99, "wasserstein")            # different init: everything must come from the file
    assert not torch.equal(m2.ref_flat, m1.ref_flat)
    ck.load(path, m2, tr2)
    torch.cuda.synchronize()
    assert torch.equal(m2.ref_flat, m1.ref_flat) and torch.equal(m2.flat, m1.flat)
    assert torch.equal(tr2.m, tr1.m) and torch.equal(tr2.v, tr1.v) and tr2.nstep == 2


@pytest.mark.parametrize("metric", METRICS)
def test_two_shards_and_graph_replay_at_128(metric):
    """tests/test_stosa_oddwidth_hip.py::test_two_shards_and_graph_replay at 128 / 1, its bounds: a batch of 4 split 2 + 2 with global
    normalisers and global dropout indices (b_offset 2 on the second shard) sums to the whole batch's gradient (1e-4); four graph-replayed
    steps equal four eager ones (loss 1e-4, weights 5e-3)."""
    from adt_amd.stosa.trainer import FusedStosaTrainer
    cfg, P, batch = make_case(128, 1, lens=(12, 7, 3, 9))
    cfg.dropout, cfg.attention_dropout = 0.2, 0.2
    lam1, lam2 = [0.3], [0.2]
    nt = int((batch[2] > 0).sum())
    m = build(cfg, P, "f32", metric, 0.2, 0.2)
    grads = []
    for lo, hi in ((0, 4), (0, 2), (2, 4)):
        one_pass(m, cfg, batch, lam1, lam2, lo, hi, seed=31337, B_global=4, nt=nt)
        grads.append(m.flat_grad.clone())
    err = rel((grads[1] + grads[2]).cpu().numpy(), grads[0].cpu().numpy())
    print("shards against the whole batch: %.3g" % err)
    assert err < 1e-4
    outs = []
    for use_graph in (False, True):
        m = build(cfg, P, "bf16", metric, 0.2, 0.2)
        tr = FusedStosaTrainer(m, lam1, lam2, use_graph=use_graph, seed=5)
        for _ in range(4):
            tr.step(*batch)
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().copy()))
    print("eager loss %.7f graph loss %.7f weights %.3g" % (outs[0][0], outs[1][0], rel(outs[1][1], outs[0][1])))
    assert np.isfinite(outs[0][0]) and abs(outs[0][0] - outs[1][0]) < 1e-4 * abs(outs[0][0])
    assert rel(outs[1][1], outs[0][1]) < 5e-3


# ---- ranking ----------------------------------------------------------------------------------------------------------------------------
def _check_ranking(m, inp, D, k, **kw):
    B, V = D.shape
    tol = 1e-4 * np.abs(D).max()
    tgt = np.array([3, 17, 200, 299])
    seen = np.zeros((B, V), np.int8)
    for b in range(B):
        seen[b, inp[b][inp[b] > 0]] = 1
    rank, n_elig, top_idx, top_dist = (t.cpu().numpy() for t in m.rank_full(inp, tgt, seen, k, **kw))
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
    ids, dist = m.recommend(inp, k, seen, **kw)
    assert np.array_equal(ids.cpu().numpy(), top_idx) and np.isfinite(dist.cpu().numpy()).all()


def test_ranking_at_100_wasserstein():
    """rank_full and recommend on the padded tables against a numpy ranking of the materialised distances (predict_full), the way
    tests/test_stosa_oddwidth_hip.py::test_ranking_at_d50 compares them."""
    V, L, k = 300, 12, 5
    cfg, P, batch = make_case(100, 1, V=V, L=L, lens=(12, 7, 3, 9))
    m = build(cfg, P, "f32")
    m.eval()
    D = m.predict_full(batch[0]).cpu().numpy().astype(np.float64)
    assert D.shape == (4, V)
    _check_ranking(m, batch[0], D, k)


def test_ranking_at_100_rowwise_kl():
    """Under KL the per-user ranking is by the row-wise divergence, in float64 here on the live lanes of the model's own last states
    (tests/test_stosa_kl_oddwidth_hip.py::test_kl_rowwise_ranking_at_d50)."""
    V, L, k = 300, 12, 5
    cfg, P, batch = make_case(100, 1, V=V, L=L, lens=(12, 7, 3, 9))
    m = build(cfg, P, "f32", "kl")
    m.eval()
    sm, sc = (x.cpu().numpy() for x in m._last_state(batch[0]))
    live = (np.arange(m.dp) % m.hd_pad) < m.hd
    assert not np.any(sm[:, ~live]) and not np.any(sc[:, ~live])
    tm, tc = torch.tensor(sm[:, live], dtype=torch.float64), torch.tensor(sc[:, live], dtype=torch.float64)
    Em = torch.tensor(m.R("item_mean_embeddings.weight").cpu().numpy(), dtype=torch.float64)
    Ec = torch.nn.functional.elu(torch.tensor(m.R("item_cov_embeddings.weight").cpu().numpy(), dtype=torch.float64)) + 1
    D = np.stack([kl_rows64(tm[b:b + 1].expand(V, -1), tc[b:b + 1].expand(V, -1), Em, Ec).numpy() for b in range(4)])
    assert np.isfinite(D).all()
    _check_ranking(m, batch[0], D, k, rowwise=True)


# ---- maxlen 272 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_maxlen_272_trains_one_step_and_runs_a_full_sort(metric):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    cfg, P, batch = make_case(128, 1, V=60, L=272, lens=(272, 200, 17))
    m = build(cfg, None, "bf16", metric, 0.2, 0.2)
    w0 = m.flat.clone()
    tr = FusedStosaTrainer(m, [0.2], [0.1], lr=1e-3, seed=5)
    tr.step(*batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(tr.loss())) and bool(torch.isfinite(m.flat).all()) and float((m.flat - w0).abs().max()) > 1e-4
    D = m.predict_full(batch[0]).cpu().numpy()
    assert D.shape == (3, 60) and np.isfinite(D).all()
    seen = np.zeros((3, 60), np.int8)
    top, ans = tr.full_sort([(batch[0], seen, batch[2][:, -1:])], topk=10)
    assert top.shape == (3, 10) and (top >= 0).all() and (top < 60).all()


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,extra", [(128, []), (100, ["--distance_metric", "kl", "--device_batches", "--device_scores"])], ids=["128-host", "100-kl-device"])
def test_main_trains_two_epochs(tmp_path, capsys, width, extra):
    """stosa/main.py --synthetic tiny --hidden_units {128, 100} --num_heads 1: two epochs, finite losses and metrics; the checkpoint shows
    the true width.  The data set's template sets the width itself, so it goes through --override too."""
    from adt_amd.stosa.main import main
    out = tmp_path / "out"
    over = {"epochs": 2, "hidden_units": width, "num_heads": 1, "maxlen": 20, "batch_size": 32, "eval_batch_size": 48}
    if "kl" in extra:
        over["distance_metric"] = "kl"
    main(["--dataset", "Beauty", "--data_dir", str(tmp_path / "data") + "/", "--output_dir", str(out) + "/", "--synthetic", "tiny",
          "--hidden_units", str(width), "--num_heads", "1", "--epochs", "2", "--eval_set", "64", "--override", json.dumps(over)] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["epoch"] for l in lines] == [0, 1]
    for l in lines:
        assert np.isfinite(l["rec_cur_loss"]) and np.isfinite(l["auc"]) and l["sequences_per_sec"] > 0
        for key in ("valid_HIT@10", "valid_NDCG@10", "valid_MRR"):
            assert np.isfinite(l[key]) and 0.0 <= l[key] <= 1.0, (key, l)
    ck = [f for f in os.listdir(out) if f.endswith(".pt")]
    assert len(ck) == 1 and "-%d-" % width in ck[0]
    sd = torch.load(os.path.join(out, ck[0]), map_location="cpu")
    assert tuple(sd["item_mean_embeddings.weight"].shape)[1] == width


# ---- the constructor ----------------------------------------------------------------------------------------------------------------------
def test_the_flag_is_an_opt_in_and_the_other_refusals_stay(monkeypatch):
    from adt_amd import ops
    from adt_amd._lib import AdtError
    from adt_amd.stosa.supernet import DisenDistSASupernet
    from adt_amd.stosa.trainer import FusedStosaTrainer
    c128 = make_case(128, 1)[0]
    for metric in METRICS:
        with pytest.raises(AdtError, match="head size") as ei:
            build(c128, None, "f32", metric, allow_wide_heads=False)
        assert "allow_wide_heads=True" in str(ei.value) and "d=128" in str(ei.value)
    for d, H in ((256, 1), (300, 1)):          # 256 lanes stay refused, flag or not, and say why
        with pytest.raises(AdtError, match="head size") as ei:
            build(make_case(d, H)[0], None, "f32")
        assert "256" in str(ei.value)
    with pytest.raises(AdtError, match="kl"):          # KL at a padded width still needs its own flag
        from adt_amd.stosa.models import DisenDistSAModel
        DisenDistSAModel(args_of(make_case(100, 1)[0], "f32", "kl"), allow_wide_heads=True)
    with pytest.raises(AdtError):
        DisenDistSASupernet(args_of(c128, "bf16", "wasserstein"), [0.0, 0.5], [0.0, 0.5])
    # with the flag the attention is the new family, at a short maxlen too; a tiled width never reaches it
    calls = []
    for name in ("wattn_hd128_fwd", "wattn_hd128_bwd", "klattn_hd128_fwd", "klattn_hd128_bwd"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    cfg, _, batch = make_case(64, 4, lens=(12, 7, 3))
    FusedStosaTrainer(build(cfg, None, "bf16", dropout=0.2, attention_dropout=0.2), [0.2], [0.1]).step(*batch)
    assert calls == []
    FusedStosaTrainer(build(c128, None, "bf16"), [0.2], [0.1]).step(*batch)
    assert set(calls) == {"wattn_hd128_fwd", "wattn_hd128_bwd"}
    FusedStosaTrainer(build(make_case(100, 1)[0], None, "bf16", "kl"), [0.2], [0.1]).step(*batch)
    torch.cuda.synchronize()
    assert {"klattn_hd128_fwd", "klattn_hd128_bwd"} <= set(calls)
