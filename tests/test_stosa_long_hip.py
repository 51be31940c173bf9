"""STOSA-ADT past the length the whole-(b, h) attention kernels hold in LDS: DisenDistSAModel at maxlen 272, d 64, one head (head size 64:
ops.wattn_max_len is 141), which runs the streamed kernels of adt_wattn_long.cuh, both metrics.

Against the two fixtures recorded from the imported reference (tests/golden/stosa_l272.npz, stosa_kl_l272.npz; compacted: tensors above 2048
entries are checked on their norm and 1024 strided samples): finetune outputs, full-sort distances, the step-0 loss and gradients, at the
bounds of test_stosa_hip.py / test_stosa_kl_hip.py -- exact fp32 1e-4 activations and loss / 5e-4 gradients, bf16 operands 3e-2 / relative
Frobenius 0.1 (the bf16 loss is held to the bf16 activation bound, 3e-2: it is a mean of such activations' distances).  Then a dropout-on
step against the numpy oracle, a HIP-graph replay against the eager step, a two-shard b_offset split, rank_full / recommend and the fused
full sort, a two-epoch run of stosa/main.py at maxlen 300, and the refusal above 1024."""
import contextlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import stosa_oracle as so, tape as tp  # noqa: E402
from tools.gen_golden_inputs import sample_idx  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METRICS = ["wasserstein", "kl"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


class Args:
    pass


def load_case(metric):
    g = np.load(os.path.join(GOLD, "stosa_kl_l272.npz" if metric == "kl" else "stosa_l272.npz"))
    V, L, d, H, nl, nu = [int(x) for x in g["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, num_users=nu, pvn_weight=float(g["pvn_weight"]))
    P = so.init_params(cfg, int(g["seed"]))
    r = np.random.RandomState(int(g["seed"]) + 1)
    for k in P:
        if k.endswith(".bias") and "LayerNorm" not in k:
            P[k] = (0.02 * r.standard_normal(P[k].shape)).astype(np.float32)
    return g, cfg, P


def build(cfg, P, prec, metric, dropout=0.0, attention_dropout=0.0, maxlen=None):
    from adt_amd.stosa.models import DisenDistSAModel
    a = Args()
    a.device, a.item_size, a.maxlen, a.hidden_units, a.num_heads, a.num_layers, a.num_users = ("cuda:0", cfg.item_size, maxlen or cfg.maxlen, cfg.hidden_units,
                                                                                             cfg.num_heads, cfg.num_layers, cfg.num_users)
    a.dropout, a.attention_dropout, a.pvn_weight, a.precision, a.distance_metric = dropout, attention_dropout, cfg.pvn_weight, prec, metric
    m = DisenDistSAModel(a)
    if maxlen is None:
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
    err = np.abs(a - b).max() / scale
    ok = err < tol
    if norm is not None:
        ok = ok and abs(np.linalg.norm(np.asarray(got, np.float64)) - norm) < tol * max(norm, 1e-9)
    print("  %s %.3g" % (key, err))
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
            assert np.abs(a - b).max() < 5e-4 * floor, (k, np.abs(a - b).max() / floor)
            if norm is not None:
                assert abs(np.linalg.norm(got.astype(np.float64)) - norm) < 5e-4 * max(norm, 1e-3 * gmax * np.sqrt(got.size)), k
        else:
            assert np.linalg.norm(a - b) < 0.1 * max(np.linalg.norm(b), 1e-3 * gmax * np.sqrt(b.size)), k


def loss_weights(cfg, lam1, lam2):
    w = [1.0, 1.0, 0.0]
    for l in range(cfg.num_layers):
        w += [lam1[l]] * 2
    for l in range(cfg.num_layers):
        w += [lam2[l]] * 2
    return np.array(w)


def one_pass(m, g, cfg, lo=0, hi=None, seed=None):
    """loss_forward_backward on rows lo:hi of the fixture batch with the whole batch's normalisers -> (loss slots summed, flat gradient)."""
    B, L = g["input_ids"].shape
    hi = B if hi is None else hi
    m.train()
    if seed is not None:
        m.set_seed(seed)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    st = m.stage(g["input_ids"][lo:hi], g["dec_ids"][lo:hi], g["pos_ids"][lo:hi], g["neg_ids"][lo:hi], n_target_global=int((g["pos_ids"] > 0).sum()))
    norms = torch.tensor([0.0, B * L * cfg.hidden_units, B * L * cfg.num_heads], device="cuda:0")
    slots = torch.zeros(3 + 4 * cfg.num_layers, 64, device="cuda:0")
    m.flat_grad.zero_()
    m.loss_forward_backward(st, lam1, lam2, norms, slots, b_offset=lo)
    torch.cuda.synchronize()
    return float((slots.sum(1).cpu().numpy() * loss_weights(cfg, lam1, lam2)).sum()), m.flat_grad.cpu().numpy().copy()


def test_the_model_takes_the_long_path_exactly_past_the_bound():
    from adt_amd import _lib, ops
    g, cfg, P = load_case("wasserstein")
    assert ops.wattn_max_len(64) == 141 and ops.wattn_max_len(16) == ops.wattn_max_len(32) == 256 and ops.wattn_max_len(128) == 0
    assert build(cfg, P, "f32", "wasserstein")._long_attn
    assert not build(cfg, P, "f32", "kl", maxlen=141)._long_attn and build(cfg, P, "f32", "kl", maxlen=142)._long_attn
    assert build(cfg, P, "bf16", "wasserstein", maxlen=1024)._long_attn
    with pytest.raises(_lib.AdtError, match="maxlen"):
        build(cfg, P, "bf16", "wasserstein", maxlen=1025)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("metric", METRICS)
def test_finetune_and_predict_full_match_reference(metric, prec):
    g, cfg, P = load_case(metric)
    m = build(cfg, P, prec, metric)
    m.eval()
    mo, co, _, margins, enc_in, enc_rec, dec_out = m.finetune(g["input_ids"], g["dec_ids"], np.zeros(len(g["input_ids"]), np.int64))
    tol = 1e-4 if prec == "f32" else 3e-2
    print(metric, prec)
    assert close(g, "mean_out", mo.cpu().numpy(), tol) and close(g, "cov_out", co.cpu().numpy(), tol)
    for i in range(cfg.num_layers):
        assert close(g, "enc_in_mean_%d" % i, enc_in[i][0].cpu().numpy(), tol) and close(g, "enc_in_cov_%d" % i, enc_in[i][1].cpu().numpy(), tol)
        assert close(g, "rec_mean_%d" % i, enc_rec[i][0].cpu().numpy(), tol) and close(g, "rec_cov_%d" % i, enc_rec[i][1].cpu().numpy(), tol)
        assert close(g, "dec_out_mean_%d" % i, dec_out[i][0].cpu().numpy(), tol) and close(g, "dec_out_cov_%d" % i, dec_out[i][1].cpu().numpy(), tol)
    assert close(g, "full_dist", m.predict_full(g["input_ids"], g["dec_ids"]).cpu().numpy(), tol)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("metric", METRICS)
def test_step0_loss_and_gradients_match_reference(metric, prec):
    g, cfg, P = load_case(metric)
    m = build(cfg, P, prec, metric)
    loss, _ = one_pass(m, g, cfg)
    print(metric, prec, "loss", loss, "reference", float(g["loss"]))
    assert abs(loss - float(g["loss"])) < (1e-4 if prec == "f32" else 3e-2) * abs(float(g["loss"]))
    grads_match(g, P, lambda k: m.G(k).cpu().numpy(), prec)


# ---- the numpy oracle with the KL distances swapped in (as in test_stosa_kl_hip.py) -------------------------------------------
def _recip(a):
    r = (np.float32(1) / a.v).astype(np.float32)
    out = tp.Var(r, (a,))
    out.vjp = lambda gr: a.acc(-gr * r * r)
    return out


def _tpose(x):
    return tp.transpose(x, tuple(range(x.v.ndim - 2)) + (x.v.ndim - 1, x.v.ndim - 2))


def tape_kl_distance(m1, c1, m2, c2):
    ic2 = _recip(c2)
    df = tp.sub(m2, m1)
    s = tp.add(tp.sum_(tp.mul(c1, ic2), axis=-1), tp.sum_(tp.mul(tp.mul(df, ic2), df), axis=-1))
    det = tp.sub(tp.sum_(tp.log(c2), axis=-1), tp.sum_(tp.log(c1), axis=-1))
    return tp.scale(tp.add(tp.add_const(s, -float(m1.v.shape[1])), det), 0.5)


def tape_kl_distance_matmul(m1, c1, m2, c2):
    ic2 = _recip(c2)
    logdet = tp.sub(_tpose(tp.sum_(tp.log(c2), axis=-1, keepdims=True)), tp.sum_(tp.log(c1), axis=-1, keepdims=True))
    mean = tp.matmul(tp.square(tp.sub(m1, m2)), _tpose(ic2))
    trace = tp.matmul(ic2, _tpose(c1))
    return tp.scale(tp.add_const(tp.add(tp.add(logdet, mean), trace), -float(m1.v.shape[-1])), 0.5)


@contextlib.contextmanager
def oracle_for(metric):
    saved = so.wasserstein_distance, so.wasserstein_distance_matmul
    if metric == "kl":
        so.wasserstein_distance, so.wasserstein_distance_matmul = tape_kl_distance, tape_kl_distance_matmul
    try:
        yield so
    finally:
        so.wasserstein_distance, so.wasserstein_distance_matmul = saved


@pytest.mark.parametrize("metric", METRICS)
def test_training_step_with_dropout_matches_oracle(metric):
    """Dropout 0.3 everywhere: the streamed kernels draw the attention's keep decisions at the oracle's indices ((b H + h) L + i) L + j."""
    g, cfg, P = load_case(metric)
    cfg.dropout, cfg.attention_dropout = 0.3, 0.3
    m = build(cfg, P, "f32", metric, 0.3, 0.3)
    got, _ = one_pass(m, g, cfg, seed=9001)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    with oracle_for(metric):
        loss, parts, G = so.loss_and_grads(P, cfg, g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"], lam1, lam2, training=True, seed=9001)
    print(metric, "loss", got, "oracle", loss)
    assert abs(got - loss) < 1e-4 * abs(loss)
    gmax = max(float(np.abs(v).max()) for v in G.values() if v is not None)
    for k in P:
        if G[k] is not None:
            err = np.abs(m.G(k).cpu().numpy() - G[k]).max() / max(np.abs(G[k]).max(), 1e-3 * gmax)
            assert err < 5e-4, (k, err)


@pytest.mark.parametrize("metric", METRICS)
def test_two_shard_split_equals_the_whole_batch(metric):
    g, cfg, P = load_case(metric)
    grads = []
    for lo, hi in ((0, 2), (0, 1), (1, 2)):
        m = build(cfg, P, "f32", metric, 0.2, 0.2)
        grads.append(one_pass(m, g, cfg, lo, hi, seed=31337)[1])
    e = rel(grads[1] + grads[2], grads[0])
    print(metric, "shards vs whole", e)
    assert e < 1e-4


@pytest.mark.parametrize("metric", METRICS)
def test_graph_replay_equals_the_eager_step(metric):
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g, cfg, P = load_case(metric)
    lam1, lam2 = [float(x) for x in g["lambda1"]], [float(x) for x in g["lambda2"]]
    outs = []
    for use_graph in (False, True):
        m = build(cfg, P, "bf16", metric, 0.2, 0.2)
        tr = FusedStosaTrainer(m, lam1, lam2, use_graph=use_graph, seed=5)
        for _ in range(4):
            tr.step(g["input_ids"], g["dec_ids"], g["pos_ids"], g["neg_ids"])
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().copy()))
    print(metric, "loss eager / graph", outs[0][0], outs[1][0], "weights", rel(outs[1][1], outs[0][1]))
    assert np.isfinite(outs[0][0]) and abs(outs[0][0] - outs[1][0]) < 1e-4 * abs(outs[0][0])
    assert rel(outs[1][1], outs[0][1]) < 5e-3


# ---- ranking ---------------------------------------------------------------------------------------------------------------
def seen_matrix(g, V):
    B = len(g["input_ids"])
    seen = np.zeros((B, V), np.uint8)
    for b in range(B):
        seen[b, g["input_ids"][b][-30:]] = 1       # the last 30 items of each history: plenty of the 39 items stay eligible
    seen[:, 0] = 0
    return seen


def check_topk(ids, dist, D, seen, k, tol, what):
    """ids / dist against reference distances D (B, V): unseen items >= 1, no repeats, each returned distance within tol of its id's, ascending,
    and the k-th within 2 tol of the true k-th."""
    for b in range(len(D)):
        got = ids[b]
        assert (got >= 1).all() and len(set(got.tolist())) == k and (seen[b, got] == 0).all(), (what, b, got)
        assert (np.abs(dist[b] - D[b, got]) <= tol).all() and (np.diff(dist[b]) >= 0).all(), (what, b)
        Db = np.where(seen[b] > 0, np.inf, D[b])
        Db[0] = np.inf
        assert D[b, got[-1]] <= np.sort(Db)[k - 1] + 2 * tol, (what, b)


def test_rank_full_recommend_and_fused_full_sort_wasserstein():
    from adt_amd.stosa.trainer import FusedStosaTrainer
    g, cfg, P = load_case("wasserstein")
    m = build(cfg, P, "f32", "wasserstein")
    V, k = cfg.item_size, 10
    D = g["full_dist"].astype(np.float64)           # the reference's own distances of this batch
    tol = 1e-4 * np.abs(D).max()                    # the fp32 bound of full_dist above
    seen = seen_matrix(g, V)
    target = g["pos_ids"][:, -1].astype(np.int32)
    ids, dist = m.recommend(g["input_ids"], k, seen=seen)
    check_topk(ids.cpu().numpy(), dist.cpu().numpy().astype(np.float64), D, seen, k, tol, "recommend")
    rank, nel, ti, td = m.rank_full(g["input_ids"], target, seen, topk=k)
    rank, nel = rank.cpu().numpy(), nel.cpu().numpy()
    item = np.arange(V)
    for b in range(len(D)):
        other = (item >= 1) & ((seen[b] == 0) | (item == target[b])) & (item != target[b])
        assert nel[b] == other.sum()
        lo, hi = (other & (D[b] < D[b, target[b]] - tol)).sum(), (other & (D[b] < D[b, target[b]] + tol)).sum()
        assert lo <= rank[b] <= hi, (b, lo, int(rank[b]), hi)
    tr = FusedStosaTrainer(m, [0.1], [0.05])
    batches = [(g["input_ids"], seen, target[:, None])]
    want, ans_w = tr.full_sort(batches, topk=k)
    got, ans_g = tr.full_sort(batches, topk=k, fused=True)
    assert np.array_equal(ans_w, ans_g) and got.shape == want.shape == (len(D), k)
    for b in range(len(D)):
        Db = np.sort(np.where(seen[b] > 0, np.inf, D[b]))
        if Db[k] - Db[k - 1] > 2 * tol:
            assert set(got[b].tolist()) == set(want[b].tolist()), b
        assert (seen[b, got[b]] == 0).all() and len(set(got[b].tolist())) == k


def test_rank_full_and_recommend_rowwise_kl():
    """Under KL the per-user ranking is by the row-wise divergence (kl_distance of the last state from each item), in float64 here."""
    g, cfg, P = load_case("kl")
    m = build(cfg, P, "f32", "kl")
    V, k = cfg.item_size, 10
    sm, sc = (x.cpu().numpy().astype(np.float64) for x in m._last_state(g["input_ids"]))
    Em = P["item_mean_embeddings.weight"].astype(np.float64)
    Ec = P["item_cov_embeddings.weight"].astype(np.float64)
    Ec = np.where(Ec > 0, Ec, np.exp(np.minimum(Ec, 0)) - 1) + 1
    D = np.stack([((sc[b] / Ec).sum(-1) + ((Em - sm[b]) ** 2 / Ec).sum(-1) - Em.shape[1] + (np.log(Ec).sum(-1) - np.log(sc[b]).sum())) / 2
                  for b in range(len(sm))])
    tol = 1e-4 * np.abs(D).max()
    seen = seen_matrix(g, V)
    ids, dist = m.recommend(g["input_ids"], k, seen=seen, rowwise=True)
    check_topk(ids.cpu().numpy(), dist.cpu().numpy().astype(np.float64), D, seen, k, tol, "recommend rowwise")
    target = g["pos_ids"][:, -1].astype(np.int32)
    rank, nel, ti, td = m.rank_full(g["input_ids"], target, seen, topk=k, rowwise=True)
    item = np.arange(V)
    for b in range(len(D)):
        other = (item >= 1) & ((seen[b] == 0) | (item == target[b])) & (item != target[b])
        lo, hi = (other & (D[b] < D[b, target[b]] - tol)).sum(), (other & (D[b] < D[b, target[b]] + tol)).sum()
        assert int(nel[b]) == other.sum() and lo <= int(rank[b]) <= hi, (b, lo, int(rank[b]), hi)


# ---- the command line -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--device_batches", "--device_scores", "--distance_metric", "kl"]], ids=["host-wasserstein", "device-kl"])
def test_main_trains_two_epochs_at_maxlen_300(tmp_path, capsys, extra):
    """stosa/main.py --synthetic at --maxlen 300 --num_heads 1 (head size 64, the streamed kernels; the HIP graph is on by default): two epochs
    with finite losses and metrics.  The template of the data set sets maxlen and num_heads itself, so they go through --override too."""
    from adt_amd.stosa.main import _write_synthetic, main
    data = tmp_path / "data"
    data.mkdir()
    _write_synthetic(str(data / "Beauty.txt"), users=96, items=150, seed=3)
    over = {"epochs": 2, "maxlen": 300, "num_heads": 1, "batch_size": 32, "eval_batch_size": 48}
    main(["--dataset", "Beauty", "--data_dir", str(data) + "/", "--output_dir", str(tmp_path / "out") + "/", "--synthetic", "1", "--maxlen", "300",
          "--num_heads", "1", "--epochs", "2", "--eval_set", "64", "--override", json.dumps(over)] + extra)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["epoch"] for l in lines] == [0, 1]
    for l in lines:
        assert np.isfinite(l["rec_cur_loss"]) and np.isfinite(l["auc"]) and l["sequences_per_sec"] > 0
        for key in ("valid_HIT@10", "valid_NDCG@10", "valid_MRR"):
            assert np.isfinite(l[key]) and 0.0 <= l[key] <= 1.0, (key, l)
