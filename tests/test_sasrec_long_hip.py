"""GPU: SASRec-ADT on the wide HIP path (adt_amd/sasrec/model_wide.py) at maxlen past what the resident attention kernels take (224 rows at
head size <= 64, 256 above): the attention calls go to ops.attn_long_* there (adt_amd/csrc/adt_attn_long.cuh), everything else is row-wise
and unchanged.  Dropout-on parity against the numpy oracle, bf16 evaluation against fp32, a fixture recorded from the reference at L = 272
(tests/golden/sasrec_l272.npz: the flagship width 64 with two heads), the trainer under a HIP graph, the constructor's bound and
adt_amd.sasrec.main end to end.  Tolerances are those of tests/test_sasrec_wide_hip.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sasrec_oracle as so  # noqa: E402
from tools.gen_golden_inputs import make_batch, sample_idx  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
LAM1, LAM2 = [0.104292, 0.065892], [0.100833, 0.000607]


class Args:
    pass


def build(cfg, P, prec, dropout=0.0):
    from adt_amd.sasrec.model_wide import SASRecADTWide
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = "cuda:0", cfg.num_heads, cfg.maxlen, cfg.num_layers, cfg.hidden_units, dropout, prec
    m = SASRecADTWide(1, cfg.item_num, a)
    if P is not None:
        m.load_numpy(P)
    return m


def close(a, b, tol, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)
    print("%s: rel err %.3g (bound %.3g)" % (what, err, tol))
    assert err < tol, "%s: rel err %.3g" % (what, err)


# (d, H, L): the flagship width; a padded head (50 in 64 lanes: the scaled call); one 128-wide head just past its 256 rows
@pytest.mark.parametrize("d,H,L", [(64, 2, 300), (50, 1, 272), (128, 1, 260)])
def test_dropout_step_matches_oracle(d, H, L):
    """tests/test_sasrec_wide_hip.py::test_d256_dropout_step_matches_oracle past the resident kernels' lengths, its bound (5e-4 of the
    tensor's maximum): the long kernels index the attention dropout as the oracle does, over more than one workgroup per (b, h)."""
    V, nl, B, p = 300, 2, 3, 0.3
    cfg = so.Cfg(V, L, d, H, nl, dropout=p)
    P = so.init_params(cfg, seed=5)
    batch = make_batch(np.random.RandomState(6), B, L, V)
    m = build(cfg, P, "f32", p)
    assert m._long_attn
    m.train()
    m.set_seed(777)
    wd = 1e-3
    ids = tuple(m.ids(a) for a in batch)
    norms = torch.tensor([float(np.count_nonzero(batch[2])), B * L * d, B * L * H], device="cuda:0", dtype=torch.float32)
    slots = torch.zeros(2 + 2 * nl, 64, device="cuda:0")
    m.flat_grad.zero_()
    m.loss_forward_backward(ids, LAM1, LAM2, norms, slots)
    torch.cuda.synchronize()
    out = so.forward(P, cfg, *batch, training=True, seed=777)
    _, _, seeds = so.loss_and_seeds(P, cfg, out, batch[2], LAM1, LAM2, wd)
    G = so.backward(P, cfg, out[5], seeds, wd, add_wd=False)
    gmax = max(float(np.abs(g).max()) for g in G.values() if g is not None)
    for k, _ in so.param_shapes(cfg):
        if G[k] is not None:
            err = np.abs(m.GR(k).cpu().numpy() - G[k]).max()
            assert err < 5e-4 * max(np.abs(G[k]).max(), 1e-3 * gmax), (k, err)


def test_bf16_eval_forward_predict_and_full_ranking():
    """bf16 operands in eval mode at (V 300, L 300, d 64, H 2, two layers) against the float32 oracle at the wide path's 3e-2: the training
    forward's outputs, predict on candidates and on every item.  rank_full counts the items scoring above the target; a logit within 3e-2 of
    the largest may move by that much, so the rank must lie between the counts of the fp32 logits above target + 2 tol and above target - 2 tol.
    The number of such near ties is printed."""
    V, L, d, H, nl, B, tol = 300, 300, 64, 2, 2, 3, 3e-2
    cfg = so.Cfg(V, L, d, H, nl, dropout=0.0)
    P = so.init_params(cfg, seed=9)
    r = np.random.RandomState(10)
    batch = make_batch(r, B, L, V)
    m = build(cfg, P, "bf16")
    assert m._long_attn
    m.eval()
    want = so.forward(P, cfg, *batch, training=False)
    pl, nlg, ei, do, rc = m(None, *batch)
    close(pl.cpu().numpy(), want[0], tol, "pos_logits")
    close(nlg.cpu().numpy(), want[1], tol, "neg_logits")
    for i in range(nl):
        close(ei[i].cpu().numpy(), want[2][i], tol, "enc_in.%d" % i)
        close(do[i].cpu().numpy(), want[3][i], tol, "dec_out.%d" % i)
    cand = r.randint(1, V + 1, size=(B, 11)).astype(np.int64)
    close(m.predict(None, batch[0], cand).cpu().numpy(), so.predict(P, cfg, batch[0], cand), tol, "predict")
    full32 = so.predict(P, cfg, batch[0], np.tile(np.arange(V + 1), (B, 1)))
    close(m.predict(None, batch[0], None, full=True).cpu().numpy(), full32, tol, "predict full")
    targets = batch[2][:, -1].astype(np.int64)
    rank, n_elig, top_idx, _ = m.rank_full(batch[0], targets, None, 5)
    rank = rank.cpu().numpy()
    assert list(n_elig.cpu().numpy()) == [V - 1] * B
    margin = 2 * tol * np.abs(full32).max()
    ties = 0
    for b in range(B):
        others = np.delete(full32[b, 1:], targets[b] - 1)
        t = full32[b, targets[b]]
        lo, hi = int((others > t + margin).sum()), int((others > t - margin).sum())
        ties += hi - lo
        assert lo <= rank[b] <= hi, (b, rank[b], lo, hi, int((others > t).sum()))
    print("ranks %s (fp32 %s), %d logits within the tolerance of their target's" % (list(rank), [int((np.delete(full32[b, 1:], targets[b] - 1) > full32[b, targets[b]]).sum())
                                                                                                for b in range(B)], ties))
    ids, _ = m.recommend(batch[0], 5)
    assert torch.equal(ids, top_idx) and int(ids.min()) >= 1


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_l272_matches_reference_samples(prec):
    """tests/test_sasrec_wide_hip.py::test_d256_matches_reference_samples at L = 272, d = 64, H = 2, its tolerances: samples the reference
    itself produced past L = 224 (tools/gen_golden.py long)."""
    from adt_amd.sasrec.model_wide import WideSasrecTrainer
    z = np.load(os.path.join(GOLD, "sasrec_l272.npz"))
    V, L, d, H, nl = [int(x) for x in z["cfg"]]
    assert (L, d, H) == (272, 64, 2)
    cfg = so.Cfg(V, L, d, H, nl, dropout=0.0)
    seed, B = int(z["seed"]), int(z["B"])
    P = so.init_params(cfg, seed=seed)
    batch = make_batch(np.random.RandomState(seed + 1), B, L, V)
    m = build(cfg, P, prec)
    assert m._long_attn
    m.eval()
    pl, nlg, ei, do, rc = m(None, *batch)
    tol = 1e-4 if prec == "f32" else 3e-2
    close(pl.cpu().numpy(), z["pos_logits"], tol, "pos_logits")
    close(nlg.cpu().numpy(), z["neg_logits"], tol, "neg_logits")
    for i in range(nl):
        for nm, t in (("enc_in", ei[i]), ("dec_out", do[i])):
            t = t.cpu().numpy().reshape(-1)
            close(t[sample_idx(t.size, 1024)], z["%s.%d.sample" % (nm, i)], tol, nm)
        rn = float(np.sqrt((rc[i].cpu().numpy().astype(np.float64) ** 2).sum()))      # rows are permuted in the reference: compare the norm
        assert abs(rn - float(z["rec_ind.%d.norm" % i])) < tol * float(z["rec_ind.%d.norm" % i])
    close(m.predict(None, batch[0], z["cand"]).cpu().numpy(), z["predict_cand"], tol, "predict")
    if prec != "f32":
        return
    # the oracle itself against the reference beyond L = 200
    want = so.forward(P, cfg, *batch, training=False)
    close(want[0], z["pos_logits"], 1e-4, "oracle pos_logits")
    tr = WideSasrecTrainer(m, list(z["lam1"]), list(z["lam2"]), weight_decay=float(z["wd"]))
    tr.step(*batch)
    torch.cuda.synchronize()
    print("loss %.7f (ref %.7f) grad norm %.7f (ref %.7f)" % (float(tr.loss()), float(z["loss"]), float(tr.grad_norm()), float(z["total_norm"])))
    assert abs(float(tr.loss()) - float(z["loss"])) < 1e-4 * abs(float(z["loss"]))
    assert abs(float(tr.grad_norm()) - float(z["total_norm"])) < 3e-4 * float(z["total_norm"])
    for k, _ in so.param_shapes(cfg):
        g = m.G(k).cpu().numpy().reshape(-1).astype(np.float64)
        if "gnone." + k in z.files:
            assert np.all(g == 0.0), k
            continue
        gn = float(np.sqrt((g ** 2).sum()))
        assert abs(gn - float(z["gnorm." + k])) <= 2e-3 * float(z["gnorm." + k]) + 1e-7, k
        close(g[sample_idx(g.size)], z["gsample." + k], 2e-3, "grad sample " + k)
        w1 = m.P(k).cpu().numpy().reshape(-1)
        big = np.abs(z["gsample." + k]) > 1e-5
        if big.any():
            assert np.abs(w1[sample_idx(w1.size)] - z["w1sample." + k])[big].max() < 0.05 * 1e-3, k


def test_graph_replay_equals_eager():
    """Two steps of WideSasrecTrainer at maxlen 300 under the HIP graph (an eager warm-up with the capture, then the replay) against two eager
    steps from the same weights, dropout on: the same loss (1e-5) and the same weights, at the bound the suite already holds graph replay
    against eager steps to (tests/dp_nccl_cases.py::test_one_rank_rccl_step_equals_plain_step): the weight gradients of the dense layers are
    summed with float atomics whose order varies from run to run, and Adam's first steps move a weight by about lr whatever the size of its
    gradient, so a gradient of rounding noise around zero whose sign flips moves its weight by up to 2 lr per step.  Fewer than one weight
    in a thousand may differ by more than 1e-5, none by more than 4 lr per step."""
    from adt_amd.sasrec.model_wide import WideSasrecTrainer
    V, L, d, H, nl, B, p = 300, 300, 64, 2, 2, 4, 0.3
    cfg = so.Cfg(V, L, d, H, nl, dropout=p)
    P = so.init_params(cfg, seed=5)
    r = np.random.RandomState(6)
    batches = [make_batch(r, B, L, V) for _ in range(2)]
    outs = []
    for use_graph in (False, True):
        m = build(cfg, P, "bf16", p)
        m.train()
        w0 = m.flat.cpu().numpy().copy()
        tr = WideSasrecTrainer(m, LAM1, LAM2, lr=1e-3, weight_decay=1e-3, clip=5.0, use_graph=use_graph, seed=5)
        for b in batches:
            tr.step(*b)
        torch.cuda.synchronize()
        outs.append((float(tr.loss()), m.flat.cpu().numpy().copy()))
        assert np.isfinite(outs[-1][0]) and np.abs(outs[-1][1] - w0).max() > 1e-3      # two Adam steps of 1e-3 moved the weights
    assert abs(outs[0][0] - outs[1][0]) < 1e-5 * abs(outs[0][0])
    d = np.abs(outs[1][1] - outs[0][1])
    frac, worst = float((d > 1e-5).mean()), float(d.max())
    print("loss %.7f / %.7f; %.3g of the weights differ by more than 1e-5, the worst by %.3g" % (outs[0][0], outs[1][0], frac, worst))
    assert frac < 1e-3 and worst <= 4 * 2 * 1e-3


def test_constructor_takes_1024_and_refuses_1025():
    from adt_amd._lib import AdtError
    m = build(so.Cfg(20, 1024, 64, 2, 1, dropout=0.0), None, "bf16")
    assert m._long_attn and m.maxlen == 1024
    assert not build(so.Cfg(20, 224, 64, 2, 1, dropout=0.0), None, "bf16")._long_attn      # up to their bound the resident kernels, as before
    assert not build(so.Cfg(20, 256, 256, 2, 1, dropout=0.0), None, "bf16")._long_attn
    assert build(so.Cfg(20, 257, 256, 2, 1, dropout=0.0), None, "bf16")._long_attn
    with pytest.raises(AdtError, match="maxlen <= 1024"):
        build(so.Cfg(20, 1025, 64, 2, 1, dropout=0.0), None, "bf16")


@pytest.mark.parametrize("d,H", [(64, 2), (50, 1)])
def test_main_at_maxlen_300_end_to_end(tmp_path, d, H):
    """adt_amd.sasrec.main with --maxlen 300 at the flagship width (past the fused executor's 224 rows the wide path trains and evaluates)
    and at the command line's default width 50 (a padded head)."""
    cmd = [sys.executable, "-m", "adt_amd.sasrec.main", "--dataset", "ml-1m", "--train_dir", "long", "--data_dir", str(tmp_path / "data"), "--synthetic",
           "ml1m-small", "--no_template", "--maxlen", "300", "--hidden_units", str(d), "--num_heads", str(H), "--num_epochs", "1", "--eval_interval", "1"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=480)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    recs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(recs) == 1, p.stdout[-2000:]
    r = recs[0]
    print(r)
    assert np.isfinite(r["loss"])
    for split in ("valid", "test"):
        assert 0.0 <= r[split]["ndcg10"] <= 1.0 and 0.0 <= r[split]["hr10"] <= 1.0 and np.isfinite(r[split]["auc"])
