"""GPU parity of the SASRec-ADT supernet at widths above 64 (adt_amd/sasrec/supersasrec.py on the stage kernels, general masked attention
at head sizes 128 and 256) against golden tensors recorded from the imported reference (tools/gen_golden_super.py wide: forward and
predict under two block choices, the warm-up loss, every gradient, the weights after one and two Adam steps; dropout 0), against the
numpy oracle with dropout on, batched against one-at-a-time candidate ranks, run-to-run agreement, the one-head 256-wide plain
model (SASRecADTWide) against its fixture, and the reference's default search command end to end.

Tolerances (tests/test_superwide_hip.py): exact-fp32 mode 2e-4 of the tensor magnitude on activations, 1e-3 on gradients; bf16-operand
mode 4e-2 on activations."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sasrec_oracle as so  # noqa: E402
from oracle import super_oracle as su  # noqa: E402
from tools.gen_golden_inputs import golden_err, make_batch, sample_idx  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
K = 96
TAGS = ["d256h1", "d256h2", "d128h1"]


class Args:
    pass


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


def err(got, g, key):
    return golden_err(got.detach().cpu().numpy() if hasattr(got, "detach") else got, g, key, K)


def rec_err(a, b, H):
    a, b = np.asarray(a, np.float64).reshape(-1, H * H), np.asarray(b, np.float64).reshape(-1, H * H)
    a, b = a[np.lexsort(a.T)], b[np.lexsort(b.T)]      # reference rows are permuted (sasrec/modules.py:518)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-6)


def test_width_checks():
    from adt_amd import _lib
    cfg = su.Cfg(10, 50, 256, 1, 1, [0, 0.01], [0, 0.002])
    for d, H, L in ((96, 1, 50), (192, 1, 50), (256, 1, 257), (128, 2, 225), (64, 1, 225)):
        cfg.hidden_units, cfg.num_heads, cfg.maxlen = d, H, L
        with pytest.raises(_lib.AdtError, match="hidden_units in"):
            build(cfg, {}, "f32")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_predict_match_reference(tag, prec):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    assert not m.fused_layers()
    tr = SuperTrainer(m)
    tol = 2e-4 if prec == "f32" else 4e-2
    for c, sfx in ((g["cand"], ""), (g["cand2"], "2")):
        tr.set_choice([float(x) for x in c])
        m.eval()
        pl, nl, ei, do, rc = m(None, g["seq"], g["dec"], g["pos"], g["neg"])
        assert err(pl, g, "pos_logits" + sfx) < tol and err(nl, g, "neg_logits" + sfx) < tol
        if not sfx:
            assert [list(s[0]) for s in m.shared] == g["shared_idx"].tolist()
            for i in range(cfg.num_layers):
                assert err(ei[i], g, "enc_in_%d" % i) < tol and err(do[i], g, "dec_out_%d" % i) < tol
                if prec == "f32":
                    assert rec_err(rc[i].cpu().numpy(), g["rec_%d" % i], cfg.num_heads) < tol
                else:
                    assert abs(float(rc[i].mean()) - float(g["rec_%d" % i].mean())) < tol
        assert err(m.predict(None, g["seq"], g["items"]), g, "predict" + sfx) < tol


def _weights_close(got, g, key, lr, nsteps):
    """tests/test_super_wide_cpu.py: post-step weights in units of lr."""
    t = got.detach().cpu().numpy().astype(np.float64).reshape(-1)
    if key in g.files:
        want, s = np.asarray(g[key], np.float64).reshape(-1), t
    else:
        want, s = np.asarray(g[key + "@sample"], np.float64), t[sample_idx(t.size, K)]
        norm = float(g[key + "@norm"])
        assert abs(np.sqrt((t ** 2).sum()) - norm) < 2e-4 * norm, key
    diff = np.abs(s - want)
    assert diff.max() < 1.01 * nsteps * lr, "%s: %.3g lr" % (key, diff.max() / lr)
    assert np.median(diff) < 0.05 * lr, "%s: median %.3g lr" % (key, np.median(diff) / lr)


@pytest.mark.parametrize("tag", TAGS)
def test_warmup_steps_match_reference_fp32(tag):
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = load_case(tag)
    m = build(cfg, P, "f32")
    lr = float(g["lr"])
    tr = SuperTrainer(m, lr=lr, weight_decay=float(g["wd"]), clip=float(g["clip"]))
    tr.set_choice([float(x) for x in g["cand"]])
    tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
    torch.cuda.synchronize()
    assert abs(float(tr.loss()) - float(g["loss"])) < 2e-4 * abs(float(g["loss"]))
    assert abs(float(tr.grad_norm()) - float(g["grad_norm"])) < 5e-4 * float(g["grad_norm"])
    none = set(str(x) for x in g["grad_none"])
    checked = 0
    for k in P:
        if k in none:
            assert float(m.G(k).abs().max()) == 0.0, k
            assert np.array_equal(m.P(k).cpu().numpy(), P[k]), k      # untouched: no decay, no step
            continue
        assert err(m.G(k), g, "grad." + k) < 1e-3, k
        checked += 1
    assert checked > 20
    for step in (1, 2):
        if step == 2:
            tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
            torch.cuda.synchronize()
        keys = sorted({f.split("@")[0][3:] for f in g.files if f.startswith("w%d." % step)})
        assert len(keys) > 10
        for k in keys:
            _weights_close(m.P(k), g, "w%d.%s" % (step, k), lr, step)


def test_dropout_step_matches_oracle_d256():
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = load_case("d256h1", dropout=0.3)
    m = build(cfg, P, "f32")
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
            assert np.abs(m.G(k).cpu().numpy() - G[k]).max() < 1e-3 * max(np.abs(G[k]).max(), 1e-3 * gmax), k


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["d256h1", "d128h1"])
def test_batched_candidate_ranks(tag, prec):
    from adt_amd.supersearch import cand_to_block, get_shared
    g, cfg, P = load_case(tag)
    m = build(cfg, P, prec)
    rc, ic, nl = g["rec_choice"], g["ind_choice"], cfg.num_layers
    r = np.random.RandomState(5)
    cands = [[float(x) for x in g["cand"]], [float(x) for x in g["cand2"]]] + [[float(x) for x in r.rand(2 * nl)] for _ in range(5)]
    shared = [get_shared(rc, ic, cand_to_block(rc, ic, c)[0]) for c in cands]
    stats = {}
    ranks = m.predict_rank_candidates(g["seq"], g["items"], shared, stats=stats).cpu().numpy()
    for p, c in enumerate(cands):
        m.set_choice(cand_to_block(rc, ic, c)[0])
        _, r1 = m.predict_rank(g["seq"], g["items"])
        assert (ranks[p] == r1.cpu().numpy()).all(), p
    assert stats["layer_calls"] < 4 * nl * len(cands)


def test_identical_steps_agree():
    """Two runs of the same dropout-on step from the same state: the forward (no float atomics) gives the same bits; the gradients
    agree to float-accumulation order (the embedding / item-table scatters and some weight-gradient flushes of the stage kernels add
    with atomics, so the wide supernet step is not bit-reproducible; the d = 64 fused path keeps its own guarantees)."""
    from adt_amd.sasrec.supersasrec import SuperTrainer
    g, cfg, P = load_case("d256h1", dropout=0.3)
    runs = []
    for _ in range(2):
        m = build(cfg, P, "bf16")
        tr = SuperTrainer(m, lr=1e-3, weight_decay=1e-4, seed=11)
        tr.set_choice([float(x) for x in g["cand"]])
        m.eval()
        pl = m(None, g["seq"], g["dec"], g["pos"], g["neg"])[0].cpu().numpy().copy()
        tr.step(g["seq"], g["dec"], g["pos"], g["neg"])
        torch.cuda.synchronize()
        runs.append((pl, m.flat_grad.cpu().numpy().copy(), float(tr.loss())))
        del m, tr
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert abs(runs[0][2] - runs[1][2]) <= 1e-6 * abs(runs[0][2])
    g0, g1 = runs[0][1].astype(np.float64), runs[1][1].astype(np.float64)
    assert np.abs(g0 - g1).max() <= 1e-5 * np.abs(g0).max()


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_wide_model_d256_h1_matches_reference_samples(prec):
    """SASRecADTWide at hidden_units 256, one head (head size 256): tests/golden/sasrec_d256_h1.npz (tools/gen_golden.py d256h1)."""
    from adt_amd.sasrec.model_wide import SASRecADTWide, WideSasrecTrainer
    z = np.load(os.path.join(GOLD, "sasrec_d256_h1.npz"))
    V, L, d, H, nl = [int(x) for x in z["cfg"]]
    assert (d, H) == (256, 1)
    cfg = so.Cfg(V, L, d, H, nl, dropout=0.0)
    seed, B = int(z["seed"]), int(z["B"])
    P = so.init_params(cfg, seed=seed)
    batch = make_batch(np.random.RandomState(seed + 1), B, L, V)
    a = Args()
    a.device, a.num_heads, a.maxlen, a.num_layers, a.hidden_units, a.dropout, a.precision = "cuda:0", H, L, nl, d, 0.0, prec
    m = SASRecADTWide(1, V, a)
    m.load_numpy(P)
    m.eval()
    pl, nlg, ei, do, rc = m(None, *batch)
    tol = 1e-4 if prec == "f32" else 3e-2

    def close(x, y, t, what):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        e = np.abs(x - y).max() / max(np.abs(y).max(), 1e-6)
        assert e < t, "%s: rel err %.3g" % (what, e)
    close(pl.cpu().numpy(), z["pos_logits"], tol, "pos_logits")
    close(nlg.cpu().numpy(), z["neg_logits"], tol, "neg_logits")
    for i in range(nl):
        for nm, t in (("enc_in", ei[i]), ("dec_out", do[i])):
            t = t.cpu().numpy().reshape(-1)
            close(t[sample_idx(t.size, 1024)], z["%s.%d.sample" % (nm, i)], tol, nm)
    close(m.predict(None, batch[0], z["cand"]).cpu().numpy(), z["predict_cand"], tol, "predict")
    if prec != "f32":
        return
    tr = WideSasrecTrainer(m, list(z["lam1"]), list(z["lam2"]), weight_decay=float(z["wd"]))
    tr.step(*batch)
    torch.cuda.synchronize()
    assert abs(float(tr.loss()) - float(z["loss"])) < 1e-4 * abs(float(z["loss"]))
    assert abs(float(tr.grad_norm()) - float(z["total_norm"])) < 3e-4 * float(z["total_norm"])
    for k, _ in so.param_shapes(cfg):
        gk = m.G(k).cpu().numpy().reshape(-1).astype(np.float64)
        if "gnone." + k in z.files:
            assert np.all(gk == 0.0), k
            continue
        gn = float(np.sqrt((gk ** 2).sum()))
        assert abs(gn - float(z["gnorm." + k])) <= 2e-3 * float(z["gnorm." + k]) + 1e-7, k
        close(gk[sample_idx(gk.size)], z["gsample." + k], 2e-3, "grad sample " + k)


def test_reference_default_search_end_to_end(tmp_path):
    """The reference's default search shape (sasrec/evolution.py:31-36: d 256, one head, 4 layers, L 50), passed explicitly, in a child
    process with a time limit: one warm-up epoch, one search epoch, a population of 4."""
    cmd = [sys.executable, "-m", "adt_amd.sasrec.evolution", "--dataset", "ml-1m", "--synthetic", "ml1m-small", "--hidden_units", "256",
           "--num_heads", "1", "--num_layers", "4", "--maxlen", "50", "--warmup_epochs", "1", "--search_epochs", "1", "--population_num", "4",
           "--select_num", "2", "--crossover_num", "1", "--mutation_num", "1", "--eval_set", "128", "--data_dir", str(tmp_path / "data"),
           "--out_dir", str(tmp_path / "res")]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=480)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    files = glob.glob(str(tmp_path / "res" / "*.jsonl"))
    assert len(files) == 1
    recs = [json.loads(l) for l in open(files[0])]
    assert recs and all(np.isfinite(r["auc"]) and 0.0 <= r["auc"] <= 1.0 for r in recs)
    for r in recs:
        assert len(json.loads(r["cand"])) == 8 and len(json.loads(r["rec"])) == 4
