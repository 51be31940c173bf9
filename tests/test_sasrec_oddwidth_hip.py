"""GPU: SASRec-ADT at widths that are not multiples of 64 -- the CLI default hidden_units 50 (one head; two heads of 25, padded
to 32) and 100 (two heads of 50, padded to 64) -- on the wide HIP path (adt_amd/sasrec/model_wide.py, adt_amd/csrc/adt_lanes.cuh).
Reference parity against tests/golden/sasrec_w*.npz with the tolerances of tests/test_sasrec_wide_hip.py, dropout-on parity against
the numpy oracle, the LayerNorm kernels alone, and the properties of the padded layout: pad lanes stay exactly zero, checkpoints
and parameters show the reference's shapes only."""
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
ODD = ["sasrec_w50_h1", "sasrec_w50_h2", "sasrec_w100_h2"]
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


def pad_mask(m):
    """True on every float of the flat layout that no reference element maps to (pad lanes and alignment gaps)."""
    mask = torch.ones(m.n_flat, dtype=torch.bool, device=m.dev)
    mask[m.lane_idx.long()] = False
    return mask


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", ODD)
def test_matches_reference_samples(name, prec):
    """tests/test_sasrec_wide_hip.py::test_d256_matches_reference_samples at the odd widths, its tolerances."""
    from adt_amd.sasrec.model_wide import WideSasrecTrainer
    z = np.load(os.path.join(GOLD, name + ".npz"))
    V, L, d, H, nl = [int(x) for x in z["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, dropout=0.0)
    seed, B = int(z["seed"]), int(z["B"])
    P = so.init_params(cfg, seed=seed)
    batch = make_batch(np.random.RandomState(seed + 1), B, L, V)
    m = build(cfg, P, prec)
    assert m.lanes is not None and m.dp % 64 == 0 and m.dp > d
    m.eval()
    pl, nlg, ei, do, rc = m(None, *batch)
    tol = 1e-4 if prec == "f32" else 3e-2
    close(pl.cpu().numpy(), z["pos_logits"], tol, "pos_logits")
    close(nlg.cpu().numpy(), z["neg_logits"], tol, "neg_logits")
    for i in range(nl):
        for nm, t in (("enc_in", ei[i]), ("dec_out", do[i])):
            assert tuple(t.shape) == (B, L, d)
            t = t.cpu().numpy().reshape(-1)
            close(t[sample_idx(t.size, 1024)], z["%s.%d.sample" % (nm, i)], tol, nm)
        rn = float(np.sqrt((rc[i].cpu().numpy().astype(np.float64) ** 2).sum()))      # rows are permuted in the reference: compare the norm
        assert abs(rn - float(z["rec_ind.%d.norm" % i])) <= tol * float(z["rec_ind.%d.norm" % i])     # one head: log_softmax over one value, both exactly 0
    close(m.predict(None, batch[0], z["cand"]).cpu().numpy(), z["predict_cand"], tol, "predict")
    if prec != "f32":
        return
    tr = WideSasrecTrainer(m, list(z["lam1"]), list(z["lam2"]), weight_decay=float(z["wd"]))
    tr.step(*batch)
    torch.cuda.synchronize()
    print("loss %.7f (ref %.7f) grad norm %.7f (ref %.7f)" % (float(tr.loss()), float(z["loss"]), float(tr.grad_norm()), float(z["total_norm"])))
    assert abs(float(tr.loss()) - float(z["loss"])) < 1e-4 * abs(float(z["loss"]))
    assert abs(float(tr.grad_norm()) - float(z["total_norm"])) < 3e-4 * float(z["total_norm"])
    for k, shape in so.param_shapes(cfg):
        assert tuple(m.GR(k).shape) == tuple(shape), k
        g = m.GR(k).cpu().numpy().reshape(-1).astype(np.float64)
        if "gnone." + k in z.files:
            assert np.all(g == 0.0), k
            continue
        gn = float(np.sqrt((g ** 2).sum()))
        assert abs(gn - float(z["gnorm." + k])) <= 2e-3 * float(z["gnorm." + k]) + 1e-7, k
        close(g[sample_idx(g.size)], z["gsample." + k], 2e-3, "grad sample " + k)
        w1 = m.R(k).cpu().numpy().reshape(-1)
        big = np.abs(z["gsample." + k]) > 1e-5
        if big.any():
            assert np.abs(w1[sample_idx(w1.size)] - z["w1sample." + k])[big].max() < 0.05 * 1e-3, k


@pytest.mark.parametrize("p", [0.5, 0.2])
@pytest.mark.parametrize("d,H", [(50, 1), (100, 2)])
def test_dropout_step_matches_oracle(d, H, p):
    """tests/test_sasrec_wide_hip.py::test_d256_dropout_step_matches_oracle at the odd widths, its bound: every dropout site must
    index the counter RNG by the TRUE width (row * d + column), where a register quad straddles two rows."""
    V, L, nl, B = 50, 24, 2, 3
    cfg = so.Cfg(V, L, d, H, nl, dropout=p)
    P = so.init_params(cfg, seed=5)
    batch = make_batch(np.random.RandomState(6), B, L, V)
    m = build(cfg, P, "f32", p)
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
    loss, _, seeds = so.loss_and_seeds(P, cfg, out, batch[2], LAM1, LAM2, wd)
    G = so.backward(P, cfg, out[5], seeds, wd, add_wd=False)
    gmax = max(float(np.abs(g).max()) for g in G.values() if g is not None)
    for k, _ in so.param_shapes(cfg):
        if G[k] is not None:
            err = np.abs(m.GR(k).cpu().numpy() - G[k]).max()
            assert err < 5e-4 * max(np.abs(G[k]).max(), 1e-3 * gmax), (k, err)
    assert float(m.flat_grad[pad_mask(m)].abs().max()) == 0.0


@pytest.mark.parametrize("H,hd,hd_pad", [(1, 50, 64), (2, 25, 32), (2, 50, 64)])
def test_layernorm_lanes_against_float64(H, hd, hd_pad):
    from adt_amd import ops
    T, d, dp, eps = 77, H * hd, H * hd_pad, 1e-8             # 77 rows: not a multiple of the 16-row tile
    live = (np.arange(dp) % hd_pad) < hd
    r = np.random.RandomState(H * 100 + hd)
    X, dY = np.zeros((T, dp), np.float32), np.zeros((T, dp), np.float32)
    gam, bet = np.zeros(dp, np.float32), np.zeros(dp, np.float32)
    X[:, live] = r.randn(T, d) * 2 + 0.5
    dY[:, live] = r.randn(T, d)
    gam[live], bet[live] = 1 + 0.3 * r.randn(d), 0.2 * r.randn(d)
    dev = "cuda:0"
    tX, tdY, tg, tb = (torch.from_numpy(a).to(dev) for a in (X, dY, gam, bet))
    Y = ops.layernorm_lanes_fwd(tX, tg, tb, eps, (H, hd, hd_pad)).cpu().numpy()
    dX0 = 0.1 * r.randn(T, dp).astype(np.float32) * live
    tdX, tdg, tdb = torch.from_numpy(dX0.astype(np.float32)).to(dev), torch.zeros(dp, device=dev), torch.zeros(dp, device=dev)
    ops.layernorm_lanes_bwd(tdY, tX, tg, eps, tdX, True, tdg, tdb, (H, hd, hd_pad))
    tdX2 = torch.full((T, dp), 7.0, device=dev)
    ops.layernorm_lanes_bwd(tdY, tX, tg, eps, tdX2, False, torch.zeros(dp, device=dev), torch.zeros(dp, device=dev), (H, hd, hd_pad))
    torch.cuda.synchronize()
    x, dy, g = X[:, live].astype(np.float64), dY[:, live].astype(np.float64), gam[live].astype(np.float64)
    mu = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + eps)
    xh = (x - mu) * rstd
    dxh = dy * g
    dx = rstd * (dxh - dxh.mean(1, keepdims=True) - xh * (dxh * xh).mean(1, keepdims=True))
    close(Y[:, live], xh * g + bet[live], 2e-6, "y")
    close(tdX.cpu().numpy()[:, live], dx + dX0[:, live], 1e-5, "dx (accumulated)")
    close(tdX2.cpu().numpy()[:, live], dx, 1e-5, "dx")
    close(tdg.cpu().numpy()[live], (dy * xh).sum(0), 1e-5, "dgamma")
    close(tdb.cpu().numpy()[live], dy.sum(0), 1e-5, "dbeta")
    for nm, t in (("y", Y), ("dx", tdX.cpu().numpy()), ("dx overwrite", tdX2.cpu().numpy())):
        assert (t[:, ~live].view(np.uint32) == 0).all(), nm          # bit-exact +0.0
    for nm, t in (("dgamma", tdg), ("dbeta", tdb)):
        assert (t.cpu().numpy()[~live].view(np.uint32) == 0).all(), nm


def _trainer(d, H, seed, p=0.3, prec="f32", V=300, L=24, nl=2, use_graph=False, **kw):
    from adt_amd.sasrec.model_wide import WideSasrecTrainer
    torch.manual_seed(seed)
    cfg = so.Cfg(V, L, d, H, nl, dropout=p)
    m = build(cfg, None, prec, p)
    for _, q in m.named_parameters():
        if q.dim() >= 2:
            torch.nn.init.xavier_normal_(q.data)
    m.train()
    return m, WideSasrecTrainer(m, LAM1, LAM2, lr=1e-3, weight_decay=1e-3, clip=0.25, use_graph=use_graph, seed=5, **kw)


def _batches(L, n=5, B=16, V=300):
    r = np.random.RandomState(1)
    out = []
    for _ in range(n):
        seq = r.randint(1, V + 1, size=(B, L)); seq[:, :7] = 0
        dec = np.roll(seq, 1, 1); dec[:, 0] = 0
        out.append((seq, dec, r.randint(1, V + 1, size=(B, L)) * (seq > 0), r.randint(1, V + 1, size=(B, L)) * (seq > 0)))
    return out


@pytest.mark.parametrize("d,H", [(50, 1), (50, 2), (100, 2)])
def test_pad_lanes_stay_zero_through_adam(d, H):
    """Five steps, dropout, weight decay and an active clip (0.25, below every step's gradient norm): every float of the weights, the
    gradient and both moments that is not a reference element is exactly 0.0, and the weights did move."""
    m, tr = _trainer(d, H, 3, prec="bf16")
    w0 = m.ref_flat.clone()
    pads = pad_mask(m)
    assert int(pads.sum()) > 0
    for b in _batches(24):
        tr.step(*b)
        assert float(tr.grad_norm()) > 0.25       # the clip is active
    torch.cuda.synchronize()
    for nm, t in (("flat", m.flat), ("flat_grad", m.flat_grad), ("exp_avg", tr.m), ("exp_avg_sq", tr.v)):
        assert (t[pads].view(torch.int32) == 0).all(), nm
    assert float((m.ref_flat - w0).abs().max()) > 1e-3
    assert torch.equal(m.compact(m.flat), m.ref_flat)


def test_padding_is_invisible_in_checkpoints(tmp_path):
    from adt_amd import checkpoint as ck
    from adt_amd.sasrec.model import param_table
    d, H, L = 50, 2, 24
    m, tr = _trainer(d, H, 11)
    ref = dict(param_table(300, L, d, H, 2))
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in ref.items()}
    assert [n for n, _ in m.named_parameters()] == list(sd.keys())
    batches = _batches(L, n=4)
    for b in batches:
        tr.step(*b)
    want = m.ref_flat.clone()

    m1, tr1 = _trainer(d, H, 11)
    for b in batches[:2]:
        tr1.step(*b)
    path = os.path.join(tmp_path, "ck.pt")
    ck.save(path, m1, tr1)
    saved = torch.load(path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == {k: tuple(s) for k, s in ref.items()}
    m2, tr2 = _trainer(d, H, 99)               # different init: everything must come from the file
    ck.load(path, m2, tr2)
    assert tr2.nstep == 2 and float(tr2.scal[2]) == 2.0
    for b in batches[2:]:
        tr2.step(*b)
    dlt = (m2.ref_flat - want).abs()           # the bound of tests/test_checkpoint_hip.py::test_resume_equals_uninterrupted (float atomics)
    assert float((dlt > 1e-5).float().mean()) < 1e-3 and float(dlt.max()) <= 4e-3

    # torch.optim.Adam state: reference shapes out, and back in bit for bit
    osd = ck.to_torch_adam_state(tr1, skip_untrained=False)
    params = list(m1.parameters())
    assert [tuple(osd["state"][i]["exp_avg"].shape) for i in range(len(params))] == [tuple(q.shape) for q in params]
    opt = torch.optim.Adam(params, lr=1e-3, betas=tuple(tr1.betas), eps=tr1.eps)
    opt.load_state_dict(osd)
    m0, v0 = tr1.m.clone(), tr1.v.clone()
    ck.from_torch_adam_state(tr1, osd)
    torch.cuda.synchronize()
    assert torch.equal(tr1.m, m0) and torch.equal(tr1.v, v0) and float(tr1.scal[2]) == 2.0


@pytest.mark.parametrize("name", ["sasrec_w50_h1", "sasrec_w100_h2"])
def test_predict_and_rank(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    V, L, d, H, nl = [int(x) for x in z["cfg"]]
    cfg = so.Cfg(V, L, d, H, nl, dropout=0.0)
    seed, B = int(z["seed"]), int(z["B"])
    P = so.init_params(cfg, seed=seed)
    batch = make_batch(np.random.RandomState(seed + 1), B, L, V)
    m = build(cfg, P, "f32")
    close(m.predict(None, batch[0], z["cand"]).cpu().numpy(), z["predict_cand"], 1e-4, "predict (fixture)")
    full = m.predict(None, batch[0], None, full=True).cpu().numpy()
    assert full.shape == (B, V + 1)
    want = so.predict(P, cfg, batch[0], np.tile(np.arange(V + 1), (B, 1)))
    close(full, want, 1e-4, "predict full")
    logits, rank = m.predict_rank(batch[0], z["cand"])
    lg = so.predict(P, cfg, batch[0], z["cand"])
    close(logits.cpu().numpy(), lg, 1e-4, "rank logits")
    assert list(rank.cpu().numpy()) == list(so.rank_of_first(lg))


def test_two_shards_equal_the_whole_batch():
    """The data-parallel decomposition at (50, 1): the global batch of 3 split 2 + 1 with global normalisers and global dropout
    indices (b_offset).  The two shards' gradients, summed -- what the flat all-reduce computes, pads (zeros) included -- equal the
    whole batch's.  Run in one process on one GPU; the collective itself is the unchanged code of adt_amd/dp.py."""
    V, L, d, H, nl, B, p = 50, 24, 50, 1, 2, 3, 0.5
    cfg = so.Cfg(V, L, d, H, nl, dropout=p)
    P = so.init_params(cfg, seed=5)
    batch = make_batch(np.random.RandomState(6), B, L, V)
    m = build(cfg, P, "f32", p)
    m.train()
    norms = torch.tensor([float(np.count_nonzero(batch[2])), B * L * d, B * L * H], device="cuda:0", dtype=torch.float32)

    def run(lo, hi):
        m.set_seed(777)
        slots = torch.zeros(2 + 2 * nl, 64, device="cuda:0")
        m.flat_grad.zero_()
        m.loss_forward_backward(tuple(m.ids(a[lo:hi]) for a in batch), LAM1, LAM2, norms, slots, b_offset=lo)
        torch.cuda.synchronize()
        return m.flat_grad.clone(), slots.sum(1).cpu().numpy()
    g, s = run(0, 3)
    g0, s0 = run(0, 2)
    g1, s1 = run(2, 3)
    assert float((g0 + g1 - g).abs().max()) <= 5e-5 * float(g.abs().max())     # tests/test_dp_gpu.py's gradient bound
    assert np.abs(s0 + s1 - s).max() <= 1e-5 * np.abs(s).max()
    assert float((g0 + g1)[pad_mask(m)].abs().max()) == 0.0


DP_WD = 1e-3


def _dp_case(init_seed):
    V, L, d, H, nl, B, p = 50, 24, 50, 1, 2, 3, 0.5
    cfg = so.Cfg(V, L, d, H, nl, dropout=p)
    m = build(cfg, so.init_params(cfg, seed=init_seed), "f32", p)
    m.train()
    return cfg, m, make_batch(np.random.RandomState(6), B, L, V)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from adt_amd.dp import shard_bounds, global_norms
    from adt_amd.sasrec.model_wide import WideSasrecTrainer
    cfg, m, batch = _dp_case(5 if rank == 0 else 77)        # rank 1 starts from other weights: everything comes from rank 0
    dist.broadcast(m.master, 0)                              # adt_amd/sasrec/main.py: the reference-shaped buffer travels, then push()
    m.push()
    tr = WideSasrecTrainer(m, LAM1, LAM2, lr=1e-3, weight_decay=DP_WD, clip=5.0, process_group=dist.group.WORLD, seed=5)
    lo, hi = shard_bounds(len(batch[0]), rank, world)
    assert (lo, hi) == ((0, 2), (2, 3))[rank]
    tr.step(*[a[lo:hi] for a in batch], norms=global_norms(batch[2], cfg.hidden_units, cfg.num_heads), b_offset=lo)   # the TRUE d = 50
    torch.cuda.synchronize()
    pads = pad_mask(m)
    zero = {nm: bool((t[pads].view(torch.int32) == 0).all()) for nm, t in (("flat", m.flat), ("flat_grad", m.flat_grad), ("exp_avg", tr.m), ("exp_avg_sq", tr.v))}
    w = m.ref_flat.clone()
    dist.all_reduce(w, op=dist.ReduceOp.MAX)                 # the ranks hold the same weights after the step
    same = bool(torch.equal(w, m.ref_flat))
    loss = float(tr.loss())                                  # a collective: every rank calls it
    if rank == 0:
        q.put((m.flat.cpu().numpy(), m.flat_grad.cpu().numpy(), m.ref_flat.cpu().numpy(), float(tr.grad_norm()), loss, zero, same))
    else:
        q.put(("rank1", same))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_trainer_matches_single_process():
    """tests/test_dp_gpu.py at (50, 1): two processes on cuda:0 with a gloo group, WideSasrecTrainer(process_group=...) on the shards
    2 + 1 of a global batch of 3, global normalisers with the true d, global dropout indices, the bucketed all-reduce of the PADDED
    gradient, clip + Adam after it, pull(); against the single-process step, with that test's bounds."""
    import torch.multiprocessing as mp
    from adt_amd.sasrec.model_wide import WideSasrecTrainer
    cfg, m, batch = _dp_case(5)
    tr = WideSasrecTrainer(m, LAM1, LAM2, lr=1e-3, weight_decay=DP_WD, clip=5.0, seed=5)
    tr.step(*batch)
    torch.cuda.synchronize()
    f1, g1, w1, n1, l1 = m.flat.cpu().numpy(), m.flat_grad.cpu().numpy(), m.ref_flat.cpu().numpy(), float(tr.grad_norm()), float(tr.loss())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300), q.get(timeout=300)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    r1 = [x for x in got if len(x) == 2][0]
    f2, g2, w2, n2, l2, zero, same = [x for x in got if len(x) == 7][0]
    print("grad norm %.7f / %.7f, loss %.7f / %.7f, max grad diff %.3g of %.3g, max weight diff %.3g"
          % (n1, n2, l1, l2, np.abs(g1 - g2).max(), np.abs(g1).max(), np.abs(w1 - w2).max()))
    assert same and r1[1], "the two ranks ended the step with different weights"
    assert all(zero.values()), zero
    assert abs(n1 - n2) <= 1e-4 * n1
    assert abs(l1 - l2) <= 1e-5 * abs(l1)
    assert np.abs(g1 - g2).max() <= 5e-5 * max(np.abs(g1).max(), 1e-6)
    for a, b, ga in ((w1, w2, m.compact(torch.from_numpy(g1).to(m.dev)).cpu().numpy()), (f1, f2, g1)):
        dlt = np.abs(a - b)
        noisy = np.abs(ga) < 1e-6           # Adam turns rounding noise on exactly-zero gradients into +-lr
        assert dlt.max() <= 2 * 1e-3 * 1.01 and dlt[~noisy].max() <= 3e-5


def test_main_with_default_width_end_to_end(tmp_path):
    """sasrec.main with its default --hidden_units 50 --num_heads 1 --maxlen 50 (none of them passed), graph replay on."""
    cmd = [sys.executable, "-m", "adt_amd.sasrec.main", "--dataset", "ml-1m", "--train_dir", "odd", "--data_dir", str(tmp_path / "data"), "--synthetic",
           "ml1m-small", "--no_template", "--batch_size", "128", "--num_epochs", "2", "--eval_interval", "1", "--use_graph", "true"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=480)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    recs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(recs) == 2, p.stdout[-2000:]
    print([r["loss"] for r in recs])
    assert all(np.isfinite(r["loss"]) for r in recs) and recs[1]["loss"] < recs[0]["loss"]
    for r in recs:
        for split in ("valid", "test"):
            assert 0.0 <= r[split]["ndcg10"] <= 1.0 and 0.0 <= r[split]["hr10"] <= 1.0 and np.isfinite(r[split]["auc"])


def test_multiples_of_64_are_untouched():
    from adt_amd.sasrec.model import param_table
    from adt_amd.wide import padded_layout
    assert padded_layout(256, 2) == (128, 128, 256) and padded_layout(64, 2) == (32, 32, 64)
    cfg = so.Cfg(50, 24, 256, 2, 1, dropout=0.0)
    m = build(cfg, None, "bf16")
    assert m.lanes is None and m.ref_flat is None and m.master is m.flat
    assert m.n_flat == sum((int(np.prod(s)) + 3) // 4 * 4 for _, s in param_table(50, 24, 256, 2, 1))
    assert m.P("item_emb.weight").data_ptr() == m.item_emb.weight.data_ptr()


def test_loop_reference_is_refused_for_padded_widths():
    from adt_amd._lib import AdtError
    cfg = so.Cfg(50, 24, 50, 1, 1, dropout=0.0)
    m = build(cfg, None, "f32")
    m.train()
    batch = make_batch(np.random.RandomState(1), 2, 24, 50)
    with pytest.raises(AdtError, match="loop fused"):
        m(None, *batch)
